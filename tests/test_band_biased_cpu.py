"""CPU-side checks of the packed band kernel's copies on biased offsets for the sets beyond (2,1) (tests/band_biased_matrix.py): the table equals what the two
new objects hold — host stubs and gfx950 kernels —, no instantiation is listed by two tables, the fixture tests/golden/band_biased.jsonl (compiled reference,
tests/golden/make_golden_band_biased.py) is reproduced by the oracle, and the inputs of every cell hold what tests/test_band_biased_matrix_gpu.py relies on —
sized from the oracle alone."""
import pytest

import miniwfa_amd as mw
import band_matrix as bm
import band_deep_matrix as dm
import band_biased_matrix as xm
from conftest import load_golden, golden_inputs
from test_band_deep_cpu import cigar_matches

VEC = load_golden("band_biased.jsonl")
N_KERNELS = {"bi": 12, "bi_deep": 12}   # (2,2): 2 slot counts x TB x FOLD = 8, every other set 2 x TB = 4


@pytest.mark.parametrize("unit", sorted(xm.BIASED_OBJS))
def test_table_equals_the_instantiations_in_the_new_objects(unit):
    """Per unit: exactly the entries of the table that name it.  The objects are the library's own: once mw.lib() has built it they are there, and a tree
    without the units fails here."""
    mw.lib()
    built = xm.object_instantiations(unit)
    assert not isinstance(built, str), built
    declared = xm.declared_instantiations(unit)
    assert len(declared) == N_KERNELS[unit] and len(xm.declared_instantiations()) == len(xm.MATRIX) == sum(N_KERNELS.values())
    missing = sorted(xm.inst_id(i) for i in built - declared)
    stale = sorted(xm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without an entry: {missing}; entries without an instantiation: {stale}"


@pytest.mark.parametrize("unit", sorted(xm.BIASED_OBJS))
def test_table_equals_the_kernels_in_the_device_code(unit):
    """... and what is compiled for the GPU: the kernels of the unit's gfx950 code object (a dispatch arm that never runs leaves no host stub but still
    instantiates its kernels on the device side)."""
    mw.lib()
    built = xm.device_instantiations(unit)
    assert not isinstance(built, str), built
    declared = xm.declared_instantiations(unit)
    missing = sorted(xm.inst_id(i) for i in built - declared)
    stale = sorted(xm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"device kernels without an entry: {missing}; entries without a device kernel: {stale}"


def test_no_instantiation_is_listed_twice_and_the_other_tables_are_untouched():
    """The three tables are disjoint; the private instance carries the new sets and the opened class rule, the public one and the deep module's do not."""
    a, b, c = bm.declared_instantiations(), dm.declared_instantiations(), xm.declared_instantiations()
    assert not (a & b) and not (a & c) and not (b & c)
    assert len(a) == 62 and len(b) == 42 and len(c) == 24
    assert all(i.T == 512 and i.K in (5, 6) and i.BI4 and i.S2 and (i.FOLD == 0 or (i.E1, i.E2) == (2, 2)) for i in c)
    assert {(i.E1, i.E2) for i in c} == {(2, 2), (1, 1), (3, 1), (3, 2), (4, 1)}
    assert not set(dm.DEEP_PEN) & set(bm.PEN) and set(dm.DEEP_PEN) <= set(xm.base.PEN)
    # the class rule: a 10 kb pair under -a is class 14 for the private instance alone; (2,1) is class 14 for all three
    p = bm.PEN["a22"]
    assert xm.base.host_class(p, 10000, 10000) == 14 and bm.host_class(p, 10000, 10000) == 13 and dm.base.host_class(p, 10000, 10000) == 13
    assert xm.base.host_class(bm.PEN["default"], 17800, 17800) == bm.host_class(bm.PEN["default"], 17800, 17800) == 14
    # the guard rails the rule keeps: three slots, the span geometry for everything, (4,2)
    assert xm.base.host_class(p, 10000, 10000, wide_slots=3) == 13 and xm.base.host_class(p, 10000, 10000, band_span=2) == 13
    assert xm.base.host_class(dm.NOT_BUILT_PEN["e42"], 10000, 10000) == 13


def test_fixture_covers_every_set():
    ids = {v["id"] for v in VEC}
    assert {f"biased12k-{t}-{m}" for t in xm.BUILT for m in ("score", "cigar")} | {f"biased{n}-a22-{m}" for n in ("7k", "10k") for m in ("score", "cigar")} == ids
    for v in VEC:
        tag = v["id"].split("-")[1]
        assert {k: v["opt"][k] for k in ("x", "o1", "e1", "o2", "e2")} == xm.PEN[tag], v["id"]
        # every vector is a pair past plain 16-bit offsets that the class rule gives to the copies
        assert v["tl"] + xm.base.penalty_bound(xm.PEN[tag], v["tl"], v["ql"]) >= 32767 and xm.base.host_class(xm.PEN[tag], v["tl"], v["ql"]) == 14, v["id"]


@pytest.mark.parametrize("vid", [v["id"] for v in VEC])
def test_oracle_matches_reference(oracle, vid):
    from oracle.pyoracle import make_opt
    v = next(x for x in VEC if x["id"] == vid)
    t, q = golden_inputs(v)
    s, n_iter, cig = oracle.align(t, q, make_opt(**v["opt"]))
    assert (s, n_iter) == (v["expect"]["s"], v["expect"]["n_iter"]), vid
    assert cigar_matches(cig, v["expect"]), vid


def test_every_cell_has_its_inputs(oracle, capsys):
    """Group sizes, the pair within a chunk of the admission limit, the kinds of pairs, and the share of width-fit candidates the hand-back rules drop
    (at most a quarter), for both geometries x every set."""
    lines = []
    xm.self_check(oracle, log=lines.append)
    with capsys.disabled():
        print()
        for ln in lines:
            print("   " + ln)
