"""CPU-side checks of the packed band kernel's instantiations for gap extensions of 3 and 4 (tests/band_deep_matrix.py): the table equals what the two
new objects hold, the fixture tests/golden/band_pen.jsonl (compiled reference, tests/golden/make_golden_band_pen.py) is reproduced by the oracle, and the
inputs of every cell hold what tests/test_band_deep_matrix_gpu.py relies on — sized from the oracle alone."""
import hashlib

import numpy as np
import pytest

import miniwfa_amd as mw
import band_matrix as bm
import band_deep_matrix as dm
from conftest import load_golden, golden_inputs

VEC = load_golden("band_pen.jsonl")


def cigar_matches(cig, exp) -> bool:
    """A CIGAR (uint32 words, or None) against a vector's expectation: the words themselves, or their count and SHA-256 where the CIGAR is long."""
    if exp["n_cigar"] is None:
        return cig is None or len(cig) == 0
    if cig is None or len(cig) != exp["n_cigar"]:
        return False
    if "cigar" in exp:
        return [int(w) for w in cig] == exp["cigar"]
    return hashlib.sha256(np.asarray(cig, dtype="<u4").tobytes()).hexdigest() == exp["cigar_sha256"]


@pytest.mark.parametrize("e1", [3, 4])
def test_table_equals_the_instantiations_in_the_new_objects(e1):
    """Per unit: fourteen kernels for each of its sets — (3,1) and (3,2); (4,1) — and exactly the entries of the table with that e1."""
    mw.lib()
    built = dm.object_instantiations(e1)
    if isinstance(built, str):
        pytest.skip(built)
    declared = dm.declared_instantiations(e1)
    assert len(declared) == (28 if e1 == 3 else 14) and len(dm.declared_instantiations()) == len(dm.MATRIX) == 42
    missing = sorted(dm.inst_id(i) for i in built - declared)
    stale = sorted(dm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without an entry: {missing}; entries without an instantiation: {stale}"


@pytest.mark.parametrize("e1", [3, 4])
def test_table_equals_the_kernels_in_the_device_code(e1):
    """... and what is compiled for the GPU: the kernels of the unit's gfx950 code object, which a dispatch arm that never runs would add to without
    leaving a host stub (an `if` on a macro's value instead of `#if`: a second copy of fourteen (3,2) kernels in the e1 = 4 unit, once)."""
    mw.lib()
    built = dm.device_instantiations(e1)
    if isinstance(built, str):
        pytest.skip(built)
    declared = dm.declared_instantiations(e1)
    missing = sorted(dm.inst_id(i) for i in built - declared)
    stale = sorted(dm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"device kernels without an entry: {missing}; entries without a device kernel: {stale}"


def test_the_public_matrix_is_untouched():
    """The private instance of band_matrix.py carries the new sets; the one every other test imports does not, and no instantiation is listed by both tables."""
    assert not set(dm.DEEP_PEN) & set(bm.PEN) and set(dm.DEEP_PEN) <= set(dm.base.PEN)
    assert not dm.declared_instantiations() & bm.declared_instantiations()
    assert all(not i.FOLD and not i.BI4 and (i.E1, i.E2) in ((3, 1), (3, 2), (4, 1)) for i in dm.declared_instantiations())
    assert [dm.crossover(dm.DEEP_PEN[k]) for k in ("e31", "e32", "e41")] == [10, 20, 7]


def test_fixture_covers_every_set():
    ids = {v["id"] for v in VEC}
    assert {f"band10k-{t}-{m}" for t in dm.DEEP_PEN for m in ("score", "cigar")} | {f"band3k-{t}-cigar" for t in dm.DEEP_PEN} <= ids
    assert {f"rec{i}-e31-{e}" for i in range(7) for e in ("chain", "auto")} <= ids
    for v in VEC:
        tag = v["id"].split("-")[1]
        assert {k: v["opt"][k] for k in ("x", "o1", "e1", "o2", "e2")} == dm.DEEP_PEN[tag], v["id"]
    assert sorted(v["tl"] for v in VEC if v["entry"] == "chain") == [5000] * 6 + [30000]


@pytest.mark.parametrize("vid", [v["id"] for v in VEC if v["entry"] == "exact"])
def test_oracle_matches_reference(oracle, vid):
    from oracle.pyoracle import make_opt
    v = next(x for x in VEC if x["id"] == vid)
    t, q = golden_inputs(v)
    s, n_iter, cig = oracle.align(t, q, make_opt(**v["opt"]))
    assert (s, n_iter) == (v["expect"]["s"], v["expect"]["n_iter"]), vid
    assert cigar_matches(cig, v["expect"]), vid


def test_every_cell_has_its_inputs(oracle, capsys):
    """Group sizes, the pair within a chunk of the admission limit, the kinds of pairs, and the share of width-fit candidates the hand-back rules drop
    (at most a quarter), for every geometry x set."""
    lines = []
    dm.self_check(oracle, log=lines.append)
    with capsys.disabled():
        print()
        for ln in lines:
            print("   " + ln)
