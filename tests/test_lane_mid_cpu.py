"""CPU-side checks of the lane / mid kernel table (tests/lane_mid_matrix.py): its entries are exactly the instantiations of wfa_lane_kernel and
wfa_mid_kernel in the built objects, the inputs of every cell hold what tests/test_lane_mid_matrix_gpu.py relies on — sized from the oracle alone, before any
GPU time is spent — and the oracle reproduces the compiled reference under every penalty set those tests use (tests/golden/lane_mid_pen.jsonl)."""
import hashlib

import numpy as np
import pytest

import miniwfa_amd as mw
import lane_mid_matrix as lm
from conftest import load_golden, golden_inputs
from oracle.pyoracle import make_opt

GOLDEN = load_golden("lane_mid_pen.jsonl")


@pytest.mark.parametrize("kernel,n", [("lane", 6), ("mid", 18)])
def test_table_equals_the_instantiations_in_the_object(kernel, n):
    """Adding, removing or re-parameterising an instantiation without its entry fails here and names it."""
    mw.lib()   # (builds the library, and with it the objects, where that has not happened yet)
    built = lm.object_instantiations(kernel)
    if isinstance(built, str):
        pytest.skip(built)
    declared = lm.declared_instantiations(kernel)
    assert len(declared) == n == sum(c.kernel == kernel for c in lm.MATRIX), "an instantiation is listed twice"
    missing = sorted(lm.inst_id(i) for i in built - declared)
    stale = sorted(lm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without an entry: {missing}; entries without an instantiation: {stale}"


def test_limit_sets_sit_on_the_limits():
    d, m = lm.PEN["lane_deep"], lm.PEN["mid_deep"]
    assert lm.nH(d) + 2 * d["e1"] + 2 * d["e2"] == 96 and lm.lane_supported(d) and not lm.lane_supported(lm.PEN_BEYOND["lane_97"])
    assert lm.nH(m) == 64 and lm.mid_supported(m)
    assert [lm.mid_supported(lm.PEN_BEYOND[k]) for k in ("mid_nH65", "mid_e1_9", "mid_e2_9")] == [False] * 3
    assert {p["e1"] for p in lm.EDGE_PEN.values()} == {1, 2, 3, 8} and {p["e2"] for p in lm.EDGE_PEN.values()} == {1, 2, 8}


def test_restated_lds_rules_on_known_layouts():
    """mid_layout / lane_lds_bytes restated in Python, on values worked out from the sources by hand: the default set on a 64-column span (27 rows of 72 entries,
    17 good words, 17 windows, 48 bytes of bookkeeping) and the lane kernel's deepest rings on four chunks (96 rows of 130 dwords)."""
    p = lm.PEN["default"]
    assert lm.mid_seq_off(p, 64) == 27 * 72 * 2 + 17 * 8 + 17 * 8 + 48 + 0 == 4208
    assert lm.lane_lds_bytes(lm.PEN["lane_deep"], 4, 0) == 96 * 130 * 4 + 64


def test_every_cell_has_its_inputs(oracle, capsys):
    """Group sizes, the pair within a chunk / group of the limit, the kinds of pairs, the pairs at the lane kernel's penalty limit, and the share of candidates the
    forecast's margin leaves out (at most a quarter; none for the lane kernel), for every run of every cell."""
    lines = []
    lm.self_check(oracle, log=lines.append)
    with capsys.disabled():
        print()
        for ln in sorted(set(lines)):
            print("   " + ln)


def test_oracle_reproduces_the_reference_under_the_tables_penalty_sets(oracle):
    """Every set of the table, of the limits and of the edge tests has its rows, and the oracle reproduces each: s, n_iter, the CIGAR."""
    sets = {**lm.PEN, **lm.PEN_BEYOND, **lm.EDGE_PEN}
    have = {tuple(v["opt"][k] for k in ("x", "o1", "e1", "o2", "e2")) for v in GOLDEN}
    assert have == {tuple(p[k] for k in ("x", "o1", "e1", "o2", "e2")) for p in sets.values()}
    assert any(v["expect"]["s"] > 512 for v in GOLDEN) and any(v["tl"] <= 300 for v in GOLDEN) and len(GOLDEN) >= 4 * len(have)
    for v in GOLDEN:
        t, q = golden_inputs(v)
        s, n_iter, cig = oracle.align(t, q, make_opt(**v["opt"]))
        exp = v["expect"]
        assert (s, n_iter) == (exp["s"], exp["n_iter"]), v["id"]
        assert (None if cig is None else len(cig)) == exp["n_cigar"], v["id"]
        if cig is not None and "cigar" in exp:
            assert [int(w) for w in cig] == exp["cigar"], v["id"]
        elif cig is not None:
            assert hashlib.sha256(np.asarray(cig, dtype="<u4").tobytes()).hexdigest() == exp["cigar_sha256"], v["id"]
