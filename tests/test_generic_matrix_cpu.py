"""CPU-side checks of the generic kernel's table (tests/generic_matrix.py): its entries are exactly the instantiations of wfa_batch_kernel and
wfa_bigring_kernel in the built object, the inputs of every cell hold what tests/test_generic_matrix_gpu.py relies on — checked from the lengths, the plan's
rules restated and the oracle's band trace, before any GPU time is spent — and the oracle reproduces the compiled reference under every penalty set and mode
those tests use (tests/golden/generic_pen.jsonl)."""
import hashlib

import numpy as np
import pytest

import miniwfa_amd as mw
import generic_matrix as gm
from conftest import load_golden, golden_inputs
from oracle.pyoracle import make_opt

GOLDEN = load_golden("generic_pen.jsonl")
PEN_KEYS = ("x", "o1", "e1", "o2", "e2")


def test_table_equals_the_instantiations_in_the_object():
    """Adding, removing or re-parameterising an instantiation without its entry fails here and names it.  (The four LDS2 forms no route launched — 512 threads on
    32-bit rows, 512 with traceback and 768 score-only on 16-bit rows — are no longer built: run_batch_kernel takes 768 threads unless the rows are 16 bits wide and
    the run is score-only.)"""
    mw.lib()   # (builds the library, and with it the objects, where that has not happened yet)
    built = gm.object_instantiations()
    if isinstance(built, str):
        pytest.skip(built)
    declared = gm.declared_instantiations()
    assert len(declared) == 15 == len(gm.MATRIX), "an instantiation is listed twice"
    missing = sorted(gm.inst_id(i) + str(tuple(i)) for i in built - declared)
    stale = sorted(gm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without an entry: {missing}; entries without an instantiation: {stale}"


def test_penalty_sets_sit_where_the_table_says():
    P = gm.PEN
    assert gm.nH(P["edit"]) == 2 and gm.nH(P["ring256"]) == 256 and gm.nH(P["ring257"]) == 257
    assert P["o1zero"]["o1"] == 0 and P["edit"]["x"] == P["edit"]["o1"] + P["edit"]["e1"]           # aliasing source slices: j1 == jg1, jx == j1
    assert P["e33"]["e1"] == P["e33"]["e2"] and P["e2gt"]["e2"] > P["e2gt"]["e1"] and gm.nH(P["xdeep"]) == P["xdeep"]["x"] + 1
    assert gm.n_slices(P["default"]) == 17 + 6 + 4 and gm.n_slices(P["e88"]) == 29 + 18 + 18
    assert {P[n]["e2"] for n in gm.BIG_SETS} == {1, 2} and {P[n]["e1"] for n in gm.BIG_SETS} == {2, 3}
    for n in gm.FAST_SETS:   # the low-memory steps around the ring's depth, and no step twice
        steps = [m[1]["step"] for m in gm.modes(n) if "step" in m[1] and m[2] == "low"]
        assert len(steps) == len(set(steps)) and gm.nH(P[n]) in steps and 97 in steps and (gm.nH(P[n]) - 1 in steps or n == "edit"), (n, steps)


def test_every_cell_has_its_inputs(oracle, capsys):
    """One launch per run (the low-memory batches hold no pair below the step), the wide form's rule on every LDS2 batch, A/C/G/T only and no possible 16-bit overflow
    where the rows are 16 bits wide, targets on both sides of a chunk edge — and, from the oracle's band trace, that the 8400 x 8400 pair's window hands E2/F2 over from
    LDS to HBM and back under the three sets said to, and never under the edit set."""
    lines = []
    for c in gm.MATRIX:
        gm.check_cell_inputs(oracle, c, log=lines.append)
    with capsys.disabled():
        print()
        for ln in sorted(set(lines)):
            print("   " + ln)


def test_oracle_reproduces_the_reference_under_the_tables_sets_and_modes(oracle):
    """Every (set, mode) of the table has its rows, and the oracle reproduces each: s, n_iter, the CIGAR."""
    have = {(tuple(v["opt"][k] for k in PEN_KEYS), v["opt"]["flag"], v["opt"]["step"], v["opt"]["max_s"], v["opt"]["max_iter"]) for v in GOLDEN}
    want = set()
    for name, p in gm.PEN.items():
        for _, okw, _ in gm.all_modes(name):
            want.add((tuple(p[k] for k in PEN_KEYS), okw.get("flag", 0), okw.get("step", 0), okw.get("max_s", 0), okw.get("max_iter", 0)))
    assert have == want and len(GOLDEN) >= 2 * len(want)
    assert any(v["expect"]["s"] > 512 for v in GOLDEN) and any(v["tl"] <= gm.SMALL_MAX for v in GOLDEN)
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
