"""CPU-side checks of the whole-device kernel's table (tests/sys_matrix.py): its entries are exactly the instantiations of wfa_sys_kernel and
wfa_sys_seg_kernel in the two built objects, the inputs of every cell hold what tests/test_sys_matrix_gpu.py relies on — sized from the oracle alone, before any
GPU time is spent —, the restated host rules give known values, and the oracle reproduces the compiled reference under every penalty set those tests use
(tests/golden/sys_pen.jsonl)."""
import hashlib

import numpy as np
import pytest

import miniwfa_amd as mw
import sys_matrix as sm
from conftest import load_golden, golden_inputs
from oracle.pyoracle import make_opt

GOLDEN = load_golden("sys_pen.jsonl")


def test_table_equals_the_instantiations_in_the_objects():
    """Adding, removing or re-parameterising an instantiation without its entry fails here and names it."""
    mw.lib()   # (builds the library, and with it the objects, where that has not happened yet)
    built = sm.object_instantiations()
    if isinstance(built, str):
        pytest.skip(built)
    declared = sm.declared_instantiations()
    assert len(declared) == 48 == len(sm.MATRIX), "an instantiation is listed twice"
    missing = sorted(sm.inst_id(i) for i in built - declared)
    stale = sorted(sm.inst_id(i) for i in declared - built)
    assert not missing and not stale, f"instantiations without an entry: {missing}; entries without an instantiation: {stale}"


def test_limit_sets_sit_on_the_limit():
    assert all(sm.nH(sm.PEN[k]) == 256 and sm.coop_supported(sm.PEN[k]) for k in sm.RING256)
    assert all(sm.nH(p) == 257 and not sm.coop_supported(p) for p in sm.PEN_BEYOND.values())
    assert sorted(sm.ext(p) for p in sm.PEN_BEYOND.values()) == [(1, 1), (2, 1), (2, 2), (3, 1), (4, 2)]


def test_restated_host_rules_on_known_values():
    """Worked out from mwf_plan.cpp by hand: 256 chunk slots of 48 / 240 owned columns; the first pass's estimate; the groups of a batch on 256 CUs."""
    assert (sm.owned_cols(1), sm.owned_cols(4)) == (48, 240)
    assert sm.window_cap(1) == 252 * 48 - 530 == 11566 and sm.window_cap(4) == 252 * 240 - 530
    assert sm.est1(18000) == 8192 and sm.est1(40000) == 8192 and sm.est1(60000) == 12000 and sm.est1(5000) == 5001
    assert sm.auto_c(sm.PEN["default"], 40000, 0)[0] == 1 and sm.auto_c(sm.PEN["default"], 60000, 0)[0] == 4
    assert sm.est2(sm.PEN["default"], 40000, 5000) == 2 * (5000 + 34) + 8 and sm.auto_c(sm.PEN["default"], 40000, 5745)[1] == 1 and sm.auto_c(sm.PEN["default"], 40000, 5746)[1] == 4
    assert sm.coop_group_size(256, 12000, False) == 16 and sm.coop_group_size(16, 12000, True) == 16 and sm.coop_group_size(256, 12000, True) == 64
    assert sm.side_by_side([100] * 30, 256) == [(16, 16), (14, 16)] and sm.side_by_side([100] * 17, 256) == [(16, 16), (1, 64)]
    assert sm.side_by_side([100, 200, 300], 16) == [(1, 16)] * 3
    # sixteen pairs side by side take the two-pass form under the default budget; the table's walk runs set a budget that keeps the walk
    assert sm.two_pass_rule(12000, 16, 1, 0) and sm.two_pass_rule(12000, 16, 4, 0) and not sm.two_pass_rule(12000, 1, 1, 0)
    assert not sm.two_pass_rule(20000, 16, 1, sm.WALK_BUDGET_MB) and sm.two_pass_rule(0, 1, 4, 1)


def test_restated_chunk_rule_on_known_windows():
    """sys_pass's gA / gB / n_ep on hand-made traces: a window of one column at the origin, and one that spans a whole 5200 x 3900 matrix."""
    tl, ql = 5200, 3900
    one = np.zeros((10, 2), dtype=np.int32)
    assert sm.epoch_chunks(one, tl, ql, 4) == [(5201 + 265) // 240 - (5201 - 265) // 240 + 1]
    full = np.tile(np.array([[-tl, ql]], dtype=np.int32), (600, 1))
    assert sm.epoch_chunks(full, tl, ql, 1)[1] == (tl + ql + 1) // 48 + 1 and sm.chunks_fit(full, tl, ql, 1) and not sm.chunks_overflow(full, tl, ql, 1)
    wide = np.tile(np.array([[-9000, 9000]], dtype=np.int32), (600, 1))
    assert sm.chunks_overflow(wide, 9000, 9000, 1) and sm.chunks_fit(wide, 9000, 9000, 4)


def test_every_cell_has_its_inputs(oracle, capsys):
    """Group sizes, the kinds of pairs, the pairs either side of a ring's wrap, the overflow groups of the C = 1 cells, and the share of candidates the margin
    leaves out (none for C = 4), for every (penalty set, columns per lane) of the table."""
    lines = []
    sm.self_check(oracle, log=lines.append)
    with capsys.disabled():
        print()
        for ln in lines:
            print("   " + ln)


def test_oracle_reproduces_the_reference_under_the_tables_penalty_sets(oracle):
    """Every set of the table and of the limit has its rows — score, CIGAR and low-memory —, and the oracle reproduces each: s, n_iter, the CIGAR."""
    sets = {**sm.PEN, **sm.PEN_BEYOND}
    key = lambda o: tuple(o[k] for k in ("x", "o1", "e1", "o2", "e2"))
    have = {key(v["opt"]) for v in GOLDEN}
    assert have == {key(p) for p in sets.values()}
    for k in have:
        mine = [v for v in GOLDEN if key(v["opt"]) == k]
        assert {(v["opt"]["flag"], v["opt"]["step"] > 0) for v in mine} == {(0, False), (1, False), (1, True)}, k
        assert any(v["opt"]["step"] > 0 and v["expect"]["s"] >= v["opt"]["step"] for v in mine), k   # (a low-memory vector that takes no snapshot tests nothing)
    assert any(v["expect"]["s"] > 512 for v in GOLDEN)
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
