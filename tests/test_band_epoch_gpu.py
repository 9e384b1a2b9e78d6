"""The packed band kernel's window epoch (mwf_band2_kernel.h: a penalty whose window meets the same chunks as the last one reuses the slot state of the last full
header) on the inputs at which a stale cache would show — tests/band_epoch_cases.py, whose properties tests/test_band_epoch_cpu.py asserts.  s, n_iter and
the CIGAR words equal the oracle's; the launch record names the geometry the case was built for."""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, synth_pair
from oracle.pyoracle import make_opt
import band_matrix as bm
import band_epoch_cases as ec

pytestmark = pytest.mark.gpu

BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs")
_expected: dict = {}


def expected(orc, key, pairs, pen, **kw):
    """[(s, n_iter, cigar)] with CIGAR, computed once per case (s and n_iter of a score-only run are the same)."""
    if key not in _expected:
        _expected[key] = orc.align_many(pairs, make_opt(flag=1, **pen, **kw), threads=bm.ORACLE_THREADS)[0]
    return _expected[key]


def run(pairs, tunables, pen, flag, capfd, aligns=1, **kw):
    """`aligns` aligns of one upload: [(s, n_iter, cigars | None, n_retries, band launches [(T, K, TB, BI4, FOLD, pairs)])]."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    out = []
    try:
        for k, v in tunables:
            eng.set(k, v)
        if flag:
            eng.set("tb_budget_mb", 1024)
        b = eng.upload(pk)
        for _ in range(aligns):
            capfd.readouterr()
            b.align(mw.opt_init(flag=flag, **pen, **kw))
            s, it, nc = b.results()
            cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if flag else None
            err = capfd.readouterr().err
            ls = [(int(m.group(1)), int(m.group(2)), int(m.group(5)), int(m.group(7)), int(m.group(8)), int(m.group(9))) for m in BAND_LINE.finditer(err)]
            out.append((np.array(s).copy(), np.array(it).copy(), cig, int(eng.stats().n_retries), ls))
        b.free()
    finally:
        eng.close()
    return out


def check(got, exp, flag, label):
    s, it, cig = got[:3]
    for i, (es, eit, ecig) in enumerate(exp):
        assert (int(s[i]), int(it[i])) == (es, eit), (label, "pair", i, (int(s[i]), int(it[i])), (es, eit))
        if flag:
            assert cig[i] == (ecig or []), (label, "pair", i, "CIGAR")


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_epoch_case(name, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    c = ec.case(oracle, name)
    g = ec.GEOM[c.nwk]
    exp = expected(oracle, name, c.pairs, c.pen)
    for flag in (0, 1):
        got, = run(c.pairs, ec.tunables(c.nwk, c.band_fold), c.pen, flag, capfd)
        ls = got[4]
        fold = int(bool(c.band_fold and bm.pen_folds(c.pen) and g.T >= 512))   # (the CIGAR twin folds too: the forward bits)
        assert ls and ls[0] == (g.T, g.K, flag, 0, fold, len(c.pairs)), (name, flag, ls)
        assert got[3] == 0 and len(ls) == 1, (name, flag, "a pair the geometry finishes was handed back", got[3], ls)
        check(got, exp, flag, f"{name} flag {flag}")


@pytest.mark.parametrize("name", ec.STOP_NAMES)
def test_stop_at_an_epoch_change(name, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    _, nwk, pair, kw, s_star = ec.stop_case(oracle, name)
    g = ec.GEOM[nwk]
    exp = expected(oracle, name, [pair], ec.DEFAULT, **kw)
    for flag in (0, 1):
        got, = run([pair], ec.tunables(nwk, 1), ec.DEFAULT, flag, capfd, **kw)
        assert got[4] and got[4][0][:3] == (g.T, g.K, flag), (name, got[4])
        check(got, exp, flag, f"{name} flag {flag} stop at {s_star}")


def test_handed_back_where_the_window_first_meets_too_many_chunks(oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    for nwk, pairs, where in ec.overflow_cases(oracle):
        g = ec.GEOM[nwk]
        exp = expected(oracle, ("overflow", nwk), pairs, ec.DEFAULT)
        for flag in (0, 1):
            got, = run(pairs, ec.tunables(nwk, 1), ec.DEFAULT, flag, capfd)
            ls = got[4]
            assert ls and ls[0][:3] == (g.T, g.K, flag) and ls[0][5] == len(pairs), (nwk, flag, ls)
            # every pair is handed back by the chunk rule and re-run ONCE: the estimate it is handed back with sends it to a kernel that finishes it (the count the
            # kernel gave before the window epoch: 6 of 6 on each of the three geometries, score-only and with CIGAR)
            assert got[3] == len(pairs) == ec.MAX_PER_CASE, (nwk, flag, got[3], where)
            check(got, exp, flag, f"overflow nwk {nwk} flag {flag}")


def test_three_slot_note_of_the_four_slot_form(oracle, capfd, monkeypatch):
    """Default routing (wide_slots 0): the first align of a batch of the 512-thread class runs on four slots and notes whether three would have held every
    pair; the second align returns to three slots when they would, and stays on four when one pair's window met more than 23 chunks.  Read from the launch
    record.  (A note set for nothing would keep the narrow batch on four slots; a note lost would re-run the wide pair.)"""
    monkeypatch.setenv("MWF_DEBUG", "1")
    narrow, wide = ec.note_batches(oracle)
    for label, pairs, k_second in (("narrow", narrow, 3), ("wide", wide, 4)):
        exp = expected(oracle, ("note", label), pairs, ec.DEFAULT)
        first, second = run(pairs, bm.COMMON_DEFAULT_ROUTING, ec.DEFAULT, 0, capfd, aligns=2)
        assert first[4] and first[4][0][:2] == (512, 4) and first[4][0][5] == len(pairs), (label, first[4])
        assert second[4] and second[4][0][:2] == (512, k_second) and second[4][0][5] == len(pairs), (label, second[4])
        assert first[3] == 0 and second[3] == 0 and len(first[4]) == 1 and len(second[4]) == 1, (label, first[3], second[3], first[4], second[4])
        check(first, exp, 0, f"note {label} first align")
        check(second, exp, 0, f"note {label} second align")


def test_byte_wise_768_threads(oracle, capfd, monkeypatch):
    """NW = 12: the priority rule's other branch; a base outside A/C/G/T keeps the pair on the byte-wise copy."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    t, q = synth_pair(93000, 2400, 0.12)
    t = t[:700] + b"N" + t[701:]
    rng = np.random.default_rng(931)
    pairs = [(t, q), (bm._rand(rng, 895), bm._rand(rng, 930))]
    exp = expected(oracle, "768", pairs, ec.DEFAULT)
    for flag in (0, 1):
        got, = run(pairs, bm.tunables(ec.G768, 1), ec.DEFAULT, flag, capfd)
        assert got[4] and got[4][0][:3] == (768, 2, flag), got[4]
        check(got, exp, flag, f"768 flag {flag}")


@pytest.mark.parametrize("key", [(512, 5, 1), (1024, 5, 0)], ids=["biased-512x5", "span-1024x5"])
def test_biased_and_span_geometries(key, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    g = bm.GEOMS[key]
    pairs = [synth_pair(94000 + key[0], g.L, 0.02)]
    assert bm.host_admits(g, ec.DEFAULT, len(pairs[0][0]), len(pairs[0][1]))
    exp = expected(oracle, key, pairs, ec.DEFAULT)
    got, = run(pairs, bm.tunables(g, 1), ec.DEFAULT, 0, capfd)
    assert got[4] and got[4][0][:2] == (g.T, g.K) and got[4][0][3] == g.BI4, got[4]
    check(got, exp, 0, f"{key}")
