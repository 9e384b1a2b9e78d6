"""The packed band kernel's table form (mwf_band2_tab.hip: the first probe of the match extension on per-position 8-mer tables in LDS) on the inputs of
tests/band_tab_cases.py, whose properties tests/test_band_tab_cpu.py asserts.  Geometry forced to 512 threads on three and on four chunk slots, score-only and
with CIGAR: s, n_iter and the CIGAR words equal the oracle's and, bit for bit, those of the same align with "probe_table" 0; the launch record says which form ran."""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
import band_tab_cases as tc
import fuzzlib

pytestmark = pytest.mark.gpu

BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs")
TAB_LINE = re.compile(r"\[libmwf_hip\] band2 table probe: table (\d+) B, lds (\d+) B")


def run(pairs, slots, flag, capfd, probe_table=1, hooks=()):
    """One align on 512 threads x `slots` chunk slots: (s, n_iter, cigars | None, n_retries, band launches [(T, K, E1, E2, TB, S2, BI4, FOLD, pairs)], table lines [(table, lds)])."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in (("force_kind", 2), ("block", 512), ("band_pack", 1), ("band_fold", 1), ("wide_slots", slots), ("probe_table", probe_table)):
            eng.set(k, v)
        for k, v in hooks:
            eng.set(k, v)
        if flag:
            eng.set("tb_budget_mb", 1024)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=flag, **tc.DEFAULT))
        s, it, nc = b.results()
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if flag else None
        err = capfd.readouterr().err
        ls = [tuple(int(x) for x in m.groups()) for m in BAND_LINE.finditer(err)]
        tabs = [tuple(int(x) for x in m.groups()) for m in TAB_LINE.finditer(err)]
        out = (np.array(s).copy(), np.array(it).copy(), cig, int(eng.stats().n_retries), ls, tabs)
        b.free()
        return out
    finally:
        eng.close()


def check(got, exp, flag, label, pairs):
    """s, n_iter and — with CIGAR — the words against the oracle's, by tests/fuzzlib.py's comparison: every mismatching pair is listed."""
    bad = []
    fuzzlib.compare((got[0], got[1], got[2], None), exp, label, pairs, bad, False, check_cigar=bool(flag))
    assert not bad, bad[:8]


def same(a, b, flag, label):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (label, "s / n_iter differ between the two forms")
    if flag:
        assert a[2] == b[2], (label, "CIGAR words differ between the two forms")


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("name", tc.GROUPS)
def test_table_form(name, slots, flag, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = tc.group(name)
    exp = tc.expected(oracle, name)
    tab = run(pairs, slots, flag, capfd)
    plain = run(pairs, slots, flag, capfd, probe_table=0)
    label = f"{name} slots {slots} flag {flag}"
    # one launch each, of the instantiation asked for, no pair handed back (every pair fits both geometries: tests/test_band_tab_cpu.py)
    record = (512, slots, 2, 1, flag, 1, 0, 1, len(pairs))
    assert tab[4] == [record] and plain[4] == [record], (label, tab[4], plain[4])
    assert len(tab[5]) == 1 and plain[5] == [], (label, "which form ran", tab[5], plain[5])
    longest = max(len(t) + len(q) for t, q in pairs)
    assert tab[5][0][0] >= 2 * (longest + 258) and tab[5][0][0] % 16 == 0 and tab[5][0][1] > tab[5][0][0], (label, tab[5])
    assert tab[3] == 0 and plain[3] == 0, (label, "re-runs", tab[3], plain[3])
    check(tab, exp, flag, label + " table form", pairs)
    check(plain, exp, flag, label + " probe_table 0", pairs)
    same(tab, plain, flag, label)


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
def test_fall_back_when_the_table_does_not_fit(flag, oracle, capfd, monkeypatch):
    """The LDS budget lowered by the hook below what the pair's table and copies need: the plain form, wfa_band2_kernel, runs and answers the same."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pair = tc.fallback_pair()
    exp = tc.expected(oracle, "fallback")
    need = 2 * (len(pair[0]) + len(pair[1]) + 258)
    tab = run([pair], 3, flag, capfd)
    low = run([pair], 3, flag, capfd, hooks=(("probe_table_lds", need),))   # (the table alone fills it: the 2-bit copies no longer fit beside it)
    record = (512, 3, 2, 1, flag, 1, 0, 1, 1)
    assert tab[4] == [record] and len(tab[5]) == 1, (tab[4], tab[5])
    assert low[4] == [record] and low[5] == [], (low[4], low[5])
    check(tab, exp, flag, "fallback, table form", [pair])
    check(low, exp, flag, "fallback, budget lowered", [pair])
    same(tab, low, flag, "fallback")
