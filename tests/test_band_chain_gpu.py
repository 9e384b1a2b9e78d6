"""The table form's chunk chain (mwf_band2_kernel.h, kChain / kGeo: per-slot probe geometry in registers, the interior chunk as a straight line) on the inputs of
tests/band_chain_cases.py, whose properties tests/test_band_chain_cpu.py asserts.  Geometry forced to 512 threads on three and on four chunk slots, score-only and
with CIGAR, "probe_table" 1: s, n_iter and the CIGAR words equal the oracle's and, bit for bit, those of the same align with "probe_table" 0 (the plain form
recomputes the geometry every penalty); one launch, no pair handed back, and the launch record names the table form."""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
import band_chain_cases as cc
import fuzzlib

pytestmark = pytest.mark.gpu

BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs")
TAB_LINE = re.compile(r"\[libmwf_hip\] band2 table probe: table (\d+) B, lds (\d+) B")


def run(pairs, slots, flag, capfd, probe_table, **kw):
    """One align on 512 threads x `slots` chunk slots: (s, n_iter, cigars | None, n_retries, band launches, table lines)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in (("force_kind", 2), ("block", 512), ("band_pack", 1), ("band_fold", 1), ("wide_slots", slots), ("probe_table", probe_table)):
            eng.set(k, v)
        if flag:
            eng.set("tb_budget_mb", 1024)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=flag, **cc.DEFAULT, **kw))
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


def both_forms(pairs, exp, slots, flag, capfd, label, stopped=False, **kw):
    tab = run(pairs, slots, flag, capfd, 1, **kw)
    plain = run(pairs, slots, flag, capfd, 0, **kw)
    # one launch each, of the instantiation asked for, no pair handed back or left out (every pair fits both geometries: tests/test_band_chain_cpu.py)
    record = (512, slots, 2, 1, flag, 1, 0, 1, len(pairs))
    assert tab[4] == [record] and plain[4] == [record], (label, tab[4], plain[4])
    assert len(tab[5]) == 1 and plain[5] == [], (label, "which form ran", tab[5], plain[5])
    assert tab[3] == 0 and plain[3] == 0, (label, "re-runs", tab[3], plain[3])
    assert len(tab[0]) == len(plain[0]) == len(exp) == len(pairs), label
    for got, form in ((tab, "table form"), (plain, "probe_table 0")):
        if stopped:   # (as tests/test_band_epoch_gpu.py compares a stopped pair: s, n_iter, and the words the oracle gives, if any)
            for i, (es, eit, ecig) in enumerate(exp):
                assert (int(got[0][i]), int(got[1][i])) == (es, eit), (label, form, i, (int(got[0][i]), int(got[1][i])), (es, eit))
                if flag:
                    assert got[2][i] == (ecig or []), (label, form, i, "CIGAR")
        else:
            bad = []
            fuzzlib.compare((got[0], got[1], got[2], None), exp, f"{label} {form}", pairs, bad, False, check_cigar=bool(flag))
            assert not bad, bad[:8]
    assert np.array_equal(tab[0], plain[0]) and np.array_equal(tab[1], plain[1]), (label, "s / n_iter differ between the two forms")
    if flag:
        assert tab[2] == plain[2], (label, "CIGAR words differ between the two forms")


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("name", cc.GROUPS)
def test_chunk_chain(name, slots, flag, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    both_forms(cc.group(oracle, name), cc.expected(oracle, name), slots, flag, capfd, f"{name} slots {slots} flag {flag}")


@pytest.mark.parametrize("flag", [0, 1], ids=["score", "cigar"])
@pytest.mark.parametrize("slots", [3, 4])
def test_stop_where_a_wave_runs_two_chunks(slots, flag, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    pair, kw, s_star = cc.stop_case(oracle)
    both_forms([pair], cc.expected(oracle, "stop", **kw), slots, flag, capfd, f"stop at {s_star} slots {slots} flag {flag}", stopped=True, **kw)
