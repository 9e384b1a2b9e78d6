"""The table form's second fold (miniwfa_amd/csrc/mwf_band2_tab2.hip; mwf_band2_kernel.h, kFold2) on the inputs of tests/band_fold2_cases.py, whose properties
tests/test_band_fold2_cpu.py asserts.  Geometry forced to 512 threads on three and on four chunk slots, score-only: s and n_iter equal the oracle's and, bit for
bit, those of the same align with "band_fold2" 0 (the table form: the row of lag o2 + e2 loaded in front of the recurrence); one launch, no pair handed back, and the
launch record names the form that ran.  A penalty set the routing rule refuses launches the table form, and so does "band_fold2" 0."""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
import band_fold2_cases as fc

pytestmark = pytest.mark.gpu

BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs")
TAB_LINE = re.compile(r"\[libmwf_hip\] band2 table probe: table (\d+) B, lds (\d+) B")
FOLD2_LINE = re.compile(r"\[libmwf_hip\] band2 second fold: wfa_band2_tab2_kernel, row of lag (\d+) folded one penalty ahead \(o2 \+ e2 (\d+), bound (\d+)\)")


def run(pairs, slots, capfd, fold2, pen=fc.DEFAULT, **kw):
    """One score-only align on 512 threads x `slots` chunk slots: (s, n_iter, n_retries, band launches, table lines, second-fold lines)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in (("force_kind", 2), ("block", 512), ("band_pack", 1), ("band_fold", 1), ("wide_slots", slots), ("probe_table", 1), ("band_fold2", fold2)):
            eng.set(k, v)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=0, **pen, **kw))
        s, it, _ = b.results()
        err = capfd.readouterr().err
        out = (np.array(s).copy(), np.array(it).copy(), int(eng.stats().n_retries), [tuple(int(x) for x in m.groups()) for m in BAND_LINE.finditer(err)],
               [tuple(int(x) for x in m.groups()) for m in TAB_LINE.finditer(err)], [tuple(int(x) for x in m.groups()) for m in FOLD2_LINE.finditer(err)])
        b.free()
        return out
    finally:
        eng.close()


def both(pairs, exp, slots, capfd, label, pen=fc.DEFAULT, takes=True, **kw):
    assert 0 < len(pairs) <= 64 and len(exp) == len(pairs), label
    on, off = run(pairs, slots, capfd, 1, pen, **kw), run(pairs, slots, capfd, 0, pen, **kw)
    record = (512, slots, 2, 1, 0, 1, 0, 1, len(pairs))
    assert on[3] == [record] and off[3] == [record], (label, on[3], off[3])
    assert len(on[4]) == 1 and len(off[4]) == 1, (label, "both are launches of the table probe", on[4], off[4])
    lag = (pen["o2"], pen["o2"] + pen["e2"], fc.FOLD2_MAX_LAG)
    assert on[5] == ([lag] if takes else []) and off[5] == [], (label, "which form ran", on[5], off[5])
    assert on[2] == 0 and off[2] == 0, (label, "re-runs", on[2], off[2])
    for got, form in ((on, "band_fold2 1"), (off, "band_fold2 0")):
        bad = [(i, (int(got[0][i]), int(got[1][i])), (e[0], e[1])) for i, e in enumerate(exp) if (int(got[0][i]), int(got[1][i])) != (e[0], e[1])]
        assert not bad, (label, form, len(bad), bad[:6])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]), (label, "s / n_iter differ between the two forms")


@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("name", fc.GROUPS)
def test_second_fold(name, slots, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs, exp = fc.group(oracle, name), fc.expected(oracle, name)
    if name == "fuzz":   # (the few pairs a geometry of 24 chunks may hand back are left out: tests/test_band_fold2_cpu.py counts them)
        keep = fc.fits_both(oracle, pairs)
        pairs, exp = [p for p, k in zip(pairs, keep) if k], [e for e, k in zip(exp, keep) if k]
    both(pairs, exp, slots, capfd, f"{name} slots {slots}")


@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("tag", sorted(fc.PENS))
def test_penalty_sets_on_both_sides_of_the_rule(tag, slots, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = fc.PENS[tag]
    both(fc.pen_pairs(), fc.expected(oracle, "pens", pen), slots, capfd, f"{tag} slots {slots}", pen=pen, takes=fc.TAKES[tag])


@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("which", ["max_s", "max_iter"])
def test_stops(which, slots, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    kw = fc.stop_opts(oracle)[0 if which == "max_s" else 1]
    both(fc.stop_pairs(oracle), fc.expected(oracle, "stops", **kw), slots, capfd, f"stop {kw} slots {slots}", **kw)


def test_cigar_launch_keeps_the_table_form(oracle, capfd, monkeypatch):
    """With CIGAR the second fold does not exist: "band_fold2" 1 launches the table form's traceback kernel and no second-fold line is written."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = fc.group(oracle, "adjacent")
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in (("force_kind", 2), ("block", 512), ("band_pack", 1), ("wide_slots", 3), ("band_fold2", 1), ("tb_budget_mb", 1024)):
            eng.set(k, v)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=mw.MWF_F_CIGAR, **fc.DEFAULT))
        s, it, nc = b.results()
        err = capfd.readouterr().err
        assert [tuple(int(x) for x in m.groups()) for m in BAND_LINE.finditer(err)] == [(512, 3, 2, 1, 1, 1, 0, 1, len(pairs))]
        assert len(TAB_LINE.findall(err)) == 1 and not FOLD2_LINE.findall(err)
        for i, (es, eit, ecig) in enumerate(fc.expected(oracle, "adjacent")):
            assert (int(s[i]), int(it[i])) == (es, eit) and b.cigar(i, int(nc[i])).tolist() == ecig, i
        b.free()
    finally:
        eng.close()
