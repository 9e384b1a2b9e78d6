"""One test per instantiation of the packed band kernel (tests/band_matrix.py: the table, what reaches each entry, and its inputs).

Per cell and run (penalty set, band_fold), two aligns on a fresh engine:
  fit       pairs the instantiation can hold by the oracle's band trace: the launch record (MWF_DEBUG, stderr) names exactly this instantiation as the
            align's first launch, with every pair of the batch; n_retries == 0 — it finished every pair itself; s, n_iter and (TB) every CIGAR word
            equal the oracle's
  overflow  pairs whose window is more than a chunk beyond the span: same first launch, n_retries >= the group's size, a later launch took them, the
            answers equal the oracle's
Score-only cells also equal what their CIGAR twin computed on the same inputs.  Integer work: no tolerance anywhere.

That the cells can fail was tried once with a library built from a copy of the sources in which one computed value was changed — the upper threshold of the
biased copies' range check (mwf_band2_kernel.h `top`) lowered to 8000, so that the check fires early: the eight cells of 512 x 5 / 512 x 6 on biased offsets went red by
"fit pairs were handed back" (n_retries 16 and 18 for 16 fit pairs, the launch record showing the span geometry and then the generic kernel taking them); the four
512 x 4 (2,1) cells run beside them as a control went red too, in their overflow group, whose re-run goes through the span geometry — biased offsets as well — and
came back as an error of the library ("still unfinished after every retry").  Nothing faulted."""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
from oracle.pyoracle import make_opt
import band_matrix as bm

BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs, grid (\d+)")
KIND_LINE = re.compile(r"\[libmwf_hip\] kernel kind (-?\d+): .* (\d+) pairs")

_oracle_cache: dict = {}
_device_cache: dict = {}


def expected(orc, g, pen_name, fold, group):
    key = (g, pen_name, fold, group)
    if key not in _oracle_cache:
        G = bm.build_groups(orc, g, pen_name, fold)
        pairs = G.fit if group == "fit" else G.over
        _oracle_cache[key] = orc.align_many(pairs, make_opt(flag=1, **bm.PEN[pen_name]), threads=bm.ORACLE_THREADS)[0]
    return _oracle_cache[key]


def launches(err: str):
    """[(kind, Inst | None, pairs)] of one align, in launch order: every launch prints its `kernel kind` line, a band launch its `band2 launch` line after it."""
    out = []
    for ln in err.splitlines():
        m = KIND_LINE.search(ln)
        if m:
            out.append([int(m.group(1)), None, int(m.group(2))])
        m = BAND_LINE.search(ln)
        if m:
            assert out and out[-1][1] is None, err
            out[-1][1] = bm.Inst(*map(int, m.groups()[:8]))
            assert out[-1][2] == int(m.group(9)), ln
    return out


def run_group(inst, g, pen_name, band_fold, pairs, exp, capfd):
    """One align of `pairs` routed to `inst`: (s, n_iter, cigars | None, n_retries, launches)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in bm.tunables(g, band_fold):
            eng.set(k, v)
        if inst.TB:   # a traceback arena that holds every pair's rows at once: a re-run can then only be a hand-back
            need = max(int(it) + 16 * int(s) + 8192 for s, it, _ in exp)
            eng.set("tb_budget_mb", (need * len(pairs) >> 20) + 64)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=1 if inst.TB else 0, **bm.PEN[pen_name]))
        s, it, nc = b.results()   # (the re-runs of what was handed back are launched when the results are asked for)
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if inst.TB else None
        err = capfd.readouterr().err
        out = (np.array(s).copy(), np.array(it).copy(), cig, int(eng.stats().n_retries), launches(err))
        b.free()
        return out
    finally:
        eng.close()


def check_answers(got, exp, tb, label):
    s, it, cig = got[:3]
    for i, (es, eit, ecig) in enumerate(exp):
        assert (int(s[i]), int(it[i])) == (es, eit), (label, "pair", i, (int(s[i]), int(it[i])), (es, eit))
        if tb:
            assert cig[i] == (ecig or []), (label, "pair", i, "CIGAR")


@pytest.mark.gpu
@pytest.mark.parametrize("cell", bm.ALL_CELLS, ids=bm.cell_id)
def test_band_instantiation(cell, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    report = []
    try:
        _run_cell(cell, oracle, capfd, report.append)
    finally:
        with capfd.disabled():
            print()
            for ln in report:
                print(ln)


def _run_cell(cell, oracle, capfd, print):
    inst, g = cell.inst, cell.geom
    for pen_name, band_fold in cell.runs:
        G = bm.build_groups(oracle, g, pen_name, band_fold)
        label = f"{bm.cell_id(cell)} {pen_name} band_fold {band_fold}"
        print("   " + bm.check_groups(g, G, label))
        for group, pairs in (("fit", G.fit), ("overflow", G.over)):
            exp = expected(oracle, g, pen_name, band_fold, group)
            got = _device_cache.get((inst, pen_name, band_fold, group)) or run_group(inst, g, pen_name, band_fold, pairs, exp, capfd)   # (a score-only cell has already run its CIGAR twin)
            _device_cache[(inst, pen_name, band_fold, group)] = got
            n_retries, ls = got[3], got[4]
            print(f"   {label} {group}: {len(pairs)} pairs, re-runs {n_retries}, launches {[(k, bm.inst_id(i) if i else None, n) for k, i, n in ls]}")
            # reached: the align's first launch is this instantiation, with every pair of the batch
            assert ls and ls[0][0] == 2 and ls[0][1] == inst and ls[0][2] == len(pairs), (label, group, ls[:2])
            check_answers(got, exp, inst.TB, f"{label} {group}")
            if group == "fit":
                assert n_retries == 0 and len(ls) == 1, (label, "fit pairs were handed back", n_retries, ls)
            else:
                assert n_retries >= len(pairs), (label, "overflow pairs were not handed back", n_retries)
                assert sum(n for _, _, n in ls[1:]) >= len(pairs), (label, "no later launch took the pairs", ls)
            if not inst.TB:   # ... and equal what the CIGAR twin computes on the same inputs
                twin = inst._replace(TB=1)
                tkey = (twin, pen_name, band_fold, group)
                tw = _device_cache.get(tkey) or run_group(twin, g, pen_name, band_fold, pairs, exp, capfd)
                _device_cache[tkey] = tw
                assert tw[4] and tw[4][0][1] == twin, (label, group, tw[4][:1])
                assert (got[0] == tw[0]).all() and (got[1] == tw[1]).all(), (label, group, "score-only differs from its CIGAR twin")
