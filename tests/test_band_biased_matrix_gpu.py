"""One test per instantiation of the packed band kernel's copies on biased offsets for the sets beyond (2,1) (tests/band_biased_matrix.py), by the method of
tests/test_band_matrix_gpu.py: MWF_DEBUG launch records, a fresh engine per align, a *fit* and an *overflow* group sized from the oracle's band trace.

  fit       the align's first launch names exactly this instantiation, with every pair; n_retries == 0 and a single launch; s, n_iter and (TB) every CIGAR
            word equal the oracle's
  overflow  same first launch; every pair handed back and taken by a later launch; the answers equal the oracle's
A score-only cell also equals its CIGAR twin.  Integer work: no tolerance.  Before these copies existed the first launch of every such align was the span
geometry's: the launch record read T 1024 K 5."""
import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
from oracle.pyoracle import make_opt
import band_biased_matrix as xm
from test_band_matrix_gpu import launches, check_answers

_oracle_cache: dict = {}
_device_cache: dict = {}


def expected(orc, g, pen_name, band_fold, group):
    G = xm.build_groups(orc, g, pen_name, band_fold)   # (folded and unfolded runs of one set mostly share their pairs: the oracle's answers are kept per input)
    pairs = G.fit if group == "fit" else G.over
    key = (pen_name, tuple(pairs))
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.align_many(pairs, make_opt(flag=1, **xm.PEN[pen_name]), threads=xm.ORACLE_THREADS)[0]
    return _oracle_cache[key]


def run_group(inst, g, pen_name, band_fold, pairs, exp, capfd):
    """One align of `pairs` routed to `inst`: (s, n_iter, cigars | None, n_retries, launches)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in xm.tunables(g, band_fold):
            eng.set(k, v)
        if inst.TB:   # a traceback arena that holds every pair's rows at once: a re-run can then only be a hand-back
            need = max(int(it) + 16 * int(s) + 8192 for s, it, _ in exp)
            eng.set("tb_budget_mb", (need * len(pairs) >> 20) + 64)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=1 if inst.TB else 0, **xm.PEN[pen_name]))
        s, it, nc = b.results()
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if inst.TB else None
        err = capfd.readouterr().err
        out = (np.array(s).copy(), np.array(it).copy(), cig, int(eng.stats().n_retries), launches(err))
        b.free()
        return out
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", xm.ALL_CELLS, ids=xm.cell_id)
def test_band_biased_instantiation(cell, oracle, capfd, monkeypatch):
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
    (pen_name, band_fold), = cell.runs
    G = xm.build_groups(oracle, g, pen_name, band_fold)
    label = f"{xm.cell_id(cell)} {pen_name} band_fold {band_fold}"
    print("   " + xm.check_groups(g, G, label))
    for group, pairs in (("fit", G.fit), ("overflow", G.over)):
        exp = expected(oracle, g, pen_name, band_fold, group)
        got = _device_cache.get((inst, group)) or run_group(inst, g, pen_name, band_fold, pairs, exp, capfd)   # (a score-only cell has already run its CIGAR twin)
        _device_cache[(inst, group)] = got
        n_retries, ls = got[3], got[4]
        print(f"   {label} {group}: {len(pairs)} pairs, re-runs {n_retries}, launches {[(k, xm.inst_id(i) if i else None, n) for k, i, n in ls]}")
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
            tw = _device_cache.get((twin, group)) or run_group(twin, g, pen_name, band_fold, pairs, exp, capfd)
            _device_cache[(twin, group)] = tw
            assert tw[4] and tw[4][0][1] == twin, (label, group, tw[4][:1])
            assert (got[0] == tw[0]).all() and (got[1] == tw[1]).all(), (label, group, "score-only differs from its CIGAR twin")
