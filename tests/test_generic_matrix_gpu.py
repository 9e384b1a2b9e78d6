"""One test per instantiation of the generic kernel (tests/generic_matrix.py: the table, what reaches each entry, its penalty sets, modes and inputs), and the
edge tests of that kernel.

Per cell, penalty set and mode, one align on a fresh engine under force_kind 0 and the cell's tunables:
  - the launch record (MWF_DEBUG, stderr: `generic launch:`) is the align's only launch and names exactly this instantiation with every pair of the batch
    (one exception, by the plan's own rule: max_s = 60 caps the window the plan sizes the launch by, so an LDS2 cell's run under it must land on the stream form
    of 256 threads instead; the stop rule inside the LDS2 forms is exercised by max_s = 4200, which stops the wide pairs)
  - n_retries == 0
  - s, n_iter and every CIGAR word equal the oracle's (integer work: no tolerance); score-only runs also equal their CIGAR twin's s and n_iter
  - low-memory runs report lowmem_two_pass == 1
Oracle answers are computed once per (set, options, batch) and shared by the cells: the ten block cells run the same batches.  The plain score-only runs of the
LDS2 batches alone are checked against the oracle's CIGAR run of the same batch (s and n_iter do not depend on the flag; the 8400 x 8400 pairs make it worth it);
every other run is checked against the oracle's run under its own options.  Device results are shared too (_device_cache): the CIGAR run of an LDS2 MODE1 cell is
executed by whichever test asks for it first — normally the MODE0 cell's twin check — so a fault in a MODE1 form would be reported by that test, and the 0.02 - 0.05 s
of the MODE1 cells in the record are the checking alone.  A cell checks every one of its runs and fails with the list of all that are red.
No cell's sets were thinned.  On an MI355X (profiles/generic_matrix/): the block cells 1.6 - 7.8 s each (107 aligns; the first of them pays the oracle for all ten),
the LDS2 cells up to 4.2 s, every edge test below 5 s, 72 s in all.

That the cells can fail was tried once with three libraries built from copies of mwf_kernels.hip in which one computed value was changed (never an address or a
bound on an access); nothing faulted (figures: (s, n_iter) got, then the oracle's; profiles/generic_matrix/mutations.txt has every red run):
  A  the E1 / F1 ring row r1 one row further (penalty s_new - e1 + 1), both passes — in the plain score-only instantiations, on 32-bit rows, where n1 > 2 only:
     the traceback follows its bytes without a window check, so a wrong row under a CIGAR or low-memory run could read outside a row of the traceback arena.
     15 of 22 red.  All ten block cells, 20 of 107 runs each: score and score-max_s60 under the ten sets with e1 >= 2 (default (1553, 1229689) for (1613, 1281077);
     ring256 and a22 by ST_INTERNAL on pair 14).  lds2-T768-H160-MODE0 in 21 of 24 runs, lds2-T512-H161-MODE0 in its 7 max_s60 runs (the stream form they land on),
     the big-ring cell in 6 of 27, test_h16_hand_backs[0] (the 32-bit re-run: (277, 63923) for (283, 66821)), the ring-depth test.  Green, as built: the sets with
     e1 = 1 (edit, e2gt), the MODE1 cells and every CIGAR and low-memory run.
  B  take_snapshot: the penalty an E/F slice is labelled with, s - age + 1 (read by trace_checkpoints only; the second pass checks the column against its window).
     13 of 22 red.  All ten block cells, 33 of 107 runs each: lowmem-step97, -step nH and -step nH - 1 under every set but edit (224 runs by ST_INTERNAL, 115 by
     wrong answers: o1zero (1585, 149307) for (1584, 149222)); the big-ring cell in 9 of 27; test_lowmem_step_edges[e51] ((278, 56524) for (278, 56100)); the
     ring-depth test.  Green: the steps of 1 and 2 on the small pairs, the edit set, test_lowmem_step_edges[e2gt], and everything that is not low-memory
     (which the mutation cannot reach).
  C  track_good one slice short (< nH - 1).
     19 of 22 red, all by n_iter alone (s and the CIGARs stay right: a stale good bit only moves the shrink): the ten block cells in 48 - 51 of 107 runs (score,
     cigar, lowmem-step97 under all twelve sets, the nH steps under eight: default (1613, 1498815) for (1613, 1281077)), the four LDS2 cells in 16 of 24 and 8 of 16,
     both hand-back tests, both chunk-edge tests, the ring-depth test on its ring256 half.  Green: the big-ring cell — with nH > 256 the changed comparison is
     true at every penalty, the mutant computes the same there — and the step-edge tests (eight pairs of at most 1100 bases).
No mutation went unnoticed by the cells, so none asked for a cell that is missing.
"""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, random_seq, synth_pair
from oracle.pyoracle import make_opt
import band_matrix as bm
import generic_matrix as gm
from test_band_matrix_gpu import check_answers

KIND_LINE = re.compile(r"\[libmwf_hip\] kernel kind (-?\d+): block (\d+) .* (\d+) workgroup\(s\) per CU, .* (\d+) pairs")
GEN_LINE = re.compile(r"\[libmwf_hip\] generic launch: T (\d+) STREAM (\d) LDS2 (\d) H16 (\d) MODE (-?\d+) BIG (\d), lds_cols (\d+), (\d+) pairs, grid (\d+)")

_oracle_cache: dict = {}
_device_cache: dict = {}


def launches(err: str):
    """[[kind, Inst | None, pairs, lds_cols, workgroups per CU]] of one align, in launch order: every launch prints its `kernel kind` line, a launch of the
    generic kernel its own record after it."""
    out = []
    for ln in err.splitlines():
        m = KIND_LINE.search(ln)
        if m:
            out.append([int(m.group(1)), None, int(m.group(4)), None, int(m.group(3))])
            continue
        m = GEN_LINE.search(ln)
        if m:
            assert out and out[-1][1] is None and out[-1][0] == 0, err
            out[-1][1] = gm.Inst(*map(int, m.groups()[:6]))
            out[-1][3] = int(m.group(7))
            assert out[-1][2] == int(m.group(8)), ln
    return out


def _show(ls):
    return [(k, gm.inst_id(i) if i else None, n) for k, i, n, _, _ in ls]


def _okey(pen_name, okw, bkey):
    kw = dict(okw)
    if set(kw) == {"flag"} and bkey[0] == "wide":
        kw["flag"] = 1     # (the LDS2 batches only: their plain score-only run is checked against the oracle's CIGAR run's s and n_iter)
    return (pen_name, tuple(sorted(kw.items())), bkey), kw


def prefetch(orc, jobs):
    """jobs: [(pen_name, options, batch key, pairs)] — the oracle's answers for those not cached yet, all pairs of all jobs on one pool of host threads,
    the longest first (ctypes drops the GIL inside the call)."""
    todo = {}
    for pen_name, okw, bkey, pairs in jobs:
        key, kw = _okey(pen_name, okw, bkey)
        if key not in _oracle_cache and key not in todo:
            todo[key] = (make_opt(**kw, **gm.PEN[pen_name]), pairs)
    tasks = sorted(((key, i) for key, (_, pairs) in todo.items() for i in range(len(pairs))), key=lambda ki: -len(todo[ki[0]][1][ki[1]][0]) * max(1, len(todo[ki[0]][1][ki[1]][1])))
    with ThreadPoolExecutor(bm.ORACLE_THREADS) as ex:
        res = list(ex.map(lambda ki: orc.align(*todo[ki[0]][1][ki[1]], todo[ki[0]][0]), tasks))
    for key, (_, pairs) in todo.items():
        _oracle_cache[key] = [None] * len(pairs)
    for (key, i), r in zip(tasks, res):
        _oracle_cache[key][i] = r


def expected(orc, pen_name, okw, bkey, pairs):
    prefetch(orc, [(pen_name, okw, bkey, pairs)])
    return _oracle_cache[_okey(pen_name, okw, bkey)[0]]


def run_align(tun, pen: dict, okw: dict, pairs, capfd):
    """One align of `pairs` on a fresh engine with the tunables `tun`: (s, n_iter, cigars | None, n_retries, launches, lowmem_two_pass)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in tun:
            eng.set(k, v)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(**okw, **pen))
        s, it, nc = b.results()   # (a re-run of what was handed back is launched when the results are asked for)
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if okw.get("flag", 0) & 1 else None
        err = capfd.readouterr().err
        st = eng.stats()
        out = (np.array(s).copy(), np.array(it).copy(), cig, int(st.n_retries), launches(err), int(st.lowmem_two_pass))
        b.free()
        return out
    finally:
        eng.close()


def _report(lines, capfd):
    with capfd.disabled():
        print()
        for ln in lines:
            print(ln)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", gm.MATRIX, ids=gm.cell_id)
def test_generic_instantiation(cell, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    report = []
    try:
        _run_cell(cell, oracle, capfd, report.append)
    finally:
        _report(report, capfd)


def _device(cell, pen_name, mname, okw, pairs, capfd):
    key = (cell.inst, pen_name, mname)
    if key not in _device_cache:
        _device_cache[key] = run_align(cell.tun, gm.PEN[pen_name], okw, pairs, capfd)
    return _device_cache[key]


def _run_cell(cell, oracle, capfd, print):
    runs = []
    for pen_name in cell.sets:
        for mname, okw, which in gm.cell_modes(cell, pen_name):
            bkey, pairs = gm.batch(cell, pen_name, which, okw.get("step", 0))
            runs.append((pen_name, mname, okw, bkey, pairs))
    prefetch(oracle, [(pn, okw, bkey, pairs) for pn, _, okw, bkey, pairs in runs])
    red = []   # every run is checked, whatever an earlier one found: a failure names all the runs that are wrong, not the first
    for run in runs:
        try:
            _check_run(cell, oracle, capfd, print, *run)
        except (AssertionError, RuntimeError) as e:   # (RuntimeError: a pair came back with an error status, e.g. ST_INTERNAL)
            red.append(f"{run[0]} {run[1]}: {str(e).splitlines()[0][:300] if str(e) else 'assert'}")
            print(f"   RED {gm.cell_id(cell)} {red[-1]}")
    assert not red, (gm.cell_id(cell), f"{len(red)} of {len(runs)} runs", red)


def _check_run(cell, oracle, capfd, print, pen_name, mname, okw, bkey, pairs):
    label = f"{gm.cell_id(cell)} {pen_name} {mname}"
    exp = expected(oracle, pen_name, okw, bkey, pairs)
    got = _device(cell, pen_name, mname, okw, pairs, capfd)
    n_retries, ls, two_pass = got[3], got[4], got[5]
    inst = gm.launched_inst(cell, pen_name, okw, pairs)   # (the cell's own, but for an LDS2 cell's max_s = 60 run: see generic_matrix.modes)
    print(f"   {label}: {len(pairs)} pairs, penalties up to {max(e[0] for e in exp)}, re-runs {n_retries}, launches {_show(ls)}, {ls[0][4] if ls else '?'} workgroup(s) per CU")
    # reached: the align's ONLY launch is that instantiation, with every pair of the batch
    assert len(ls) == 1 and ls[0][0] == 0 and ls[0][1] == inst and ls[0][2] == len(pairs), (label, _show(ls))
    assert ls[0][3] == (gm.LDS_COLS if inst.LDS2 else 0), (label, ls[0])
    assert n_retries == 0, (label, "pairs were run again", n_retries)
    assert two_pass == (1 if okw.get("step", 0) > 0 else 0), (label, "lowmem_two_pass", two_pass)
    check_answers(got, exp, okw["flag"] & 1, label)
    if mname == "score":   # ... and equal what the CIGAR twin computes on the same inputs
        tcell = cell
        if inst.LDS2:
            tcell = next(c for c in gm.MATRIX if c.inst.LDS2 and c.inst.H16 == inst.H16 and c.inst.MODE == 1)
        tw = _device(tcell, pen_name, "cigar", dict(flag=1), pairs, capfd)
        assert tw[4] and tw[4][0][1] == tcell.inst, (label, _show(tw[4]))
        assert (got[0] == tw[0]).all() and (got[1] == tw[1]).all(), (label, "score-only differs from its CIGAR twin")


# ---- the 16-bit rows' hand-backs ---------------------------------------------------------------------------------------------------------
H16_TUN = gm.COMMON + (("block", 0), ("ring16", 2))


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [0, 1])
def test_h16_hand_backs(flag, oracle, capfd, monkeypatch):
    """Under the asm5-like set: a pair with an N (the 2-bit sequence copies of the 16-bit form hold A/C/G/T only) and a 50 kb target against its own 30 kb prefix —
    admitted by the plan (tl + (tl + ql) / 8 < 65500), and tl + s + 3 passes 65532 on the way to the 20 kb deletion — come back and are run again on 32-bit rows;
    every other pair is finished by the 16-bit form.  n_retries equals the number of such pairs, the second launch is a 32-bit form, the answers are the oracle's."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = gm.PEN["asm5"]
    t50 = random_seq(21, 50000)
    tn, qn = synth_pair(31, 900, 0.05)
    back = [(tn[:300] + b"N" + tn[301:], qn), (t50, t50[:30000])]
    pairs = [tq for tq in gm.base_pairs() if len(tq[0]) + len(tq[1]) > 600][:12] + gm.wide_pairs(cap=False) + back
    assert gm.takes_wide_form(pen, pairs) and gm.ring16_admitted(pairs)
    exp = expected(oracle, "asm5", dict(flag=1), ("h16-back", 0), pairs)
    assert len(t50) + exp[-1][0] + 3 > 65532 and all(len(t) + e[0] + 3 <= 65532 for (t, _), e in zip(pairs[:-1], exp[:-1]))
    got = run_align(H16_TUN, pen, dict(flag=flag), pairs, capfd)
    ls = got[4]
    first = gm.Inst(768, 1, 1, 1, 1, 0) if flag else gm.Inst(512, 1, 1, 1, 0, 0)
    with capfd.disabled():
        print(f"\n   asm5 flag {flag}: {len(pairs)} pairs, re-runs {got[3]}, launches {_show(ls)}")
    assert ls and ls[0][1] == first and ls[0][2] == len(pairs), _show(ls)
    assert got[3] == len(back), (got[3], _show(ls))
    assert len(ls) == 2 and ls[1][1] is not None and ls[1][1].H16 == 0 and ls[1][2] == len(back), _show(ls)
    check_answers(got, exp, flag, f"h16 hand-backs flag {flag}")


# ---- an LDS-resident window whose edges sit on chunk edges -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h16", [0, 1])
def test_lds_window_on_chunk_edges(h16, oracle, capfd, monkeypatch):
    """Under the set with o1 == 0: by the oracle's band trace the window of the 4200 x 4100 pair, while E2/F2 live in LDS, starts on the first column of a 256-column
    chunk at some penalties and ends on the last column of one at others.  The same batch with lds_e2 0 (the stream form on 512 threads, E2/F2 in HBM): both equal the oracle."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen_name = "o1zero"
    pen = gm.PEN[pen_name]
    cell = next(c for c in gm.MATRIX if c.inst.LDS2 and c.inst.H16 == h16 and c.inst.MODE == 1)
    bkey, pairs = gm.batch(cell, pen_name, "base")
    t, q = pairs[-1]
    (lohi, _), = bm._trace_all(oracle, pen, [(t, q)])
    cols = lohi.astype(np.int64) + len(t) + 1
    assert all(gm.in_lds(int(lo), int(hi), len(t)) for lo, hi in lohi)
    assert ((cols[:, 0] & 255) == 0).any() and ((cols[:, 1] & 255) == 255).any() and int((cols[:, 1] - cols[:, 0]).max()) + 1 > 4096
    exp = expected(oracle, pen_name, dict(flag=1), bkey, pairs)
    got = _device(cell, pen_name, "cigar", dict(flag=1), pairs, capfd)
    hbm = run_align(gm.COMMON + (("block", 0), ("ring16", 2 if h16 else 0), ("lds_e2", 0)), pen, dict(flag=1), pairs, capfd)
    assert _show(got[4]) == [(0, gm.cell_id(cell), len(pairs))] and got[3] == 0, _show(got[4])
    assert [l[1] for l in hbm[4]] == [gm.Inst(512, 1, 0, 0, -1, 0)] and hbm[3] == 0, _show(hbm[4])
    check_answers(got, exp, 1, "E2/F2 in LDS")
    check_answers(hbm, exp, 1, "E2/F2 in HBM")


# ---- low-memory step edges on the stream pass --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", ["e51", "e2gt"])
def test_lowmem_step_edges(pen_name, oracle, capfd, monkeypatch):
    """step == s of a pair (the snapshot due at penalty step - 1 is its last slice but one), step == s + 1 and a step above every pair's s (no snapshot is taken:
    the second pass starts from nothing), on the stream form and the one-column-per-lane form of 256 threads."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = gm.PEN[pen_name]
    pairs = [synth_pair(940 + i, (600, 700, 1024, 1100)[i % 4], 0.04 + 0.02 * (i % 3)) for i in range(8)]
    plain = expected(oracle, pen_name, dict(flag=1), ("step-edges", 0), pairs)
    s0, s_max = plain[1][0], max(e[0] for e in plain)
    report = []
    try:
        for step in (s0 - 1, s0, s0 + 1, s_max + 1):
            assert all(bm.penalty_bound(pen, len(t), len(q)) >= step for t, q in pairs) and step > 2
            exp = expected(oracle, pen_name, dict(flag=1, step=step), ("step-edges", step), pairs)
            for scalar in (0, 1):
                got = run_align(gm.COMMON + (("block", 256), ("scalar_generic", scalar)), pen, dict(flag=1, step=step), pairs, capfd)
                report.append(f"   {pen_name} step {step} (s {sorted(e[0] for e in plain)}) scalar {scalar}: re-runs {got[3]}, launches {_show(got[4])}")
                assert [l[1] for l in got[4]] == [gm.Inst(256, 1 - scalar, 0, 0, -1, 0)] and got[3] == 0 and got[5] == 1, _show(got[4])
                check_answers(got, exp, 1, f"{pen_name} step {step} scalar {scalar}")
    finally:
        _report(report, capfd)


# ---- ring depth 256 against 257 ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ring_depth_256_against_257(oracle, capfd, monkeypatch):
    """The same pairs on either side of the big-ring switch (o2 of 254 and 255), score, CIGAR and low-memory: BIG 0 at nH 256, BIG 1 at 257, each the oracle's."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [tq for tq in gm.base_pairs() if bm.penalty_bound(gm.PEN["ring256"], len(tq[0]), len(tq[1])) >= 257]
    report = []
    try:
        for pen_name, big in (("ring256", 0), ("ring257", 1)):
            for okw in (dict(flag=0), dict(flag=1), dict(flag=1, step=256), dict(flag=1, step=257)):
                exp = expected(oracle, pen_name, okw, ("ring-switch", 0), pairs)
                got = run_align(gm.COMMON + (("block", 256),), gm.PEN[pen_name], okw, pairs, capfd)
                report.append(f"   {pen_name} {okw}: {len(pairs)} pairs, re-runs {got[3]}, launches {_show(got[4])}")
                assert len(got[4]) == 1 and got[4][0][1] == (gm.Inst(256, 0, 0, 0, -1, 1) if big else gm.Inst(256, 1, 0, 0, -1, 0)) and got[3] == 0, _show(got[4])
                check_answers(got, exp, okw["flag"], f"{pen_name} {okw}")
    finally:
        _report(report, capfd)
