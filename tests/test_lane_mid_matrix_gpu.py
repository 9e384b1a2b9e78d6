"""One test per instantiation of the lane kernel and of the mid kernel (tests/lane_mid_matrix.py: the table, what reaches each entry, and its inputs),
and the edge tests of both kernels.

Per cell and run (penalty set, band_fold), two aligns on a fresh engine:
  fit       pairs the instantiation finishes by the oracle's band trace: the launch record (MWF_DEBUG, stderr: `lane launch:` / `mid launch:`) names exactly
            this instantiation as the align's first launch, with every pair of the batch; n_retries == 0 and it is the only launch — it finished every pair
            itself; s, n_iter and (TB) every CIGAR word equal the oracle's
  overflow  pairs the kernel hands back (chunks, first shrink; span, forecast): same first launch, n_retries >= the group's size, a later launch took them,
            the answers equal the oracle's.  (Penalty sets under which the mid kernel's span holds every window of a 2 kb pair have no such group.)
Score-only cells also equal what their CIGAR twin computed on the same inputs.  Integer work: no tolerance anywhere.

That the cells can fail was tried once with two libraries built from copies of the sources in which one computed value per kernel was changed (never an
address or a bound on an access); nothing faulted:
  1  lane_pass: the folded E1 / F1 store without its max(..., hx); mid_pass: the forecast's threshold C - 2 nH - 64 times 0.6.
     27 of 33 red.  Both lane FOLD cells by wrong answers in the fit group (default: pair 0 (s 32, n_iter 368) for (12, 60); f_e3: n_iter 24 for 26), the lane edge
     test under three of its five sets (score-only, the default band_fold: e.g. (220, 18188) for (98, 8242)) and test_limits on the 96-row set, which folds.  All 18 mid
     cells by "fit pairs were handed back" (1 - 16 re-runs: default 5, a22 11, e88 13, f_e8 16, e2gt 3, asm5 1), and the three FOLD-across-shrinks tests likewise.
     Green: the four unfolded lane cells and the two edge sets that cannot fold (o1 != x).
  2  lane_pass: s_shrink lowered by 40; mid_pass: the folded E1 / F1 store without its max(..., hx).
     16 of 33 red.  All six lane cells by "fit pairs were handed back" (the pairs at the penalty limit: 1 under default and asm5, 3 under f_e3, 7 under e88).  The six mid
     FOLD cells by wrong answers in the fit group (default: (144, 16944) for (64, 2654); f_e3 (66, 1920) for (30, 290); f_e8 (168, 8568) for (136, 5080)), the three
     FOLD-across-shrinks tests (f_e1 (853, 714051) for (522, 270408)) and test_limits on the nH 64 set, which folds.  Green: the twelve unfolded mid cells, the lane edge tests.
"""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, synth_pair
from oracle.pyoracle import make_opt
import band_matrix as bm
import lane_mid_matrix as lm
from test_band_matrix_gpu import BAND_LINE, KIND_LINE, check_answers

LANE_LINE = re.compile(r"\[libmwf_hip\] lane launch: TB (\d+) S2 (\d+) FOLD (\d+), chunks (\d+), (\d+) pairs, grid (\d+)")
MID_LINE = re.compile(r"\[libmwf_hip\] mid launch: T (\d+) TB (\d+) S2 (\d+) FOLD (\d+), groups (\d+), (\d+) pairs, grid (\d+)")

_oracle_cache: dict = {}
_device_cache: dict = {}


def launches(err: str):
    """[(kind, instantiation | None, pairs, chunks or groups | None)] of one align, in launch order: every launch prints its `kernel kind` line, a lane, mid or band
    launch its own record after it."""
    out = []
    for ln in err.splitlines():
        m = KIND_LINE.search(ln)
        if m:
            out.append([int(m.group(1)), None, int(m.group(2)), None])
            continue
        for rx, ctor, n in ((LANE_LINE, lm.LaneInst, 3), (MID_LINE, lm.MidInst, 4), (BAND_LINE, bm.Inst, 8)):
            m = rx.search(ln)
            if m:
                assert out and out[-1][1] is None, err
                out[-1][1] = ctor(*map(int, m.groups()[:n]))
                if n < 8:
                    out[-1][3] = int(m.group(n + 1))
                assert out[-1][2] == int(m.group(n + 2 if n < 8 else 9)), ln
    return out


def _show(ls):
    return [(k, (lm.inst_id(i) if not isinstance(i, bm.Inst) else "band " + bm.inst_id(i)) if i else None, n) for k, i, n, _ in ls]


def expected(orc, pen: dict, pairs, key=None):
    if key is None or key not in _oracle_cache:
        exp = orc.align_many(pairs, make_opt(flag=1, **pen), threads=bm.ORACLE_THREADS)[0]
        if key is None:
            return exp
        _oracle_cache[key] = exp
    return _oracle_cache[key]


def run_align(tun, pen: dict, tb: int, pairs, exp, span_cols: int, capfd):
    """One align of `pairs` on a fresh engine with the tunables `tun`: (s, n_iter, cigars | None, n_retries, launches)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in tun:
            eng.set(k, v)
        if tb:   # a traceback arena that holds every pair's rows at once — the kernel's rows of the span's width, or a re-run's: a re-run can then only be a hand-back
            need = max(max(int(it) + 16 * int(s) + 8192, (int(s) + 2) * span_cols) for s, it, _ in exp)
            eng.set("tb_budget_mb", max(lm.TB_BUDGET_MB, (need * len(pairs) >> 20) + 64))
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(mw.opt_init(flag=1 if tb else 0, **pen))
        s, it, nc = b.results()   # (the re-runs of what was handed back are launched when the results are asked for)
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if tb else None
        err = capfd.readouterr().err
        out = (np.array(s).copy(), np.array(it).copy(), cig, int(eng.stats().n_retries), launches(err))
        b.free()
        return out
    finally:
        eng.close()


def _report(lines):
    def deco(capfd):
        with capfd.disabled():
            print()
            for ln in lines:
                print(ln)
    return deco


@pytest.mark.gpu
@pytest.mark.parametrize("cell", lm.MATRIX, ids=lm.cell_id)
def test_instantiation(cell, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    report = []
    try:
        _run_cell(cell, oracle, capfd, report.append)
    finally:
        _report(report)(capfd)


def _run_cell(cell, oracle, capfd, print):
    inst = cell.inst
    for pen_name, band_fold in cell.runs:
        rk = lm.run_key(cell, pen_name)
        G = lm.build_groups(oracle, *rk)
        pen = lm.PEN[pen_name]
        label = f"{lm.cell_id(cell)} {pen_name} band_fold {band_fold}"
        print("   " + lm.check_groups(*rk, G, label))
        span_cols = 64 * G.span
        for group, pairs in (("fit", G.fit), ("overflow", G.over)):
            if not pairs:
                assert group == "overflow" and not G.can_overflow
                continue
            exp = expected(oracle, pen, pairs, rk + (group,))
            dkey = (inst, cell.chunks, pen_name, band_fold, group)
            got = _device_cache.get(dkey) or run_align(lm.tunables(cell, band_fold), pen, inst.TB, pairs, exp, span_cols, capfd)   # (a score-only cell has already run its CIGAR twin)
            _device_cache[dkey] = got
            n_retries, ls = got[3], got[4]
            print(f"   {label} {group}: {len(pairs)} pairs, re-runs {n_retries}, launches {_show(ls)}")
            # reached: the align's first launch is this instantiation, with every pair of the batch, on the span the groups were sized for
            assert ls and ls[0][0] == 2 and ls[0][1] == inst and ls[0][2] == len(pairs) and ls[0][3] == G.span, (label, group, ls[:2])
            check_answers(got, exp, inst.TB, f"{label} {group}")
            if group == "fit":
                assert n_retries == 0 and len(ls) == 1, (label, "fit pairs were handed back", n_retries, _show(ls))
            else:
                assert n_retries >= len(pairs), (label, "overflow pairs were not handed back", n_retries)
                assert sum(n for _, _, n, _ in ls[1:]) >= len(pairs), (label, "no later launch took the pairs", _show(ls))
            if not inst.TB:   # ... and equal what the CIGAR twin computes on the same inputs
                twin = inst._replace(TB=1, FOLD=0)
                tcell = cell._replace(inst=twin)
                tkey = (twin, cell.chunks, pen_name, band_fold, group)
                tw = _device_cache.get(tkey) or run_align(lm.tunables(tcell, band_fold), pen, 1, pairs, exp, span_cols, capfd)
                _device_cache[tkey] = tw
                assert tw[4] and tw[4][0][1] == twin, (label, group, tw[4][:1])
                assert (got[0] == tw[0]).all() and (got[1] == tw[1]).all(), (label, group, "score-only differs from its CIGAR twin")


# ---- lane kernel: gap runs across chunk edges --------------------------------------------------------------------------------------------
# Chunk 0 holds diagonals -32 ... 31, chunk 1 -64 ... -33 (lanes 0-31) and 32 ... 63 (lanes 32-63), chunk 2 -96 ... -65 and 64 ... 95.  The E/F row a chunk
# overwrites is the row its neighbour still reads where their blocks touch: the old F of lane 0's column and the old E of lane 63's travel to the next chunk
# in scalars (cE1 ... cF2, picked up by lanes 31 and 32), and a chunk reads the inner neighbour's column straight from the row — before that chunk rewrites it.
# Both are only exercised by a gap RUN that passes those columns.
EDGE_PEN = lm.EDGE_PEN
EDGES = ((-32, -33), (-64, -65), (31, 32), (63, 64))     # (last diagonal of the inner chunk, first of the outer one)


def gap_pair(G: int, plus: bool):
    """A pair around one gap of G bases and one of G - 24 back (the host gives the lane kernel pairs whose lengths differ by at most 24): the path leaves the main
    diagonal for diagonal -G (plus: +G) and returns to -24 (+24).  The gaps' bases occur nowhere else, so they can only be gapped or mismatched."""
    r = np.random.default_rng(G)
    seg = lambda n: np.frombuffer(b"AC", dtype=np.uint8)[r.integers(0, 2, n)].tobytes()
    a, m1, m2 = seg(8), seg(8), seg(8)
    t, q = a + b"G" * G + m1 + m2, a + m1 + b"T" * (G - lm.LANE_MAX_SKEW) + m2
    return (q, t) if plus else (t, q)


def gap_runs(cigar):
    """[(first diagonal, last diagonal)] of every gap run of a CIGAR (diagonal = query index - target index; a deletion lowers it, an insertion raises it)."""
    d, out = 0, []
    for w in cigar:
        n, op = w >> 4, "MIDNSHP=XB"[w & 0xf]
        if op in "ID":
            out.append((d, d + n if op == "I" else d - n))
            d = out[-1][1]
    return out


def crossed(runs):
    """{(edge, direction)}: the chunk edges a gap run passes, outwards or inwards."""
    got = set()
    for d0, d1 in runs:
        for inner, outer in EDGES:
            if min(d0, d1) <= min(inner, outer) and max(d0, d1) >= max(inner, outer):
                got.add(((inner, outer), "out" if abs(d1) > abs(d0) else "in"))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", sorted(EDGE_PEN))
def test_lane_gap_runs_across_chunk_edges(pen_name, oracle, capfd, monkeypatch):
    """Pairs built around one long deletion / insertion, on both sides of the main diagonal, under sets with e1 in {1, 2, 3, 8} and e2 in {1, 2, 8}, score and CIGAR,
    lane_chunks 3 and 4.  By the oracle's CIGAR the gap runs pass the first and the last column of chunk 1 — and, where the set's penalties let a gap of 65
    bases end below the first shrink, of chunk 2 — outwards and inwards; the lane kernel finishes every pair (n_retries == 0) with the oracle's answers."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = EDGE_PEN[pen_name]
    assert lm.lane_supported(pen)
    report = []
    try:
        for chunks in (3, 4):
            cand = [gap_pair(G, plus) for G in (65, 64, 57, 34, 33) for plus in (False, True)]
            assert all(lm.lane_admits(pen, len(t), len(q)) for t, q in cand)
            tr = bm._trace_all(oracle, pen, cand)
            pairs = [c for c, (lohi, _) in zip(cand, tr) if lm.lane_fits(pen, chunks, lohi)]
            exp = expected(oracle, pen, pairs)
            seen = set()
            for (t, q), (s, _, cig) in zip(pairs, exp):
                c = crossed(gap_runs(cig))
                seen |= c
                report.append(f"   {pen_name} chunks {chunks}: {len(t)} x {len(q)}, penalty {s} (first shrink at {lm.lane_s_max(pen) + 1}), gap runs {gap_runs(cig)} pass {sorted(c)}")
            # both edges of chunk 1's blocks, on both sides, in both directions
            want = {(e, way) for e in ((-32, -33), (31, 32)) for way in ("out", "in")}
            assert want <= seen, (pen_name, chunks, "no gap run passes", sorted(want - seen))
            if pen_name in ("e1_2-e2_1", "e1_1-e2_2", "e1_1-e2_8"):   # ... and of chunk 2's, where a gap of 65 bases is affordable
                want2 = {(e, way) for e in ((-64, -65), (63, 64)) for way in ("out", "in")}
                assert want2 <= seen, (pen_name, chunks, "no gap run passes", sorted(want2 - seen))
            for tb in (0, 1):
                got = run_align(lm.LANE_COMMON + (("lane_chunks", chunks),), pen, tb, pairs, exp, 64 * chunks, capfd)
                report.append(f"   {pen_name} chunks {chunks} TB {tb}: {len(pairs)} pairs, re-runs {got[3]}, launches {_show(got[4])}")
                ls = got[4]
                assert ls and isinstance(ls[0][1], lm.LaneInst) and ls[0][1].TB == tb and ls[0][2] == len(pairs) and ls[0][3] == chunks, _show(ls)
                check_answers(got, exp, tb, f"{pen_name} chunks {chunks} TB {tb}")
                assert got[3] == 0 and len(ls) == 1, (pen_name, chunks, tb, "handed back", got[3], _show(ls))
    finally:
        _report(report)(capfd)


# ---- the admission limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_limits(oracle, capfd, monkeypatch):
    """The deepest rings each kernel admits launch it; the set just beyond each limit launches neither; the answers equal the oracle's either way.
    Lane: nH + 2 e1 + 2 e2 == 96 against 97, and rings plus sequence copies beyond 60 KB (the deepest rings on four chunks are 49 920 bytes: only a pair of
    11.5 kb of target + query, under a raised lane_max_len, passes 60 KB — one nearly identical pair, a few dozen penalties).  Mid: nH == 64 against 65, e1 == 9, e2 == 9."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    report = []
    reads = [synth_pair(880 + i, 150, 0.03) for i in range(8)]
    t_long, q_long = synth_pair(890, 5900, 0.001)
    long_pair = [(t_long[:5800], q_long[:5800])]
    assert lm.lane_lds_bytes(lm.PEN["lane_deep"], 4, lm._group_seq_lds(long_pair)) > 60 * 1024 >= lm.lane_lds_bytes(lm.PEN["lane_deep"], 4, lm._group_seq_lds(reads))
    mids = [synth_pair(870 + i, 1000, 0.03) for i in range(4)]
    assert all(lm.mid_admits(lm.PEN["mid_deep"], len(t), len(q)) for t, q in mids)
    lane_tun = lm.LANE_COMMON + (("lane_chunks", 4),)
    cases = (("lane 96 rows", lane_tun, lm.PEN["lane_deep"], reads, lm.LaneInst),
             ("lane 97 rows", lane_tun, lm.PEN_BEYOND["lane_97"], reads, None),
             ("lane beyond 60 KB", lane_tun + (("lane_max_len", 8000),), lm.PEN["lane_deep"], long_pair, None),
             ("mid nH 64", lm.MID_COMMON, lm.PEN["mid_deep"], mids, lm.MidInst),
             ("mid nH 65", lm.MID_COMMON, lm.PEN_BEYOND["mid_nH65"], mids, None),
             ("mid e1 9", lm.MID_COMMON, lm.PEN_BEYOND["mid_e1_9"], mids, None),
             ("mid e2 9", lm.MID_COMMON, lm.PEN_BEYOND["mid_e2_9"], mids, None))
    try:
        for label, tun, pen, pairs, first in cases:
            exp = expected(oracle, pen, pairs)
            for tb in (0, 1):
                got = run_align(tun, pen, tb, pairs, exp, 4096, capfd)
                ls = got[4]
                report.append(f"   {label} TB {tb}: re-runs {got[3]}, launches {_show(ls)}")
                check_answers(got, exp, tb, f"{label} TB {tb}")
                if first is not None:
                    assert ls and isinstance(ls[0][1], first) and ls[0][2] == len(pairs) and got[3] == 0, (label, _show(ls), got[3])
                else:
                    assert ls and not any(isinstance(i, (lm.LaneInst, lm.MidInst)) for _, i, _, _ in ls), (label, _show(ls))
    finally:
        _report(report)(capfd)


# ---- mid kernel: FOLD across shrinks -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pen_name,T", [("f_e1", 512), ("f_e3", 512), ("f_e8", 1024)])
def test_mid_fold_across_shrinks(pen_name, T, oracle, capfd, monkeypatch):
    """The folding sets with e1 of 1, 3 and 8 on pairs whose final penalty passes 512 (two shrinks inside the kernel): folded (band_fold 1) against unfolded
    (band_fold 0) against the oracle, every pair finished by the mid kernel."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = lm.PEN[pen_name]
    assert lm.pen_folds(pen)
    G = lm.build_groups(oracle, "mid", pen_name, 0, 1)
    exp_all = expected(oracle, pen, G.fit, ("mid", pen_name, 0, 1, "fit"))
    keep = [i for i, e in enumerate(exp_all) if e[0] > 512] + [0]   # (and the group's longest pair, which sizes the launch's span)
    pairs, exp = [G.fit[i] for i in keep], [exp_all[i] for i in keep]
    assert len(pairs) >= 4 and lm.mid_groups(pen, pairs) == G.span
    report, got = [], {}
    try:
        for bf in (1, 0):
            got[bf] = run_align(lm.MID_COMMON + (("mid_block", T), ("seq2bit", 1), ("band_fold", bf)), pen, 0, pairs, exp, 64 * G.span, capfd)
            ls = got[bf][4]
            report.append(f"   {pen_name} band_fold {bf}: {len(pairs)} pairs, penalties {sorted(e[0] for e in exp)[1]} ... {max(e[0] for e in exp)}, re-runs {got[bf][3]}, launches {_show(ls)}")
            assert ls and ls[0][1] == lm.MidInst(T, 0, 1, bf) and ls[0][2] == len(pairs), _show(ls)
            check_answers(got[bf], exp, 0, f"{pen_name} band_fold {bf}")
            assert got[bf][3] == 0 and len(ls) == 1, (pen_name, bf, "handed back", got[bf][3], _show(ls))
        assert (got[1][0] == got[0][0]).all() and (got[1][1] == got[0][1]).all()
    finally:
        _report(report)(capfd)
