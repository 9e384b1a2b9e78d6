"""Inputs of the window-epoch tests of the packed band kernel (miniwfa_amd/csrc/mwf_band2_kernel.h: a penalty whose window meets the same chunks as the last one
reuses the slot state the last full header derived).  Every case is a batch of small pairs chosen ON THE CPU, from the oracle's band trace alone, for the one
moment at which a stale cache would show, and names the penalty at which it happens:

  both-cross     the window's start reaches a chunk boundary (or crosses one) and its end crosses one, in the SAME penalty
  cross-shrink   an edge crosses a boundary at a penalty that is a multiple of 256, and the shrink behind it moves an edge inward across a boundary
  climb          the window's start climbs: the slot mapping is moved up, kAgeOut penalties late
  ends-at-change the pair ends at a penalty whose chunks differ from the previous penalty's
  stop           max_s / max_iter stop the pair at such a penalty
  overflow       the pair is handed back (ST_BAND_OVERFLOW) at the penalty where its window first meets more chunks than the geometry holds
  note           default routing, 66 / 67 pairs of the 512-thread class: a batch whose windows all fit 23 chunks, and one with a pair whose window meets 24 - 31

tests/test_band_epoch_cpu.py asserts that every case has the property it is named for; tests/test_band_epoch_gpu.py runs them (s, n_iter, CIGAR == oracle)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import skewed_pairs, synth_pair
from oracle.pyoracle import make_opt
import band_matrix as bm

CHUNK = 256
DEFAULT = bm.PEN["default"]
NOFOLD = bm.PEN["nofold21"]


def columns(lohi: np.ndarray, tl: int) -> np.ndarray:
    """The kernel's (lo, hi) of every penalty, as columns (diagonal + tl + 1)."""
    return lohi.astype(np.int64) + tl + 1


def keys(lohi: np.ndarray, tl: int):
    """[(gl_next, ga, gb)] per penalty: what the kernel's epoch key packs."""
    c = columns(lohi, tl)
    return [(max(int(lo) - 1, 1) >> 8, int(lo) >> 8, int(hi) >> 8) for lo, hi in c]


def both_cross(lohi, tl):
    """First penalty (1-based) at which the start's part of the key AND the end's change together, or None."""
    k = keys(lohi, tl)
    for i in range(1, len(k)):
        if (k[i][0] != k[i - 1][0] or k[i][1] != k[i - 1][1]) and k[i][2] != k[i - 1][2]:
            return i + 1
    return None


def cross_then_shrink(lohi, tl):
    """A penalty s, multiple of 256, whose chunks differ from those of s - 1, with the window of s + 1 (behind the shrink) starting or ending in a chunk further INWARD."""
    k = keys(lohi, tl)
    for s in range(256, len(k), 256):
        if k[s - 1] != k[s - 2] and (k[s][1] > k[s - 1][1] or k[s][2] < k[s - 1][2]):
            return s
    return None


def remaps_up(lohi, tl, age_out: int):
    """Penalties at which the slot mapping moves UP (the kernel's bookkeeping behind the barrier, as tests/band_matrix.py rule_chunks restates it)."""
    gl, up_wait, up_min, out = max(tl, 1) >> 8, 0, 0, []
    for i, (gl_next, _, _) in enumerate(keys(lohi, tl)):
        if gl_next < gl:
            gl, up_wait = gl_next, 0
        elif gl_next > gl:
            up_min = gl_next if up_wait == 0 else min(up_min, gl_next)
            up_wait += 1
            if up_wait > age_out:
                gl, up_wait = up_min, 0
                out.append(i + 1)
        else:
            up_wait = 0
    return out


def ends_at_change(lohi, tl):
    k = keys(lohi, tl)
    return len(k) if len(k) >= 2 and k[-1] != k[-2] else None


def change_penalties(lohi, tl):
    k = keys(lohi, tl)
    return [i + 1 for i in range(1, len(k)) if k[i] != k[i - 1]]


def max_chunks(lohi, tl, ql):
    """The most chunks a penalty's window (and the columns next to it) meets, counted from the chunk of the column before its start."""
    c, cmax = columns(lohi, tl), tl + ql + 1
    return max((min(int(hi) + 1, cmax) >> 8) - (max(int(lo) - 1, 1) >> 8) + 1 for lo, hi in c) if len(c) else 1


def overflow_penalty(g, age_out: int, lohi, tl, ql):
    """The penalty at which rule_chunks first fails for geometry g, or None."""
    n, cmax = bm.nwk(g), tl + ql + 1
    gl, up_wait, up_min = max(tl, 1) >> 8, 0, 0
    for i, (lo, hi) in enumerate(columns(lohi, tl).tolist()):
        gl_next = max(lo - 1, 1) >> 8
        if (min(hi + 1, cmax) >> 8) - min(gl_next, gl) + 1 > n - 1:
            assert not bm.rule_chunks(g, age_out, lohi[:i + 1], tl, ql) and bm.rule_chunks(g, age_out, lohi[:i], tl, ql)   # (the restatement this one follows)
            return i + 1
        if gl_next < gl:
            gl, up_wait = gl_next, 0
        elif gl_next > gl:
            up_min = gl_next if up_wait == 0 else min(up_min, gl_next)
            up_wait += 1
            if up_wait > age_out:
                gl, up_wait = up_min, 0
        else:
            up_wait = 0
    return None


def _rand(rng, n):
    return bm._rand(rng, n)


def _pool():
    """(kind, target, query): unrelated pairs whose target length puts column tl + 1 on a multiple of 128 (both edges then meet chunk boundaries together while the
    window still grows a column a side per penalty), unrelated length-skewed pairs, related pairs of 0.6 - 2.5 kb at 8 - 25 %."""
    rng = np.random.default_rng(20240)
    out = []
    for tl in (127, 255, 383, 511, 639, 767, 895, 1023, 1151, 1279):
        for dq in (0, -37, 61):
            out.append(("unrelated", _rand(rng, tl), _rand(rng, max(40, tl + dq))))
    for i, L in enumerate((600, 900, 1300, 1700, 2100, 2500)):
        for p in (0.08, 0.15, 0.25):
            out.append(("related", *synth_pair(77000 + 10 * i + int(100 * p), L, p)))
    out += [("skewed", t, q) for t, q in skewed_pairs(1, 150, 200, 3000)[::3]]
    return out


Traced = namedtuple("Traced", "kind t q lohi far")
_traced: dict = {}


def traced(orc, pen: dict):
    key = tuple(sorted(pen.items()))
    if key not in _traced:
        pool = _pool()
        tr = bm._trace_all(orc, pen, [(t, q) for _, t, q in pool])
        _traced[key] = [Traced(k, t, q, lohi, far) for (k, t, q), (lohi, far) in zip(pool, tr)]
    return _traced[key]


# the geometries, forced through the engine's tunables as tests/band_matrix.py does: NWK = 3, 6, 12, 24 (block), 32 (four slots), and 768 threads byte-wise
GEOM = {nwk: bm.GEOMS[k] for nwk, k in ((3, (64, 3, 0)), (6, (128, 3, 0)), (12, (256, 3, 0)), (24, (512, 3, 0)), (32, (512, 4, 0)))}
G768 = bm.GEOMS[(768, 2, 0)]


def finishes(g, fold: int, pen: dict, x: Traced) -> bool:
    """The geometry finishes the pair: every documented hand-back rule passes on the oracle's trace, and the forced route takes it."""
    tl, ql = len(x.t), len(x.q)
    if not bm.host_admits(g, pen, tl, ql):
        return False
    return bm.fits(g, fold, pen, x.lohi, x.far, tl, ql)[1]


Case = namedtuple("Case", "name nwk pen band_fold pairs opts where")
# pairs: [(t, q)]; opts: one dict of extra mwf options per pair group run (max_s / max_iter), {} for none; where: {pair index: penalty} the property holds at
MAX_PER_CASE = 6


def _select(orc, nwk, pen, fold, prop, kinds=None):
    g = GEOM[nwk]
    folded = bool(fold and bm.pen_folds(pen) and g.T >= 512)
    pairs, where = [], {}
    for x in traced(orc, pen):
        if kinds and x.kind not in kinds:
            continue
        if not finishes(g, folded, pen, x):
            continue
        s = prop(x, folded)
        if s:
            where[len(pairs)] = s
            pairs.append((x.t, x.q))
            if len(pairs) == MAX_PER_CASE:
                break
    return pairs, where


def tunables(nwk: int, band_fold: int):
    """NWK 3 ... 24: the block is forced; 32: the default routing with wide_slots 4, which starts the pairs of its 512-thread class on four slots (length-skewed
    pairs of 2 - 3 kb are of that class: a forced gap weighs six-fold)."""
    return bm.tunables(GEOM[nwk], band_fold)


def build_cases(orc):
    cases = []
    for nwk in (6, 12, 24, 32):
        pairs, where = _select(orc, nwk, DEFAULT, 1, lambda x, f: both_cross(x.lohi, len(x.t)))
        cases.append(Case(f"both-cross-nwk{nwk}", nwk, DEFAULT, 1, pairs, {}, where))
    for nwk in (12, 24, 32):
        pairs, where = _select(orc, nwk, DEFAULT, 1, lambda x, f: cross_then_shrink(x.lohi, len(x.t)))
        cases.append(Case(f"cross-shrink-nwk{nwk}", nwk, DEFAULT, 1, pairs, {}, where))
    for nwk in (24, 32):
        for fold in (1, 0):
            pairs, where = _select(orc, nwk, DEFAULT, fold, lambda x, f: next((s for s in remaps_up(x.lohi, len(x.t), bm.age_out(f, 2, 1)) if s + 8 <= len(x.lohi)), None))   # (penalties run on behind the remap)
            cases.append(Case(f"climb-nwk{nwk}-fold{fold}", nwk, DEFAULT, fold, pairs, {}, where))
    for nwk in (12, 24):
        pairs, where = _select(orc, nwk, DEFAULT, 1, lambda x, f: ends_at_change(x.lohi, len(x.t)))
        cases.append(Case(f"ends-at-change-nwk{nwk}", nwk, DEFAULT, 1, pairs, {}, where))
    pairs, where = _select(orc, 24, NOFOLD, 1, lambda x, f: both_cross(x.lohi, len(x.t)))
    cases.append(Case("both-cross-nofold21-nwk24", 24, NOFOLD, 1, pairs, {}, where))
    return cases


def stop_cases(orc):
    """[(name, nwk, pair, opt kw, penalty)]: max_s stops the pair once penalty s* is done (s > max_s), max_iter once the cells counted through s* exceed it."""
    out = []
    for nwk in (6, 24):
        g = GEOM[nwk]
        for x in traced(orc, DEFAULT):
            ch = [s for s in change_penalties(x.lohi, len(x.t)) if 40 < s < len(x.lohi) - 1]
            if x.kind != "unrelated" or not ch or not finishes(g, nwk == 24, DEFAULT, x):
                continue
            s_star = ch[len(ch) // 2]
            c = columns(x.lohi, len(x.t))
            cum = np.cumsum(c[:, 1] - c[:, 0] + 1)
            out.append((f"stop-max_s-nwk{nwk}", nwk, (x.t, x.q), dict(max_s=s_star - 1), s_star))
            out.append((f"stop-max_iter-nwk{nwk}", nwk, (x.t, x.q), dict(max_iter=int(cum[s_star - 1]) - 1), s_star))
            break
    return out


def overflow_cases(orc):
    """[(nwk, pairs, {index: penalty})]: pairs the forced geometry hands back for certain by the chunk rule, with the penalty at which it does."""
    out = []
    for nwk in (3, 6, 12):
        g = GEOM[nwk]
        pairs, where = [], {}
        for x in traced(orc, DEFAULT):
            tl, ql = len(x.t), len(x.q)
            if not bm.host_admits(g, DEFAULT, tl, ql):
                continue
            s = overflow_penalty(g, bm.age_out(0, 2, 1), x.lohi, tl, ql)
            # (handed back by THIS rule: no forecast fires before it)
            if s and bm.rule_forecast(g, x.far[:s - 1], tl, ql) and bm.forecast_margin(g, x.far[:s - 1], tl, ql) > 64:
                where[len(pairs)] = s
                pairs.append((x.t, x.q))
                if len(pairs) == MAX_PER_CASE:
                    break
        out.append((nwk, pairs, where))
    return out


NOTE_PAIRS = 66
_note: list = []


def note_batches(orc):
    """(narrow, wide): two batches of the 512-thread class under the default routing, of more than 64 pairs (up to 64 the results of a first align are
    preset on the host and the align does not zero the work counters: such a batch is not started on four slots).  narrow: every window (with the columns
    next to it) meets at most 23 chunks; wide: the same pairs and one unrelated length-skewed pair whose window meets more than 23 and at most 31."""
    if _note:
        return _note[0]
    narrow = [synth_pair(91000 + i, 4200 + 10 * i, 0.03) for i in range(NOTE_PAIRS)]
    rng = np.random.default_rng(915)
    g = GEOM[32]
    for tl, ql in ((5400, 2500), (5600, 2600), (5800, 2400), (5200, 2800)):
        wide_pair = (_rand(rng, tl), _rand(rng, ql))
        (lohi, far), = bm._trace_all(orc, DEFAULT, [wide_pair])
        if bm.host_class(DEFAULT, tl, ql) == 1 and 23 < max_chunks(lohi, tl, ql) <= 31 and bm.fits(g, 1, DEFAULT, lohi, far, tl, ql)[1]:
            _note.append((narrow, narrow + [wide_pair]))
            return _note[0]
    raise AssertionError("no pair between 24 and 31 chunks")


def note_chunks(orc, pairs):
    tr = bm._trace_all(orc, DEFAULT, pairs)
    return [max_chunks(lohi, len(t), len(q)) for (t, q), (lohi, _) in zip(pairs, tr)]


def opt_of(pen: dict, **kw):
    return make_opt(**pen, **kw)


CASE_NAMES = ([f"both-cross-nwk{n}" for n in (6, 12, 24, 32)] + [f"cross-shrink-nwk{n}" for n in (12, 24, 32)] + [f"climb-nwk{n}-fold{f}" for n in (24, 32) for f in (1, 0)] +
              [f"ends-at-change-nwk{n}" for n in (12, 24)] + ["both-cross-nofold21-nwk24"])
STOP_NAMES = [f"stop-{k}-nwk{n}" for n in (6, 24) for k in ("max_s", "max_iter")]
_cases: dict = {}


def case(orc, name: str) -> Case:
    if not _cases:
        _cases.update({c.name: c for c in build_cases(orc)})
        assert list(_cases) == CASE_NAMES, list(_cases)
    return _cases[name]


_stops: dict = {}


def stop_case(orc, name: str):
    if not _stops:
        _stops.update({c[0]: c for c in stop_cases(orc)})
        assert list(_stops) == STOP_NAMES, list(_stops)
    return _stops[name]
