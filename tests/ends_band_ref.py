"""Yardsticks for ends-free and extension alignment under per-pair diagonal bands (include/miniwfa.h, mwf_band_t), independent of the library's kernel:

  dp_score_band    ends_ref.dp_score with every out-of-band H, F1 and F2 set to +inf in every row -> the optimal penalty inside the band (INF: none);
  dp_matrix_band   ext_ref.dp_matrix likewise: D[i][j] of the prefix alignments whose every cell lies inside the band;
  sweep_band       ends_ref.sweep with the header's two clamps — the origin window intersected with the band's columns [blo, bhi], every new slice
                   lo = max(wf_lo - 1, 1, blo), hi = min(wf_hi + 1, cmax, bhi) — and nothing else changed;
  wfa_ends_band    ends_ref.wfa_ends on that sweep -> (s, n_iter, te, qe), or None where the feasibility rule says the band admits nothing;
  wfa_ext_band     ext_ref.wfa_ext on that sweep -> ExtRef, or None;
  clamp_band, feasible, penalty_bound_band   the host side's pure rules (miniwfa_amd/csrc/mwf_ends_band.h) in Python.

Used by tests/test_ends_band_cpu.py (which checks them against each other) and tests/test_ends_band_gpu.py."""
from __future__ import annotations

import numpy as np

from ends_ref import INF, NEG
from ext_ref import DP_INF, ExtRef

EXT_ENDS = (0, 0x7fffffff, 0, 0x7fffffff)  # the allowances of an extension


def clamp_band(tl: int, ql: int, band):
    """The band as the pass uses it: clamped to the diagonals the matrix has, [-tl, ql] (lo > hi: empty)."""
    return max(int(band[0]), -tl), min(int(band[1]), ql)


def clamp_ends(tl: int, ql: int, ends):
    return min(int(ends[0]), tl), min(int(ends[1]), tl), min(int(ends[2]), ql), min(int(ends[3]), ql)


def feasible(tl: int, ql: int, ends, band) -> bool:
    """An alignment inside the band exists iff the clamped band is non-empty and meets the origin diagonals [-t_beg', q_beg'] and the end diagonals
    [ql - tl - q_end', ql - tl + t_end']."""
    lo, hi = clamp_band(tl, ql, band)
    t_beg, t_end, q_beg, q_end = clamp_ends(tl, ql, ends)
    meets = lambda a, b: lo <= b and a <= hi  # noqa: E731
    return lo <= hi and meets(-t_beg, q_beg) and meets(ql - tl - q_end, ql - tl + t_end)


def penalty_bound_band(pen, tl: int, ql: int) -> int:
    """s <= x min(tl, ql) + max(gap(tl), gap(ql)) inside any feasible band: diagonal steps and one gap."""
    x, o1, e1, o2, e2 = pen
    gap = lambda L: 0 if L == 0 else min(o1 + L * e1, o2 + L * e2)  # noqa: E731
    return x * min(tl, ql) + max(gap(tl), gap(ql))


def penalty_bound_plain(pen, tl: int, ql: int) -> int:
    """gap(tl) + gap(ql), the bound of an alignment without a band (mwf_plan_classes.h penalty_bound)."""
    x, o1, e1, o2, e2 = pen
    gap = lambda L: 0 if L == 0 else min(o1 + L * e1, o2 + L * e2)  # noqa: E731
    return gap(tl) + gap(ql)


def _row_mask(i: int, tl: int, band) -> np.ndarray:
    """Row i (query bases consumed), columns j = 0 ... tl (target bases consumed): the cell's diagonal i - j lies inside the band."""
    d = i - np.arange(tl + 1, dtype=np.int64)
    return (d >= int(band[0])) & (d <= int(band[1]))


def dp_score_band(t: bytes, q: bytes, pen, ends, band) -> int:
    """ends_ref.dp_score among the alignments whose every cell lies on a diagonal of [d_lo, d_hi]: out-of-band H, F1 and F2 are +inf in every row.  (The
    prefix minimum that stands for the D gaps runs along a row, where the band is an interval of columns: a gap between two in-band cells stays inside.)"""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    t_beg, t_end, q_beg, q_end = clamp_ends(tl, ql, ends)
    ta = np.frombuffer(t, dtype=np.uint8)
    idx = np.arange(tl + 1, dtype=np.int64)
    best = INF
    H = F1 = F2 = None
    for i in range(ql + 1):
        out = ~_row_mask(i, tl, band)
        Ht = np.full(tl + 1, INF, dtype=np.int64)
        if i == 0:
            Ht[:t_beg + 1] = 0
            F1 = np.full(tl + 1, INF, dtype=np.int64)
            F2 = np.full(tl + 1, INF, dtype=np.int64)
        else:
            F1 = np.minimum(F1 + e1, H + o1 + e1)
            F2 = np.minimum(F2 + e2, H + o2 + e2)
            F1[out] = INF
            F2[out] = INF
            Ht = np.minimum(F1, F2)
            if tl:
                Ht[1:] = np.minimum(Ht[1:], H[:-1] + np.where(ta == q[i - 1], 0, x))
            if i <= q_beg:
                Ht[0] = 0
        Ht[out] = INF
        H = Ht.copy()
        for o, e in ((o1, e1), (o2, e2)):
            pm = np.minimum.accumulate(Ht + o - e * idx)
            if tl:
                H[1:] = np.minimum(H[1:], pm[:-1] + e * idx[1:])
        H[out] = INF
        H = np.minimum(H, INF)
        if i == ql:
            best = min(best, int(H[tl - t_end:].min()))
        if ql - i <= q_end:
            best = min(best, int(H[tl]))
    return best


def dp_matrix_band(t: bytes, q: bytes, pen, band) -> np.ndarray:
    """ext_ref.dp_matrix inside the band: D[i][j] >= DP_INF where no in-band alignment of q[0, i) with t[0, j) exists."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    ta = np.frombuffer(t, dtype=np.uint8)
    idx = np.arange(tl + 1, dtype=np.int64)
    D = np.empty((ql + 1, tl + 1), dtype=np.int64)
    H = F1 = F2 = None
    for i in range(ql + 1):
        out = ~_row_mask(i, tl, band)
        if i == 0:
            Ht = np.full(tl + 1, DP_INF, dtype=np.int64)
            Ht[0] = 0
            F1 = np.full(tl + 1, DP_INF, dtype=np.int64)
            F2 = np.full(tl + 1, DP_INF, dtype=np.int64)
        else:
            F1 = np.minimum(F1 + e1, H + o1 + e1)
            F2 = np.minimum(F2 + e2, H + o2 + e2)
            F1[out] = DP_INF
            F2[out] = DP_INF
            Ht = np.minimum(F1, F2)
            if tl:
                Ht[1:] = np.minimum(Ht[1:], H[:-1] + np.where(ta == q[i - 1], 0, x))
        Ht[out] = DP_INF
        H = Ht.copy()
        for o, e in ((o1, e1), (o2, e2)):
            pm = np.minimum.accumulate(Ht + o - e * idx)
            if tl:
                H[1:] = np.minimum(H[1:], pm[:-1] + e * idx[1:])
        H[out] = DP_INF
        H = np.minimum(H, DP_INF)
        D[i] = H
    return D


def sweep_band(t: bytes, q: bytes, pen, lo0: int, hi0: int, blo: int, bhi: int, trace=None, shrinks=None):
    """ends_ref.sweep with the band's columns [blo, bhi] (1 <= blo <= bhi <= tl + ql + 1): the origin window lo0 ... hi0 is intersected with them (the caller
    has checked that something is left) and every new slice is held inside them.  Yields what ends_ref.sweep yields."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    ta, qa = np.frombuffer(t, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8)
    cmax = tl + ql + 1
    nH = max(x, o1 + e1, o2 + e2) + 1
    dead = np.full(cmax + 2, NEG, dtype=np.int64)
    diag = np.arange(cmax + 2, dtype=np.int64) - 1 - tl

    def in_matrix(d, k):
        i = d + k
        return (k >= -1) & (k < tl) & (i >= -1) & (i < ql)

    def extend(d, k):
        j, i = k + 1, d + k + 1
        live = np.arange(j.size)
        for _ in range(4):  # most runs end within a few bases: all cells at once
            jj, ii = j[live], i[live]
            ok = (jj < tl) & (ii < ql)
            ok[ok] = ta[jj[ok]] == qa[ii[ok]]
            live = live[ok]
            if not live.size:
                return j - 1
            j[live] += 1
            i[live] += 1
        for n in live:  # the few long ones: block by block
            jj, ii, step = int(j[n]), int(i[n]), 64
            while True:
                m = min(step, tl - jj, ql - ii)
                if m <= 0:
                    break
                ne = np.flatnonzero(ta[jj:jj + m] != qa[ii:ii + m])
                if ne.size:
                    jj += int(ne[0])
                    break
                jj, ii, step = jj + m, ii + m, step * 4
            j[n] = jj
        return j - 1

    lo0, hi0 = max(lo0, blo), min(hi0, bhi)  # clamp 1: the origin window
    assert lo0 <= hi0, "the band misses the origin window: ask feasible() first"
    c = np.arange(lo0, hi0 + 1, dtype=np.int64)
    d = diag[c]
    k = extend(d, np.where(d < 0, -d, 0) - 1)
    H0 = dead.copy()
    H0[c] = k
    rows = {0: (H0, dead, dead, dead, dead)}
    yield 0, 0, c, d, k
    get = lambda s, n: rows[s][n] if s in rows else dead  # noqa: E731
    wf_lo, wf_hi, n_iter, s = lo0, hi0, 0, 0
    while True:
        s += 1
        lo, hi = max(wf_lo - 1, 1, blo), min(wf_hi + 1, cmax, bhi)  # clamp 2: the growth
        n_iter += hi - lo + 1
        if trace is not None:
            trace.append((lo - 1 - tl, hi - 1 - tl))
        c = np.arange(lo, hi + 1, dtype=np.int64)
        hx, a, b = get(s - x, 0), get(s - o1 - e1, 0), get(s - o2 - e2, 0)
        g1e, g1f, g2e, g2f = get(s - e1, 1), get(s - e1, 2), get(s - e2, 3), get(s - e2, 4)
        ne1 = np.maximum(a[lo - 1:hi], g1e[lo - 1:hi])
        ne2 = np.maximum(b[lo - 1:hi], g2e[lo - 1:hi])
        nf1 = np.maximum(a[lo + 1:hi + 2], g1f[lo + 1:hi + 2]) + 1
        nf2 = np.maximum(b[lo + 1:hi + 2], g2f[lo + 1:hi + 2]) + 1
        nh = np.maximum(hx[lo:hi + 1] + 1, np.maximum(np.maximum(ne1, ne2), np.maximum(nf1, nf2)))
        if nh[0] >= -1:
            wf_lo = lo
        if nh[-1] >= -1:
            wf_hi = hi
        d = diag[lo:hi + 1]
        inside = np.flatnonzero(in_matrix(d, nh))
        if inside.size:
            nh[inside] = extend(d[inside], nh[inside])
        new = []
        for vals in (nh, ne1, nf1, ne2, nf2):
            r = dead.copy()
            r[lo:hi + 1] = vals
            new.append(r)
        rows[s] = tuple(new)
        yield s, n_iter, c[inside], d[inside], nh[inside]
        if (s & 0xff) == 0:
            good = np.zeros(wf_hi - wf_lo + 1, dtype=bool)
            for r in rows.values():
                for v in r:
                    if v is not dead:
                        good |= in_matrix(diag[wf_lo:wf_hi + 1], v[wf_lo:wf_hi + 1])
            at = np.flatnonzero(good)
            assert at.size, "shrink: no good column in the band"
            was = (wf_lo, wf_hi)
            wf_lo, wf_hi = was[0] + int(at[0]), was[0] + int(at[-1])
            if shrinks is not None:
                shrinks.append((s,) + was + (wf_lo, wf_hi))
        rows.pop(s - nH + 1, None)


def band_columns(tl: int, ql: int, band):
    """The clamped band in columns (column = diagonal + tl + 1), or (1, tl + ql + 1) for band None."""
    if band is None:
        return 1, tl + ql + 1
    lo, hi = clamp_band(tl, ql, band)
    return lo + tl + 1, hi + tl + 1


def wfa_ends_band(t: bytes, q: bytes, pen, ends, band, trace=None, shrinks=None):
    """The header's banded pass, restated: -> (s, n_iter, te, qe), or None for a pair whose band admits no alignment (the stopped record)."""
    tl, ql = len(t), len(q)
    if band is not None and not feasible(tl, ql, ends, band):
        return None
    t_beg, t_end, q_beg, q_end = clamp_ends(tl, ql, ends)
    blo, bhi = band_columns(tl, ql, band)
    for s, n_iter, c, d, k in sweep_band(t, q, pen, tl + 1 - t_beg, tl + 1 + q_beg, blo, bhi, trace, shrinks):
        i = d + k
        end = ((i == ql - 1) & (tl - 1 - k <= t_end)) | ((k == tl - 1) & (ql - 1 - i <= q_end))
        if end.any():
            n = int(end.argmax())
            return s, n_iter, int(k[n]) + 1, int(i[n]) + 1


def wfa_ext_band(t: bytes, q: bytes, pen, A: int, Z: int, band, trace=None, shrinks=None):
    """ext_ref.wfa_ext on the banded sweep: -> ExtRef, or None where the band excludes diagonal 0."""
    tl, ql = len(t), len(q)
    if band is not None and not feasible(tl, ql, EXT_ENDS, band):
        return None
    blo, bhi = band_columns(tl, ql, band)
    best = dict(B=None, s=0, te=0, qe=0, tie_cols=0, tie_later=0)
    F = 0
    for s, n_iter, c, d, k in sweep_band(t, q, pen, tl + 1, tl + 1, blo, bhi, trace, shrinks):
        if c.size:
            a = d + 2 * k + 2
            n = int(a.argmax())
            a_s = int(a[n])
            V = A * a_s - 2 * s
            if best["B"] is None or V > best["B"]:
                best.update(B=V, s=s, te=int(k[n]) + 1, qe=int(d[n] + k[n]) + 1, tie_cols=int((a == a_s).sum()), tie_later=0)
            elif V == best["B"]:
                best["tie_later"] += 1
            F = max(F, a_s)
        why = 0 if ((d + k == ql - 1) | (k == tl - 1)).any() else 1 if s > 0 and Z >= 0 and best["B"] - (A * F - 2 * s) > Z else None
        if why is not None:
            return ExtRef(best["s"], n_iter, best["te"], best["qe"], best["B"], s, why, F, best["tie_cols"], best["tie_later"])


def cigar_diagonals(words, tb: int, qb: int):
    """(lowest, highest) diagonal i - j over every cell a CIGAR visits, the start cell (qb, tb) included."""
    j, i = int(tb), int(qb)
    lo = hi = i - j
    for w in words:
        op, n = int(w) & 0xf, int(w) >> 4
        if op == 1:
            i += n
        elif op == 2:
            j += n
        else:
            j, i = j + n, i + n
        lo, hi = min(lo, i - j), max(hi, i - j)
    return lo, hi
