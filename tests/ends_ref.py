"""Yardsticks for the ends-free alignment (include/miniwfa.h, mwf_ends_t), independent of the library's kernel:

  dp_score      a numpy Gotoh DP (two affine gap pieces, the free-end rules) -> the optimal penalty;
  check_cigar   a CIGAR checker: ops and bases agree, the words consume exactly the ranges, the ranges obey the allowances, the words score s;
  sweep         the pass both restatements share, on full-width numpy rows: the slice of every penalty from an origin window on, the band bookkeeping,
                n_iter, and the reference's stripe shrink (wf_stripe_shrink, miniwfa.c:144-171; oracle/mwf_oracle.c ring_shrink): at every penalty that
                is a multiple of 256 the band [wf_lo, wf_hi] is cut down to its outermost good columns, a column being good if, in any of the last
                nH = max(x, o1 + e1, o2 + e2) + 1 slices, any of its H, E1, F1, E2, F2 offsets lies inside the matrix;
  wfa_ends      a small restatement of the header's pass (origin window, end rule) on that sweep -> s, n_iter and the end cell, at any penalty.

Used by tests/test_ends_cpu.py (which checks the three against each other and against the oracle) and tests/test_ends_gpu.py."""
from __future__ import annotations

import numpy as np

INF = 1 << 40
NEG = -0x40000000  # kNegInf
FREE = 0x7fffffff  # an allowance that covers any sequence


def pen_of(opt) -> tuple[int, int, int, int, int]:
    return int(opt.x), int(opt.o1), int(opt.e1), int(opt.o2), int(opt.e2)


def dp_score(t: bytes, q: bytes, pen, ends) -> int:
    """The cheapest alignment of t[tb, te) with q[qb, qe) over every choice the allowances ends = (t_beg, t_end, q_beg, q_end) permit.  A gap of
    L bases costs min(o1 + L e1, o2 + L e2).  Row i: query bases consumed; column j: target bases consumed."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    t_beg, t_end, q_beg, q_end = (min(int(ends[0]), tl), min(int(ends[1]), tl), min(int(ends[2]), ql), min(int(ends[3]), ql))
    ta = np.frombuffer(t, dtype=np.uint8)
    idx = np.arange(tl + 1, dtype=np.int64)
    best = INF
    H = F1 = F2 = None
    for i in range(ql + 1):
        Ht = np.full(tl + 1, INF, dtype=np.int64)
        if i == 0:
            Ht[:t_beg + 1] = 0  # start at (0, tb), tb <= t_beg
            F1 = np.full(tl + 1, INF, dtype=np.int64)
            F2 = np.full(tl + 1, INF, dtype=np.int64)
        else:
            F1 = np.minimum(F1 + e1, H + o1 + e1)  # query base i-1 against a gap (I)
            F2 = np.minimum(F2 + e2, H + o2 + e2)
            Ht = np.minimum(F1, F2)
            if tl:
                Ht[1:] = np.minimum(Ht[1:], H[:-1] + np.where(ta == q[i - 1], 0, x))
            if i <= q_beg:
                Ht[0] = 0  # start at (qb, 0), qb <= q_beg
        # target bases against a gap (D): a gap is never opened from a cell that itself ends in one (o >= 0), so the prefix minimum over Ht does it
        H = Ht.copy()
        for o, e in ((o1, e1), (o2, e2)):
            pm = np.minimum.accumulate(Ht + o - e * idx)
            if tl:
                H[1:] = np.minimum(H[1:], pm[:-1] + e * idx[1:])
        H = np.minimum(H, INF)
        if i == ql:
            best = min(best, int(H[tl - t_end:].min()))  # query used up, at most t_end target bases left
        if ql - i <= q_end:
            best = min(best, int(H[tl]))  # target used up, at most q_end query bases left
    return best


def check_cigar(mw, opt, t: bytes, q: bytes, words, rng, ends, s: int) -> None:
    """Asserts that `words` align t[tb, te) with q[qb, qe) (rng = (tb, te, qb, qe)), that the ranges obey the allowances and that the words cost s."""
    tl, ql = len(t), len(q)
    tb, te, qb, qe = (int(v) for v in rng)
    t_beg, t_end, q_beg, q_end = (min(int(ends[0]), tl), min(int(ends[1]), tl), min(int(ends[2]), ql), min(int(ends[3]), ql))
    assert 0 <= tb <= te <= tl and 0 <= qb <= qe <= ql, rng
    assert (tb <= t_beg and qb == 0) or (qb <= q_beg and tb == 0), (rng, ends)
    assert te == tl or qe == ql, rng
    assert tl - te <= t_end and ql - qe <= q_end, (rng, ends)
    j, i, prev = tb, qb, -1
    for w in words:
        op, n = int(w) & 0xf, int(w) >> 4
        assert n > 0 and op != prev, ("empty or unmerged run", [int(v) for v in words])
        prev = op
        if op == 7:
            assert t[j:j + n] == q[i:i + n] and j + n <= te and i + n <= qe, ("= run over unequal bases", j, i, n)
            j, i = j + n, i + n
        elif op == 8:
            assert j + n <= te and i + n <= qe and all(t[j + k] != q[i + k] for k in range(n)), ("X run over equal bases", j, i, n)
            j, i = j + n, i + n
        elif op == 1:
            i += n
        elif op == 2:
            j += n
        else:
            raise AssertionError(f"operator {op} in an ends-free CIGAR")
    assert (j, i) == (te, qe), ("the words do not consume the ranges", (j, i), rng)
    sc, ct, cq = mw.cigar2score(opt, [int(w) for w in words])
    assert (sc, ct, cq) == (s, te - tb, qe - qb), ((sc, ct, cq), s, rng)


def sweep(t: bytes, q: bytes, pen, lo0: int, hi0: int, trace=None, shrinks=None):
    """The slices of a pass whose origin window is columns lo0 ... hi0 (column = diagonal + tl + 1), rows dead outside their windows.  Yields, per penalty
    from 0 on, (s, n_iter, c, d, k): columns, diagonals and offsets of the slice's in-matrix H cells after their extension, columns ascending; the caller
    ends the pass by not asking for more.  The shrink of penalty s runs after s was yielded, as the reference's runs after its end test.
    trace, a list, receives (lo, hi) of every new slice in diagonals (what Oracle.band_trace gives); shrinks, a list, receives
    (s, wf_lo, wf_hi before, wf_lo, wf_hi after) in columns."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    ta, qa = np.frombuffer(t, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8)
    cmax = tl + ql + 1
    nH = max(x, o1 + e1, o2 + e2) + 1  # the slices a shrink looks at; no older one is read again
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

    c = np.arange(lo0, hi0 + 1, dtype=np.int64)
    d = diag[c]
    k = extend(d, np.where(d < 0, -d, 0) - 1)  # (every origin cell is inside the matrix)
    H0 = dead.copy()
    H0[c] = k
    rows = {0: (H0, dead, dead, dead, dead)}  # penalty -> H, E1, F1, E2, F2
    yield 0, 0, c, d, k
    get = lambda s, n: rows[s][n] if s in rows else dead  # noqa: E731
    wf_lo, wf_hi, n_iter, s = lo0, hi0, 0, 0
    while True:
        s += 1
        lo, hi = max(wf_lo - 1, 1), min(wf_hi + 1, cmax)
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
        if (s & 0xff) == 0:  # the shrink, over the slices of penalties s - nH + 1 ... s
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


def wfa_ends(t: bytes, q: bytes, pen, ends, trace=None, shrinks=None):
    """The header's pass, restated: -> (s, n_iter, te, qe).  The first penalty with an end cell is the answer, the lowest column wins.  trace, shrinks: see sweep."""
    tl, ql = len(t), len(q)
    t_beg, t_end, q_beg, q_end = (min(int(ends[0]), tl), min(int(ends[1]), tl), min(int(ends[2]), ql), min(int(ends[3]), ql))
    for s, n_iter, c, d, k in sweep(t, q, pen, tl + 1 - t_beg, tl + 1 + q_beg, trace, shrinks):
        i = d + k
        end = ((i == ql - 1) & (tl - 1 - k <= t_end)) | ((k == tl - 1) & (ql - 1 - i <= q_end))
        if end.any():
            n = int(end.argmax())
            return s, n_iter, int(k[n]) + 1, int(i[n]) + 1
