"""Yardsticks for the ends-free alignment (include/miniwfa.h, mwf_ends_t), independent of the library's kernel:

  dp_score      a numpy Gotoh DP (two affine gap pieces, the free-end rules) -> the optimal penalty;
  check_cigar   a CIGAR checker: ops and bases agree, the words consume exactly the ranges, the ranges obey the allowances, the words score s;
  wfa_ends      a small restatement of the header's pass (origin window, end rule, band bookkeeping) -> s, n_iter and the end cell.  It has no
                shrink, so it stands for pairs with s < 256 only.

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


def wfa_ends(t: bytes, q: bytes, pen, ends):
    """The header's pass, restated on full-width numpy rows (dead outside their windows): -> (s, n_iter, te, qe).  No shrink: s < 256 only."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    t_beg, t_end, q_beg, q_end = (min(int(ends[0]), tl), min(int(ends[1]), tl), min(int(ends[2]), ql), min(int(ends[3]), ql))
    cmax = tl + ql + 1
    dead = lambda: np.full(cmax + 2, NEG, dtype=np.int64)  # noqa: E731

    def extend(d, k):
        j, i = k + 1, d + k + 1
        while j < tl and i < ql and t[j] == q[i]:
            j, i = j + 1, i + 1
        return j - 1

    def in_matrix(d, k):
        return 0 <= k + 1 <= tl and 0 <= d + k + 1 <= ql

    def is_end(d, k):
        i = d + k
        return (i == ql - 1 and tl - 1 - k <= t_end) or (k == tl - 1 and ql - 1 - i <= q_end)

    lo, hi = tl + 1 - t_beg, tl + 1 + q_beg
    H0 = dead()
    for c in range(lo, hi + 1):
        d = c - 1 - tl
        H0[c] = extend(d, (-d if d < 0 else 0) - 1)
    for c in range(lo, hi + 1):
        if is_end(c - 1 - tl, int(H0[c])):
            return 0, 0, int(H0[c]) + 1, c - 1 - tl + int(H0[c]) + 1
    Hs, E1s, F1s, E2s, F2s = [H0], [dead()], [dead()], [dead()], [dead()]
    get = lambda rows, s: rows[s] if s >= 0 else dead()  # noqa: E731
    wf_lo, wf_hi, n_iter, s = lo, hi, 0, 0
    while True:
        s += 1
        assert s < 256, "the restatement has no shrink"
        lo, hi = max(wf_lo - 1, 1), min(wf_hi + 1, cmax)
        n_iter += hi - lo + 1
        c = np.arange(lo, hi + 1)
        hx, a, b = get(Hs, s - x), get(Hs, s - o1 - e1), get(Hs, s - o2 - e2)
        g1e, g1f, g2e, g2f = get(E1s, s - e1), get(F1s, s - e1), get(E2s, s - e2), get(F2s, s - e2)
        ne1 = np.maximum(a[c - 1], g1e[c - 1])
        ne2 = np.maximum(b[c - 1], g2e[c - 1])
        nf1 = np.maximum(a[c + 1], g1f[c + 1]) + 1
        nf2 = np.maximum(b[c + 1], g2f[c + 1]) + 1
        nh = np.maximum(hx[c] + 1, np.maximum(np.maximum(ne1, ne2), np.maximum(nf1, nf2)))
        if nh[0] >= -1:
            wf_lo = lo
        if nh[-1] >= -1:
            wf_hi = hi
        end = None
        for n, col in enumerate(c):
            d, k = int(col) - 1 - tl, int(nh[n])
            if in_matrix(d, k):
                k = extend(d, k)
                nh[n] = k
                if end is None and is_end(d, k):
                    end = (k + 1, d + k + 1)
        for rows, vals in ((Hs, nh), (E1s, ne1), (F1s, nf1), (E2s, ne2), (F2s, nf2)):
            r = dead()
            r[lo:hi + 1] = vals
            rows.append(r)
        if end is not None:
            return s, n_iter, end[0], end[1]
