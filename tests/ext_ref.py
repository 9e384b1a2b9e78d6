"""Yardsticks for the extension alignment (include/miniwfa.h, mwf_ext_t), independent of the library's kernel:

  wfa_ext          the header's rule restated on numpy rows, built like ends_ref.wfa_ends (no shrink: it asserts s_stop < 256);
  dp_best          a full prefix Gotoh matrix D[i][j] from the origin (0, 0): s_end = min of D over the last row and the last column, and the yardstick
                   max{A (i + j) - 2 D[i][j] : D[i][j] <= s_end}, which a pass without the drop rule must return exactly, with s_stop == s_end;
  check_ext_cigar  a checker for an extension's CIGAR and ranges: tb = qb = 0, the words consume t[0, te) / q[0, qe) and cost s.

Used by tests/test_ext_cpu.py (which checks them against each other) and tests/test_ext_gpu.py."""
from __future__ import annotations

import collections

import numpy as np

from ends_ref import NEG

ExtRef = collections.namedtuple("ExtRef", "s n_iter te qe V s_stop why F tie_cols tie_later")
DP_INF = 1 << 28


def wfa_ext(t: bytes, q: bytes, pen, A: int, Z: int) -> ExtRef:
    """The extension pass: -> the remembered cell (s, te, qe), n_iter, info (V, s_stop, why, F), and two counts the case list is chosen by: tie_cols, the
    columns that held a_s at the answer's penalty, and tie_later, the later penalties whose best V equalled B without replacing it."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    cmax = tl + ql + 1
    depth = max(x, o1 + e1, o2 + e2)  # rows older than this are never read again
    dead = np.full(cmax + 2, NEG, dtype=np.int64)

    def extend(d, k):
        j, i = k + 1, d + k + 1
        while j < tl and i < ql and t[j] == q[i]:
            j, i = j + 1, i + 1
        return j - 1

    def in_matrix(d, k):
        return 0 <= k + 1 <= tl and 0 <= d + k + 1 <= ql

    def is_end(d, k):
        return d + k == ql - 1 or k == tl - 1

    best = dict(B=None, s=0, te=0, qe=0, tie_cols=0, tie_later=0)
    F = 0

    def steps_1_to_3(s, cells):  # cells: (column, d, k) of every tested cell of penalty s, columns ascending
        nonlocal F
        if not cells:
            return
        a_s = max(d + 2 * k + 2 for _, d, k in cells)
        c, d, k = next(v for v in cells if v[1] + 2 * v[2] + 2 == a_s)  # the lowest column among equals
        V = A * a_s - 2 * s
        if best["B"] is None or V > best["B"]:
            best.update(B=V, s=s, te=k + 1, qe=d + k + 1, tie_cols=sum(1 for v in cells if v[1] + 2 * v[2] + 2 == a_s), tie_later=0)
        elif V == best["B"]:
            best["tie_later"] += 1
        F = max(F, a_s)

    def result(n_iter, s_stop, why):
        return ExtRef(best["s"], n_iter, best["te"], best["qe"], best["B"], s_stop, why, F, best["tie_cols"], best["tie_later"])

    k0 = extend(0, -1)
    H0 = dead.copy()
    H0[tl + 1] = k0
    steps_1_to_3(0, [(tl + 1, 0, k0)])
    if is_end(0, k0):
        return result(0, 0, 0)
    Hs, E1s, F1s, E2s, F2s = [H0], [dead], [dead], [dead], [dead]
    get = lambda rows, s: rows[s] if s >= 0 else dead  # noqa: E731
    wf_lo = wf_hi = tl + 1
    n_iter, s = 0, 0
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
        cells, end = [], False
        for n, col in enumerate(c):
            d, k = int(col) - 1 - tl, int(nh[n])
            if in_matrix(d, k):
                k = extend(d, k)
                nh[n] = k
                cells.append((int(col), d, k))
                end = end or is_end(d, k)
        for rows, vals in ((Hs, nh), (E1s, ne1), (F1s, nf1), (E2s, ne2), (F2s, nf2)):
            r = dead.copy()
            r[lo:hi + 1] = vals
            rows.append(r)
            if s - depth - 1 >= 0:
                rows[s - depth - 1] = None
        steps_1_to_3(s, cells)
        if end:
            return result(n_iter, s, 0)
        if Z >= 0 and best["B"] - (A * F - 2 * s) > Z:
            return result(n_iter, s, 1)


def dp_matrix(t: bytes, q: bytes, pen) -> np.ndarray:
    """D[i][j]: the cheapest global alignment of q[0, i) with t[0, j); a gap of L bases costs min(o1 + L e1, o2 + L e2)."""
    x, o1, e1, o2, e2 = pen
    tl, ql = len(t), len(q)
    ta = np.frombuffer(t, dtype=np.uint8)
    idx = np.arange(tl + 1, dtype=np.int64)
    D = np.empty((ql + 1, tl + 1), dtype=np.int32)
    H = F1 = F2 = None
    for i in range(ql + 1):
        if i == 0:
            Ht = np.full(tl + 1, DP_INF, dtype=np.int64)
            Ht[0] = 0
            F1 = np.full(tl + 1, DP_INF, dtype=np.int64)
            F2 = np.full(tl + 1, DP_INF, dtype=np.int64)
        else:
            F1 = np.minimum(F1 + e1, H + o1 + e1)  # query base i-1 against a gap
            F2 = np.minimum(F2 + e2, H + o2 + e2)
            Ht = np.minimum(F1, F2)
            if tl:
                Ht[1:] = np.minimum(Ht[1:], H[:-1] + np.where(ta == q[i - 1], 0, x))
        H = Ht.copy()
        for o, e in ((o1, e1), (o2, e2)):  # target bases against a gap: never opened from a cell that itself ends in one (o >= 0)
            pm = np.minimum.accumulate(Ht + o - e * idx)
            if tl:
                H[1:] = np.minimum(H[1:], pm[:-1] + e * idx[1:])
        H = np.minimum(H, DP_INF)
        D[i] = H
    return D


def dp_best(t: bytes, q: bytes, pen, A: int):
    """-> (the best V among the cells no dearer than the cheapest cell of the matrix's far edges, that cheapest penalty s_end, D)."""
    D = dp_matrix(t, q, pen)
    s_end = int(min(D[-1].min(), D[:, -1].min()))
    ij = np.add.outer(np.arange(D.shape[0], dtype=np.int64), np.arange(D.shape[1], dtype=np.int64))
    V = np.where(D <= s_end, A * ij - 2 * D.astype(np.int64), -1)
    return int(V.max()), s_end, D


def check_ext_cigar(mw, opt, t: bytes, q: bytes, words, rng, s: int) -> None:
    """Asserts that rng = (0, te, 0, qe) lies inside the pair, that `words` align t[0, te) with q[0, qe) and that they cost s."""
    tb, te, qb, qe = (int(v) for v in rng)
    assert tb == 0 and qb == 0, rng
    assert 0 <= te <= len(t) and 0 <= qe <= len(q), rng
    j = i = 0
    prev = -1
    for w in words:
        op, n = int(w) & 0xf, int(w) >> 4
        assert n > 0 and op != prev, ("empty or unmerged run", [int(v) for v in words])
        prev = op
        if op == 7:
            assert j + n <= te and i + n <= qe and t[j:j + n] == q[i:i + n], ("= run over unequal bases", j, i, n)
            j, i = j + n, i + n
        elif op == 8:
            assert j + n <= te and i + n <= qe and all(t[j + k] != q[i + k] for k in range(n)), ("X run over equal bases", j, i, n)
            j, i = j + n, i + n
        elif op == 1:
            i += n
        elif op == 2:
            j += n
        else:
            raise AssertionError(f"operator {op} in an extension's CIGAR")
    assert (j, i) == (te, qe), ("the words do not consume the ranges", (j, i), rng)
    sc, ct, cq = mw.cigar2score(opt, [int(w) for w in words])
    assert (sc, ct, cq) == (s, te, qe), ((sc, ct, cq), s, rng)
