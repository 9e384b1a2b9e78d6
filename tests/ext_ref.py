"""Yardsticks for the extension alignment (include/miniwfa.h, mwf_ext_t), independent of the library's kernel:

  wfa_ext          the header's rule restated on ends_ref.sweep — the slices of a pass from the origin cell, with the reference's stripe shrink every 256
                   penalties over the last nH slices — as ends_ref.wfa_ends is: steps 1 - 3 on every penalty's tested cells, then the two ends of the pass;
  dp_best          a full prefix Gotoh matrix D[i][j] from the origin (0, 0): s_end = min of D over the last row and the last column, and the yardstick
                   max{A (i + j) - 2 D[i][j] : D[i][j] <= s_end}, which a pass without the drop rule must return exactly, with s_stop == s_end;
  check_ext_cigar  a checker for an extension's CIGAR and ranges: tb = qb = 0, the words consume t[0, te) / q[0, qe) and cost s.

Used by tests/test_ext_cpu.py (which checks them against each other) and tests/test_ext_gpu.py."""
from __future__ import annotations

import collections

import numpy as np

from ends_ref import sweep

ExtRef = collections.namedtuple("ExtRef", "s n_iter te qe V s_stop why F tie_cols tie_later")
DP_INF = 1 << 28


def wfa_ext(t: bytes, q: bytes, pen, A: int, Z: int, trace=None, shrinks=None) -> ExtRef:
    """The extension pass: -> the remembered cell (s, te, qe), n_iter, info (V, s_stop, why, F), and two counts the case list is chosen by: tie_cols, the
    columns that held a_s at the answer's penalty, and tie_later, the later penalties whose best V equalled B without replacing it.  trace, shrinks: see ends_ref.sweep."""
    tl, ql = len(t), len(q)
    best = dict(B=None, s=0, te=0, qe=0, tie_cols=0, tie_later=0)
    F = 0
    for s, n_iter, c, d, k in sweep(t, q, pen, tl + 1, tl + 1, trace, shrinks):  # c, d, k: every tested cell of penalty s, columns ascending
        if c.size:  # steps 1 - 3
            a = d + 2 * k + 2
            n = int(a.argmax())  # the lowest column among equals
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


def dp_answer(t: bytes, q: bytes, pen, A: int, te: int, qe: int):
    """dp_best without the matrix: -> (V, s_end, D[qe][te])."""
    V, s_end, D = dp_best(t, q, pen, A)
    return V, s_end, int(D[qe][te])


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
