"""What tests/test_cigar_ops_cpu.py and tests/test_cigar_ops_gpu.py share: an independent pure-Python / numpy restatement of the
summary rule (include/miniwfa.h, mwf_aln_summary_t) and of the coordinate maps, a hand-made pair whose CIGAR is known by construction,
and the malformed word sets derived from a CIGAR together with the first_bad each must give."""
import numpy as np

FIELDS = ("score", "t_len", "q_len", "n_eq", "n_x", "n_ins", "n_del", "n_ins_runs", "n_del_runs", "n_words", "first_bad", "flags")
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
INT32_MIN = -(1 << 31)


def _i32(v: int) -> int:
    """Truncation of a Python integer to int32 (what a store of the low 32 bits reads back as)."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def py_summary(pen, words, t: bytes, q: bytes) -> tuple:
    """The twelve fields, from the rule alone.  pen = (x, o1, e1, o2, e2).  Python integers do not overflow: truncation happens once, at the end."""
    x, o1, e1, o2, e2 = pen
    ta, qa = np.frombuffer(t, dtype=np.uint8), np.frombuffer(q, dtype=np.uint8)
    tl, ql = len(t), len(q)
    ti = qj = score = n_eq = n_x = n_ins = n_del = ri = rd = 0
    bad = []
    for w, word in enumerate(words):
        op, ln = int(word) & 15, int(word) >> 4
        if op not in (OP_I, OP_D, OP_EQ, OP_X):
            bad.append(w)                                            # (a): consumes nothing, counts nowhere
            continue
        on_t, on_q = op != OP_I, op != OP_D
        is_bad = (on_t and ti + ln > tl) or (on_q and qj + ln > ql)  # (b)
        if op in (OP_EQ, OP_X):
            m = min(ln, max(0, tl - ti), max(0, ql - qj))
            if m > 0:
                same = ta[ti:ti + m] == qa[qj:qj + m]
                is_bad = is_bad or bool((~same).any() if op == OP_EQ else same.any())   # (c)
            if op == OP_EQ:
                n_eq += ln
            else:
                n_x += ln
                score += ln * x
        else:
            score += min(o1 + ln * e1, o2 + ln * e2)
            if op == OP_I:
                n_ins += ln
                ri += 1
            else:
                n_del += ln
                rd += 1
        if is_bad:
            bad.append(w)
        ti += ln if on_t else 0
        qj += ln if on_q else 0
    first_bad = bad[0] if bad else (len(words) if (ti, qj) != (tl, ql) else -1)
    return tuple(_i32(v) for v in (score, ti, qj, n_eq, n_x, n_ins, n_del, ri, rd, len(words), first_bad, 1))


NO_CIGAR = (0,) * 10 + (-1, 0)   # the record of a pair without a CIGAR


def py_maps(words, tl: int, ql: int):
    """(query -> target, target -> query) of a VALID CIGAR, by numpy expansion."""
    q2t, t2q = np.full(ql, INT32_MIN, dtype=np.int64), np.full(tl, INT32_MIN, dtype=np.int64)
    ti = qj = 0
    for word in words:
        op, ln = int(word) & 15, int(word) >> 4
        if op in (OP_EQ, OP_X):
            q2t[qj:qj + ln] = np.arange(ti, ti + ln)
            t2q[ti:ti + ln] = np.arange(qj, qj + ln)
            ti, qj = ti + ln, qj + ln
        elif op == OP_I:
            q2t[qj:qj + ln] = -1 - ti
            qj += ln
        else:
            t2q[ti:ti + ln] = -1 - qj
            ti += ln
    assert (ti, qj) == (tl, ql)
    return q2t.astype(np.int32), t2q.astype(np.int32)


def rec(r) -> tuple:
    """A numpy SUMMARY_DTYPE record as a tuple of Python ints."""
    return tuple(int(r[f]) for f in FIELDS)


# ---- a pair whose CIGAR is known by construction: 10= 1X 3D 8= 2I 12=
HAND_T = b"ACGTTGCAAC" + b"G" + b"CAT" + b"GGATCCTA" + b"CGATCGGATTAC"           # 34 bases
HAND_Q = b"ACGTTGCAAC" + b"T" + b"GGATCCTA" + b"TT" + b"CGATCGGATTAC"            # 33 bases
HAND_WORDS = [10 << 4 | OP_EQ, 1 << 4 | OP_X, 3 << 4 | OP_D, 8 << 4 | OP_EQ, 2 << 4 | OP_I, 12 << 4 | OP_EQ]
DEFAULT_PEN = (4, 4, 2, 15, 1)
BIG = 0x0FFFFFFF
# Under the default penalties: X 4, 3D min(4+6, 15+3) = 10, 2I min(4+4, 15+2) = 8.
#                 score                t_len          q_len     n_eq n_x n_ins n_del runs  n_words first_bad flags
HAND_CASES = {
    "clean":        (HAND_WORDS,                                              (22, 34, 33, 30, 1, 2, 3, 1, 1, 6, -1, 1)),
    # the 8= in the middle becomes an op 15: it consumes nothing, everything behind it shifts (and no longer ends at the ends)
    "op15":         (HAND_WORDS[:3] + [8 << 4 | 15] + HAND_WORDS[4:],         (22, 26, 25, 22, 1, 2, 3, 1, 1, 6, 3, 1)),
    # the last = runs 7 bases past both ends: rule (b)
    "eq_plus7":     (HAND_WORDS[:5] + [19 << 4 | OP_EQ],                      (22, 41, 40, 37, 1, 2, 3, 1, 1, 6, 5, 1)),
    # the first = swallows the mismatch behind it (t[10] = G, q[10] = T): rule (c)
    "eq_plus7_mid": ([17 << 4 | OP_EQ] + HAND_WORDS[1:],                      (22, 41, 40, 37, 1, 2, 3, 1, 1, 6, 0, 1)),
    # the last word dropped: every word is fine, the ends are not reached
    "dropped":      (HAND_WORDS[:5],                                          (22, 22, 21, 18, 1, 2, 3, 1, 1, 5, 5, 1)),
    # the deletion is 0x0fffffff long: min(4 + 2 L, 15 + L) = 15 + L
    "huge":         (HAND_WORDS[:2] + [BIG << 4 | OP_D] + HAND_WORDS[3:],     (4 + 15 + BIG + 8, 31 + BIG, 33, 30, 1, 2, BIG, 1, 1, 6, 2, 1)),
    # twenty of them as =: the sums pass 2^32 and are truncated on store (20 * 0x0fffffff = 0x13FFFFFEC)
    "wrap":         ([BIG << 4 | OP_EQ] * 20,                                 (0, 0x3FFFFFEC, 0x3FFFFFEC, 0x3FFFFFEC, 0, 0, 0, 0, 0, 20, 0, 1)),
    "no_words":     ([],                                                      (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)),
}
EMPTY_PAIR_RECORD = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 1)   # no words for an empty pair: a valid (empty) alignment


def malformed_variants(words):
    """The malformed set of the CPU tests applied to a real, valid CIGAR whose last word is an '=': name -> (words, first_bad)."""
    words = [int(w) for w in words]
    n, m = len(words), len(words) // 2
    assert n >= 3 and words[-1] & 15 == OP_EQ
    out = {
        "op15": (words[:m] + [(words[m] & ~15) | 15] + words[m + 1:], m),
        "eq_plus7": (words[:-1] + [words[-1] + (7 << 4)], n - 1),       # past both ends: rule (b)
        "dropped": (words[:-1], n - 1),
        "huge": (words[:m] + [BIG << 4 | (words[m] & 15)] + words[m + 1:], m),
    }
    for k in range(n - 1):  # an '=' followed by an 'X' swallows a mismatching base: rule (c), whatever follows
        if words[k] & 15 == OP_EQ and words[k + 1] & 15 == OP_X:
            out["eq_plus7_mid"] = (words[:k] + [words[k] + (7 << 4)] + words[k + 1:], k)
            break
    return out
