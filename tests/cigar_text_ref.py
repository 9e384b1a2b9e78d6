"""What tests/test_cigar_text_cpu.py and tests/test_cigar_text_gpu.py share: an independent pure-Python restatement of the six text products of a
CIGAR (include/miniwfa.h, MWF_TXT_*) and of renderability, the hand pair's six strings as literals, and the pair whose '=' runs are exactly 9, 10,
99, 100, 999 and 1000 bases long.  The restatement expands the words into alignment columns first and derives every product from the columns —
another route than the word-by-word emitters of the library."""
from itertools import groupby

from cigar_ops_ref import OP_I, OP_D, OP_EQ, OP_X

TXT_CIGAR, TXT_SAM, TXT_CS, TXT_MD, TXT_ROW_T, TXT_ROW_Q, TXT_KINDS = range(7)
KINDS = tuple(range(TXT_KINDS))

# 10= 1X 3D 8= 2I 12= on cigar_ops_ref.HAND_T / HAND_Q
HAND_TEXT = {
    TXT_CIGAR: b"10=1X3D8=2I12=",
    TXT_SAM: b"11M3D8M2I12M",
    TXT_CS: b":10*gt-cat:8+tt:12",
    TXT_MD: b"10G0^CAT20",
    TXT_ROW_T: b"ACGTTGCAACGCATGGATCCTA--CGATCGGATTAC",
    TXT_ROW_Q: b"ACGTTGCAACT---GGATCCTATTCGATCGGATTAC",
}


def renderable(words, tl: int, ql: int) -> bool:
    ti = qj = 0
    for word in words:
        op, ln = int(word) & 15, int(word) >> 4
        if op not in (OP_I, OP_D, OP_EQ, OP_X) or ln < 1:
            return False
        ti += ln if op != OP_I else 0
        qj += ln if op != OP_D else 0
        if ti > tl or qj > ql:
            return False
    return (ti, qj) == (tl, ql)


def _lower(b: int) -> int:
    return b | 0x20 if 0x41 <= b <= 0x5A else b


def _columns(words, t: bytes, q: bytes):
    """One (op, word index, target byte or None, query byte or None) per alignment column."""
    cols, ti, qj = [], 0, 0
    for w, word in enumerate(words):
        op, ln = int(word) & 15, int(word) >> 4
        for _ in range(ln):
            tb = qb = None
            if op != OP_I:
                tb, ti = t[ti], ti + 1
            if op != OP_D:
                qb, qj = q[qj], qj + 1
            cols.append((op, w, tb, qb))
    return cols


def py_text(kind: int, words, t: bytes, q: bytes):
    """The text as bytes, or None when the words are not renderable for the pair (or kind is not one of the six)."""
    words = [int(w) for w in words]
    if kind not in KINDS or not renderable(words, len(t), len(q)):
        return None
    return _render(kind, _columns(words, t, q))


def py_texts(words, t: bytes, q: bytes):
    """All six products (a list indexed by kind; the columns are expanded once), or None when the words are not renderable."""
    words = [int(w) for w in words]
    if not renderable(words, len(t), len(q)):
        return None
    cols = _columns(words, t, q)
    return [_render(kind, cols) for kind in KINDS]


def _render(kind: int, cols) -> bytes:
    out = bytearray()
    if kind == TXT_CIGAR:
        for (op, w), g in groupby(cols, key=lambda c: (c[0], c[1])):
            out += b"%d%c" % (len(list(g)), b"MIDNSHP=X"[op])
    elif kind == TXT_SAM:
        # columns under = / X merge across words; an I or D word stays one item
        for (cls, w), g in groupby(cols, key=lambda c: ("M", -1) if c[0] in (OP_EQ, OP_X) else ("ID"[c[0] - 1], c[1])):
            out += b"%d%s" % (len(list(g)), cls.encode())
    elif kind == TXT_CS:
        for (op, w), g in groupby(cols, key=lambda c: (c[0], c[1])):
            g = list(g)
            if op == OP_EQ:
                out += b":%d" % len(g)
            elif op == OP_X:
                for _, _, tb, qb in g:
                    out += bytes([0x2A, _lower(tb), _lower(qb)])
            elif op == OP_I:
                out += b"+" + bytes(_lower(c[3]) for c in g)
            else:
                out += b"-" + bytes(_lower(c[2]) for c in g)
    elif kind == TXT_MD:
        c, prev_del = 0, None
        for op, w, tb, qb in cols:
            if op == OP_EQ:
                c += 1
            elif op == OP_X:
                out += b"%d" % c + bytes([tb])
                c = 0
            elif op == OP_D:
                if prev_del != w:            # the first column of a D word
                    out += b"%d^" % c
                    c = 0
                out += bytes([tb])
            prev_del = w if op == OP_D else None
        out += b"%d" % c
    elif kind == TXT_ROW_T:
        out += bytes(0x2D if tb is None else tb for _, _, tb, _ in cols)
    else:
        out += bytes(0x2D if qb is None else qb for _, _, _, qb in cols)
    return bytes(out)


def digit_pair():
    """(t, q, words): '=' runs of exactly 9, 10, 99, 100, 999 and 1000 bases with single mismatches between them; lower-case letters, an N and a byte
    >= 0x80 among the bases — under the mismatches (cs lowers only A..Z there, MD copies verbatim) and inside the runs (rows verbatim)."""
    import random
    rng = random.Random(20)
    runs = (9, 10, 99, 100, 999, 1000)
    mism = ((ord("A"), ord("c")), (ord("N"), ord("g")), (0x80, ord("T")), (ord("t"), ord("A")), (ord("G"), 0xFE))
    t, q, words = bytearray(), bytearray(), []
    for k, n in enumerate(runs):
        run = bytearray(rng.choice(b"ACGTacgtN") for _ in range(n))
        run[n // 2] = 0x80 + k
        t += run
        q += run
        words.append(n << 4 | OP_EQ)
        if k < len(mism):
            t.append(mism[k][0])
            q.append(mism[k][1])
            words.append(1 << 4 | OP_X)
    return bytes(t), bytes(q), words
