"""The shared case list of the extension alignment's tests (tests/test_ext_cpu.py, tests/test_ext_gpu.py) and its restated answers, computed once per process.

A case is a batch of pairs under one (A, Z) and the penalty sets it is run under: both sets of tests/test_ends_gpu.py where the pass ends before the
first shrink, s_stop < 256; test_ext_cpu.py checks that every listed combination does.  (Beyond it: tests/ends_matrix.py.)"""
from __future__ import annotations

import collections
import functools

from miniwfa_amd.synth import mutate, random_seq, synth_pair

import ext_ref as xr

PEN_A, PEN_B = (4, 4, 2, 15, 1), (4, 6, 3, 26, 1)
BOTH = (PEN_A, PEN_B)

Case = collections.namedtuple("Case", "name pairs A Z pens")


def junk_tail(seed: int, good: int, p: float, n: int):
    """synth_pair(seed, good, p) with n unrelated bases appended to the target and n others to the query."""
    t, q = synth_pair(seed, good, p)
    return t + random_seq(seed + 7001, n), q + random_seq(seed + 9001, n)


_TWO = bytes.maketrans(b"GT", b"AC")


def small_pair(seed: int, letters: int, p: float):
    """What the seeded search for ties ran over (seeds 0 ... 299, two and four letters, p 0.15, 0.3 and 0.5, A 1 and 2): 20 ... 120 bases, the query the
    target mutated at rate p."""
    n = 20 + seed * 37 % 101
    t = random_seq(50000 + seed, n)
    q = mutate(t, 60000 + seed, p)
    return (t.translate(_TWO), q.translate(_TWO)) if letters == 2 else (t, q)


# (seed, letters, p, A) found by the search (test_ext_cpu.py checks what they promise under PEN_A): the first list holds pairs where two or more columns tie
# for a_s at the answer's penalty, the second pairs where a later penalty's best V ties B
TIE_COLS = ((79, 2, 0.3, 2), (235, 2, 0.3, 2), (0, 2, 0.5, 2), (293, 4, 0.5, 2))
TIE_LATER = ((3, 4, 0.15, 1), (14, 4, 0.15, 1), (15, 4, 0.15, 2))


def mixed_batch():
    """64 pairs of every kind above, none longer than 600 bases."""
    pairs = []
    for k in range(64):
        kind = k % 8
        if kind == 0:
            pairs.append(junk_tail(300 + k, 200 + 3 * k, 0.05, 100 + k))
        elif kind == 1:
            pairs.append(synth_pair(400 + k, 150 + 5 * k, 0.08))
        elif kind == 2:
            pairs.append((random_seq(500 + k, 90 + k), random_seq(600 + k, 70 + 2 * k)))
        elif kind == 3:
            pairs.append(small_pair(k, 2, 0.3))
        elif kind == 4:
            pairs.append(small_pair(k, 4, 0.15))
        elif kind == 5:
            t = random_seq(700 + k, 40 + 4 * k)
            pairs.append((t, t) if k % 16 == 5 else (t + random_seq(800 + k, 150), t[:len(t) // 2]))
        elif kind == 6:
            pairs.append(junk_tail(900 + k, 60 + k, 0.02, 260))
        else:
            pairs.append([(b"", b"ACGT"), (b"ACGTAC", b""), (b"", b""), (b"A", b"A"), (b"A", b"C"), (b"ACGT", b"ACGA"), (b"AC", b"ACGTACGT"), (b"TTTTTTTT", b"TTTT")][k // 8])
    return pairs


@functools.lru_cache(maxsize=None)
def cases():
    t200 = random_seq(1, 200)
    d = synth_pair(21, 400, 0.05)
    e = synth_pair(23, 300, 0.05)
    g = synth_pair(31, 4200, 0.01)
    out = [
        Case("a-identical", [(t200, t200)], 1, -1, BOTH),
        Case("b-empty", [(b"", b"ACGT"), (b"ACGTAC", b""), (b"", b"")], 1, -1, BOTH),
        Case("b-empty-drop", [(b"", b"ACGT"), (b"ACGTAC", b""), (b"", b"")], 2, 0, BOTH),
        Case("c-unrelated-drop", [(random_seq(2, 200), random_seq(3, 180))], 1, 30, BOTH),
        Case("c-unrelated-end", [(random_seq(4, 60), random_seq(5, 50))], 1, -1, BOTH),
        Case("d-related-A1", [d], 1, -1, BOTH),
        Case("d-related-A2", [d], 2, -1, BOTH),
        Case("e-long-target", [(e[0] + random_seq(24, 150), e[1])], 1, -1, BOTH),
        Case("f-junk40-end", [junk_tail(11, 300, 0.05, 40)], 1, -1, BOTH),
        Case("f-junk200-z50", [junk_tail(11, 300, 0.05, 200)], 1, 50, BOTH),
        Case("f-junk200-z100", [junk_tail(11, 300, 0.05, 200)], 1, 100, BOTH),
        Case("g-4200", [g], 1, -1, BOTH),
        Case("g-4200-junk300-z80", [(g[0] + random_seq(31 + 7001, 300), g[1] + random_seq(31 + 9001, 300))], 1, 80, (PEN_A,)),
    ]
    out += [Case(f"h-tie-cols-{seed}-{letters}", [small_pair(seed, letters, p)], A, -1, BOTH) for seed, letters, p, A in TIE_COLS]
    out += [Case(f"h-tie-later-{seed}-{letters}", [small_pair(seed, letters, p)], A, -1, BOTH) for seed, letters, p, A in TIE_LATER]
    # (without a drop rule the batch's unrelated pairs run beyond penalty 256, and so do they under A = 2 and the first penalty set, where the frontier's
    # two bases per penalty pay for every penalty: the drop never comes)
    out += [Case("i-mixed-z40", mixed_batch(), 1, 40, BOTH), Case("i-mixed-A2-z25", mixed_batch(), 2, 25, (PEN_B,))]
    return tuple(out)


def runs():
    """(case, penalty set) of every combination of the list."""
    return [(c, pen) for c in cases() for pen in c.pens]


@functools.lru_cache(maxsize=None)
def _want(name: str, pen):
    c = next(c for c in cases() if c.name == name)
    return tuple(xr.wfa_ext(t, q, pen, c.A, c.Z) for t, q in c.pairs)


def want(case: Case, pen):
    """The restated answers of a case's pairs under a penalty set, computed once and shared."""
    return _want(case.name, pen)
