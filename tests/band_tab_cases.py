"""Inputs of the tests of the packed band kernel's table form (miniwfa_amd/csrc/mwf_band2_tab.hip: the first probe of the match extension reads one halfword
per sequence and column from per-position 8-mer tables; a run of FULL = 8 or more matches continues in the per-lane and whole-wave walks).  Built on the CPU:

  runs       exact-match runs of 6 ... 73 bases behind a substitution — around the new FULL (8), the old one (16), and past the four per-lane trips (8 + 4 x 16 = 72)
             into the whole-wave walk — each with room left and ending exactly at the end of the target, of the query, of both
  final      final runs of 1 ... 9 bases on diagonal ql - tl in {-3, 0, +3}
  tabalign   a 1 ... 15-base deletion or insertion near the start: target and query probe positions take every pair of residues mod 16
  long       an identical 3 kb pair and a pair with one 1500-base exact run
  fuzz       64 seeded pairs of 500 - 2500 bases at 1, 5, 15, 30 %, unrelated and length-skewed
  fallback   one short pair, run with the LDS budget of the table form lowered below what it needs

tests/test_band_tab_cpu.py asserts what every case is chosen for; tests/test_band_tab_gpu.py runs them."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from fuzzlib import skewed_pairs, synth_pair   # (the generators tests/fuzzlib.py fuzzes the band kernels with)
from oracle.pyoracle import make_opt
import band_matrix as bm

DEFAULT = bm.PEN["default"]
FULL, FULL_PLAIN, LANE_TRIPS = 8, 16, 4           # mwf_band2_kernel.h: FULL of the table form and of the plain 2-bit probe; per-lane trips of sixteen bases
WAVE_WALK_FROM = FULL + 16 * LANE_TRIPS            # a run longer than this is finished by the whole wave
RUNS = (6, 7, 8, 9, 10, 15, 16, 17, 24, 73)
ENDS = ("target", "query", "both")
G3, G4 = bm.GEOMS[(512, 3, 0)], bm.GEOMS[(512, 4, 0)]

ACGT = b"ACGT"
# a run the case is about: it starts at target position ti / query position qi behind a substitution, is exactly n bases long, and ends with `end`:
# "room" (a mismatch behind it), or exactly at the end of the "target", the "query", or "both"
Run = namedtuple("Run", "ti qi n end")


def _rand(rng, n: int) -> bytes:
    return bm._rand(rng, n)


def _other(rng, b: int) -> bytes:
    return bytes([ACGT[(ACGT.index(bytes([b])) + int(rng.integers(1, 4))) % 4]])


def _sub_run(rng, t: bytearray, q: bytearray, n: int):
    """Append a substitution and an exact run of n bases whose first base differs from nothing by chance: returns the run's start."""
    a = _rand(rng, 1)
    t += a
    q += _other(rng, a[0])
    r = _rand(rng, n)
    ti, qi = len(t), len(q)
    t += r
    q += r
    return ti, qi


def lce(t: bytes, q: bytes, i: int, j: int) -> int:
    n = 0
    while i + n < len(t) and j + n < len(q) and t[i + n] == q[j + n]:
        n += 1
    return n


def runs_pairs():
    """[(t, q, [Run])]: one pair with every run length with room left, then one pair per length and end."""
    rng = np.random.default_rng(8016)
    out = []
    for lead in (301, 302, 303, 304):   # (column tl + 1 of the main diagonal: every position of a lane's quad)
        t, q, runs = bytearray(_rand(rng, lead)), None, []
        q = bytearray(t)
        for n in RUNS:
            ti, qi = _sub_run(rng, t, q, n)
            runs.append(Run(ti, qi, n, "room"))
        _sub_run(rng, t, q, 150)
        out.append((bytes(t), bytes(q), runs))
    k = 0
    for n in RUNS:
        for end in ENDS:
            # (the lead's length puts column tl + 1 of the main diagonal on quad position k mod 4: over the cases, every position)
            t = bytearray(_rand(rng, 300 + (k - 1 - 42 - n - (5 if end == "query" else 0)) % 4))
            q = bytearray(t)
            k += 1
            _sub_run(rng, t, q, 40)
            ti, qi = _sub_run(rng, t, q, n)
            if end == "target":
                q += _other(rng, t[ti]) + _rand(rng, 4)   # the query runs on: five more bases
            elif end == "query":
                t += _other(rng, q[qi]) + _rand(rng, 4)
            out.append((bytes(t), bytes(q), [Run(ti, qi, n, end)]))
    return out


def final_pairs():
    """[(t, q, [Run])]: a final run of 1 ... 9 bases ending at both ends, on diagonal ql - tl = -3, 0, +3 (a three-base gap after sixty bases)."""
    rng = np.random.default_rng(9001)
    out = []
    for n in range(1, 10):
        for dl in (-3, 0, 3):
            head, body = _rand(rng, 60), _rand(rng, 240 + n % 4)
            t = bytearray(head + (_rand(rng, 3) if dl < 0 else b"") + body)
            q = bytearray(head + (_rand(rng, 3) if dl > 0 else b"") + body)
            ti, qi = _sub_run(rng, t, q, n)
            out.append((bytes(t), bytes(q), [Run(ti, qi, n, "both")]))
    return out


def tabalign_pairs():
    """[(t, q, k)]: k > 0: k bases deleted from the query after twenty bases, k < 0: -k bases inserted; the rest 2 kb at 6 % substitutions."""
    out = []
    for k in range(1, 16):
        for sign in (1, -1):
            rng = np.random.default_rng(7000 + 16 * k + sign)
            head, gap = _rand(rng, 20), _rand(rng, k)
            body = bytearray(_rand(rng, 2000 + k))
            mut = bytearray(body)
            for p in np.nonzero(rng.random(len(body)) < 0.06)[0]:
                mut[p] = _other(rng, body[p])[0]
            t = head + (gap if sign > 0 else b"") + bytes(body)
            q = head + (gap if sign < 0 else b"") + bytes(mut)
            out.append((t, q, sign * k))
    return out


def long_pairs(where: bool = False):
    """The identical pair and the pair with the 1500-base run; where: that run as a Run instead."""
    rng = np.random.default_rng(1500)
    ident = _rand(rng, 3000)
    a, b = synth_pair(15001, 700, 0.08), synth_pair(15002, 700, 0.08)
    mid = _rand(rng, 1500)
    ta, qa = a[0] + b"A", a[1] + b"C"      # (a mismatch on either side of the run, whatever the flanks' last bases)
    if where:
        return Run(len(ta), len(qa), 1500, "room")
    return [(ident, ident), (ta + mid + b"G" + b[0], qa + mid + b"T" + b[1])]


FUZZ_N = 64


def fuzz_pairs():
    """64 seeded pairs of 500 - 2500 bases from tests/fuzzlib.py's generators: related at 1, 5, 15, 30 %, unrelated, length-skewed."""
    rng = np.random.default_rng(64064)
    out = []
    for i in range(48):
        out.append(synth_pair(640000 + i, int(rng.integers(500, 2501)), (0.01, 0.05, 0.15, 0.30)[i % 4]))
    for _ in range(8):
        out.append((_rand(rng, int(rng.integers(500, 2501))), _rand(rng, int(rng.integers(500, 2501)))))
    out += [(t, q) for t, q in skewed_pairs(64, 24, 500, 2500) if abs(len(t) - len(q)) > 200][:8]
    assert len(out) == FUZZ_N
    return out


def fallback_pair():
    return synth_pair(4242, 900, 0.05)


GROUPS = ("runs", "final", "tabalign", "long", "fuzz")
_groups: dict = {}


def group(name: str):
    """[(t, q)] of a group, built once."""
    if name not in _groups:
        build = {"runs": lambda: [(t, q) for t, q, _ in runs_pairs()], "final": lambda: [(t, q) for t, q, _ in final_pairs()],
                 "tabalign": lambda: [(t, q) for t, q, _ in tabalign_pairs()], "long": long_pairs, "fuzz": fuzz_pairs}[name]
        _groups[name] = build()
    return _groups[name]


_expected: dict = {}


def expected(orc, name: str):
    """[(s, n_iter, cigar)] of a group from the oracle, with CIGAR, computed once (s and n_iter of a score-only run are the same)."""
    if name not in _expected:
        pairs = [fallback_pair()] if name == "fallback" else group(name)
        _expected[name] = orc.align_many(pairs, make_opt(flag=1, **DEFAULT), threads=bm.ORACLE_THREADS)[0]
    return _expected[name]


def path_cells(t: bytes, q: bytes, cigar):
    """[(i, j, score so far)] of every diagonal step of the alignment (target index, query index, penalty paid BEFORE the step), from the CIGAR words."""
    from miniwfa_amd.api import CIGAR_CHARS
    i = j = s = 0
    out = []
    for w in cigar or []:
        n, op = int(w) >> 4, CIGAR_CHARS[int(w) & 0xf]
        if op in "M=X":
            for _ in range(n):
                out.append((i, j, s))
                s += 0 if t[i] == q[j] else DEFAULT["x"]
                i, j = i + 1, j + 1
        else:
            s += min(DEFAULT["o1"] + n * DEFAULT["e1"], DEFAULT["o2"] + n * DEFAULT["e2"])
            if op == "I":
                j += n
            else:
                i += n
    assert (i, j) == (len(t), len(q)), (i, j, len(t), len(q))
    return out


def lands(g, lohi: np.ndarray, tl: int, d: int, s: int):
    """(chunk, wave, slot, lane, column of the quad) of diagonal d at penalty s under the slot mapping that starts at that penalty's first chunk; None outside its window.
    (The inverse of the kernel's remap(): tests/test_band_tab_cpu.py applies remap() forwards to what this returns.)"""
    lo, hi = int(lohi[s - 1][0]), int(lohi[s - 1][1])
    if not lo <= d <= hi:
        return None
    c = d + tl + 1
    chunk, nw, n = c >> 8, g.T // 64, bm.nwk(g)
    gl = max(lo + tl + 1 - 1, 1) >> 8
    base = gl - gl % n
    rel = (chunk - base) % n
    return chunk, rel % nw, rel // nw, (c & 255) >> 2, c & 3


TAB_OBJ = os.path.join(bm.ROOT, "miniwfa_amd", "csrc", "build", "mwf_band2_tab.hip.o")


def tab_object_kernels():
    """The wfa_band2_tab_kernel<...> instantiations in mwf_band2_tab.hip.o's gfx950 code object (band_matrix.Inst), and every other kernel of that object."""
    got = bm.device_kernels(TAB_OBJ, "wfa_band2_tab_kernel")
    assert not isinstance(got, str), got
    return set(got[0]), {re.search(r"(\w+)<", name).group(1) for name in got[1]}
