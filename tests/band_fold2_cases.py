"""Inputs of the tests of the table form's second fold (miniwfa_amd/csrc/mwf_band2_tab2.hip; mwf_band2_kernel.h, band2_pass: kFold2 — the row the second gap piece
opens from is folded into the E2 / F2 registers one penalty ahead, and a chunk that left the window ages through o2 + D masked runs).  Built on the CPU from the
oracle's CIGAR and band trace:

  gaps      one deletion or insertion of 12 ... 40 bases (from 12 on the second piece is the cheaper one under the default set: 15 + n < 4 + 2 n) between exact
            flanks: the gap leaves the main diagonal in each of a lane's four quad columns, across a chunk edge (lane 0 <-> lane 63 of the neighbouring slot: the edge
            table) in both directions, and across the slot wrap (slot NWK - 1 <-> slot 0: column 6144 on three chunk slots, 8192 on four).  The wrap pairs pay an
            insertion of 5.8 / 7.9 kb first to get there: with pairs of 3 kb no column beyond 6001 exists.
  adjacent  two long gaps on neighbouring diagonals fewer than o2 penalties apart: a gap opened from a row that a gap extension also reaches
  shrinks   unrelated and length-skewed pairs of 0.3 - 3 kb whose shrink at penalty 512 takes the window's start, and its end, across a chunk boundary: the chunk
            left behind ages through the longer period (and tests/band_epoch_cases.py's cross-shrink pairs).  At penalty 256 no pair of these sizes loses a chunk: the
            window is 483 columns wide then and every diagonal in it still holds an in-matrix offset (the candidates' windows of penalty 257 are those of 256 plus one
            column either side) — the first shrink that moves an edge is the one at 512
  climb     the climbing-start pairs of tests/band_epoch_cases.py (imported): the upward remap waits the new period
  stops     max_s / max_iter stops, and pairs whose end cell lies in a chunk that has run for more than o2 penalties
  fuzz      64 pairs, seeds fixed here
  pens      penalty sets on both sides of band2_tab2_supported: o2 = 3 | o2 = 2 (refused), o2 + e2 at the bound | one above (refused), and two in between

tests/test_band_fold2_cpu.py asserts what every case is chosen for; tests/test_band_fold2_gpu.py runs them on 512 threads x 3 and x 4 chunk slots."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from oracle.pyoracle import make_opt
from miniwfa_amd.synth import synth_pair, skewed_pairs
import band_matrix as bm
import band_epoch_cases as ec
import band_tab_cases as tc

DEFAULT = bm.PEN["default"]
G3, G4 = bm.GEOMS[(512, 3, 0)], bm.GEOMS[(512, 4, 0)]
GEOM = {3: G3, 4: G4}
KERNEL_H = os.path.join(bm.ROOT, "miniwfa_amd", "csrc", "mwf_band2_kernel.h")
TAB2_OBJ = os.path.join(bm.ROOT, "miniwfa_amd", "csrc", "build", "mwf_band2_tab2.hip.o")
FOLD2_MAX_LAG = int(re.search(r"constexpr\s+int\s+kFold2MaxLag\s*=\s*(\d+)", open(KERNEL_H).read()).group(1))   # o2 + e2 up to it takes the second fold
AGE = FOLD2_MAX_LAG - 1 + 3   # kAgeOut of the form: bound - e2 + D, D = max(e1, e2) + 1 = 3
GAP_LENGTHS = (12, 13, 20, 31, 40)


def supported(p: dict) -> bool:
    """band2_tab2_supported, restated: the table form's sets (gap extensions (2,1), o1 == x folds), 3 <= o2, o2 + e2 within the bound."""
    return bm.pen_folds(p) and p["e1"] == 2 and p["e2"] == 1 and p["o2"] >= 3 and p["o2"] + p["e2"] <= FOLD2_MAX_LAG


PENS = {
    "o2_3": dict(x=4, o1=4, e1=2, o2=3, e2=1),
    "o2_2": dict(x=4, o1=4, e1=2, o2=2, e2=1),
    "o2_9": dict(x=4, o1=4, e1=2, o2=9, e2=1),
    "o2_5_x2": dict(x=2, o1=2, e1=2, o2=5, e2=1),
    "lag_bound": dict(x=4, o1=4, e1=2, o2=FOLD2_MAX_LAG - 1, e2=1),
    "lag_above": dict(x=4, o1=4, e1=2, o2=FOLD2_MAX_LAG, e2=1),
}
TAKES = {"o2_3": True, "o2_2": False, "o2_9": True, "o2_5_x2": True, "lag_bound": True, "lag_above": False}


def _rand(rng, n):
    return bm._rand(rng, n)


# ---- gaps -------------------------------------------------------------------------------------------------------------------------------
Gap = namedtuple("Gap", "t q n sign kind col")   # sign +1: insertion (E2, the column rises), -1: deletion (F2); col: the main diagonal's column where the gap opens


def _gap_pair(rng, tl_main: int, n: int, sign: int, head: bytes = b""):
    """Flanks of tl_main bases in all, split in the middle, exact but for one substitution per flank (so that the chunk has run a few penalties), the gap between
    them; `head`: unrelated bases in front of the query (the wrap pairs' climb)."""
    la = tl_main // 2
    a, b, x = bytearray(_rand(rng, la)), bytearray(_rand(rng, tl_main - la)), _rand(rng, n)
    # the gap's bases must not continue either flank, or the gap could shift: make its ends differ from the neighbouring flank bases
    x = tc._other(rng, b[0]) + x[1:-1] + tc._other(rng, a[-1])
    qa, qb = bytearray(a), bytearray(b)
    qa[la // 3] = tc._other(rng, a[la // 3])[0]
    qb[len(b) // 2] = tc._other(rng, b[len(b) // 2])[0]
    if sign < 0:
        return bytes(a) + x + bytes(b), head + bytes(qa) + bytes(qb)
    return bytes(a) + bytes(b), head + bytes(qa) + x + bytes(qb)


def gap_pairs():
    out = []
    rng = np.random.default_rng(20251)
    for n in GAP_LENGTHS:
        for sign in (1, -1):
            for r in range(4):   # quad column of the diagonal the gap leaves: (tl + 1) & 3
                tl = 380 + ((r - 1 - 380) & 3)   # (column 381 ... 384: forty columns either way stay inside chunk 1)
                tl_main = tl - (n if sign < 0 else 0)
                t, q = _gap_pair(rng, tl_main, n, sign)
                out.append(Gap(t, q, n, sign, f"quad{r}", len(t) + 1))
            # across a chunk edge: the gap starts n // 2 columns from column 512 / 768 and ends beyond it
            edge = 512 if sign < 0 else 768
            tl = edge - 1 + (n // 2 if sign < 0 else -(n // 2))
            t, q = _gap_pair(rng, tl - (n if sign < 0 else 0), n, sign)
            out.append(Gap(t, q, n, sign, "edge", len(t) + 1))
    return out


def wrap_pairs():
    """The gap crosses the column between slot NWK - 1 and slot 0: 256 NWK = 6144 (three chunk slots per wave) and 8192 (four)."""
    out = []
    rng = np.random.default_rng(20252)
    for nwk in (24, 32):
        for n, sign in ((20, 1), (31, -1)):
            tl_main = 300
            tl = tl_main + (n if sign < 0 else 0)
            start = 256 * nwk + (n // 2 if sign < 0 else -(n // 2))   # the column the gap opens at
            head = _rand(rng, start - tl - 1)
            t, q = _gap_pair(rng, tl_main, n, sign, head)
            out.append(Gap(t, q, n, sign, f"wrap{nwk}", start))
    return out


def adjacent_pairs():
    """Two gaps of 14 ... 40 bases: of opposite signs with 1 ... 3 matching bases between them (the second opens at the penalty the first ended at), of the same sign
    with 17 ... 19 bases and one substitution between them (x = 4 penalties apart; closer, one gap of both lengths is cheaper).  Either way the second gap opens
    fewer than o2 penalties behind the first, a few diagonals on: the row it opens from is one that the first gap's extension also reaches."""
    out = []
    rng = np.random.default_rng(20253)
    for k, (n1, s1, n2, s2, between) in enumerate(((14, 1, 20, 1, 17), (20, -1, 14, -1, 19), (30, 1, 40, -1, 2), (40, -1, 30, 1, 1), (14, 1, 14, 1, 18), (36, -1, 40, 1, 3))):
        a, m, b = _rand(rng, 330 + k), _rand(rng, between), _rand(rng, 350 + 3 * k)
        x1, x2 = _rand(rng, n1), _rand(rng, n2)
        if s1 != s2:   # (opposite signs: no base of one gap matches a base of the other, or a few short gaps and substitutions between them are cheaper)
            x1, x2 = x1.translate(bytes.maketrans(b"GT", b"AC")), x2.translate(bytes.maketrans(b"AC", b"GT"))
        mq = bytearray(m)
        if between > 8:
            mq[between // 2] = tc._other(rng, m[between // 2])[0]
        t = a + (x1 if s1 < 0 else b"") + m + (x2 if s2 < 0 else b"") + b
        q = a + (x1 if s1 > 0 else b"") + bytes(mq) + (x2 if s2 > 0 else b"") + b
        out.append((t, q))
    return out


def gap_events(t: bytes, q: bytes, cigar, p: dict = DEFAULT):
    """[(sign, n, column where the gap opens, penalty before it, second piece?)] of the alignment's gaps, from the CIGAR words."""
    from miniwfa_amd.api import CIGAR_CHARS
    i = j = s = 0
    out = []
    for w in cigar or []:
        n, op = int(w) >> 4, CIGAR_CHARS[int(w) & 0xf]
        if op in "M=X":
            for _ in range(n):
                s += 0 if t[i] == q[j] else p["x"]
                i, j = i + 1, j + 1
        else:
            c1, c2 = p["o1"] + n * p["e1"], p["o2"] + n * p["e2"]
            out.append((1 if op == "I" else -1, n, j - i + len(t) + 1, s, c2 < c1))
            s += min(c1, c2)
            if op == "I":
                j += n
            else:
                i += n
    return out


# ---- shrinks ----------------------------------------------------------------------------------------------------------------------------
def shrink_candidates():
    rng = np.random.default_rng(20254)
    out = []
    for tl, ql in ((700, 760), (900, 640), (1500, 1480), (600, 2400), (2500, 700), (1200, 3000), (3000, 1100), (1900, 2100)):
        out.append((_rand(rng, tl), _rand(rng, ql)))
    out += [(t, q) for t, q in skewed_pairs(2025, 30, 600, 3000) if abs(len(t) - len(q)) > 300][:10]
    # short unrelated pairs: at penalty 256 / 512 the window's end has passed a chunk boundary on diagonals with fewer in-matrix cells than the offsets have come
    for tl, ql in ((300, 300), (310, 330), (560, 560), (570, 590)):
        out.append((_rand(rng, tl), _rand(rng, ql)))
    # length-skewed, related: the target is the head of the query (2 % substitutions).  Once the main diagonal has used up the target, every diagonal below it runs past
    # the target's end: the shrink at 256 takes the start from chunk 0 / 1 up to the main diagonal's, and every later one follows the insertion up
    for n, (tl, ql) in enumerate(((300, 2700), (330, 2400), (520, 2600))):
        a = _rand(rng, tl)
        qa = bytearray(a)
        for i in range(25, tl, 50):
            qa[i] = tc._other(rng, a[i])[0]
        out.append((a, bytes(qa) + _rand(rng, ql - tl)))
    return out


def shrink_crossings(lohi: np.ndarray, tl: int):
    """[(penalty, "start" | "end")]: shrinks (penalties 256, 512, ...) behind which the window's first chunk is higher / its last chunk lower than before."""
    out = []
    cols = ec.columns(lohi, tl)
    for s in range(256, len(cols), 256):   # cols[s - 1]: penalty s, cols[s]: penalty s + 1, the first window behind the shrink
        (lo0, hi0), (lo1, hi1) = cols[s - 1], cols[s]
        if lo1 >> 8 > lo0 >> 8:
            out.append((s, "start"))
        if hi1 >> 8 < hi0 >> 8:
            out.append((s, "end"))
    return out


# ---- fuzz -------------------------------------------------------------------------------------------------------------------------------
FUZZ_N = 64


def fuzz_pairs():
    """64 seeded pairs of 300 - 3000 bases: related at 2, 6, 12, 25 % with one or two long indels of up to 60 bases, unrelated, length-skewed."""
    rng = np.random.default_rng(20255)
    out = []
    for i in range(44):
        out.append(synth_pair(202500 + i, int(rng.integers(300, 3001)), (0.02, 0.06, 0.12, 0.25)[i % 4], 1 + i % 2, 60))
    for _ in range(10):   # (unrelated: up to 2.7 kb each, so that the window — target + query + 1 columns at most — stays within three chunk slots' 5824)
        out.append((_rand(rng, int(rng.integers(300, 2701))), _rand(rng, int(rng.integers(300, 2701)))))
    out += [(t, q) for t, q in skewed_pairs(20256, 40, 300, 2700) if abs(len(t) - len(q)) > 200][:10]
    assert len(out) == FUZZ_N
    return out


# ---- groups -----------------------------------------------------------------------------------------------------------------------------
GROUPS = ("gaps", "wrap", "adjacent", "shrinks", "climb", "fuzz")
_groups: dict = {}
_traces: dict = {}
_expected: dict = {}


def traces(orc, pairs, p: dict = DEFAULT):
    key = (id(pairs), tuple(sorted(p.items())))
    if key not in _traces:
        _traces[key] = bm._trace_all(orc, p, pairs)
    return _traces[key]


def fits_both(orc, pairs, p: dict = DEFAULT):
    """Per pair: finished by both geometries with the second fold's ageing period (width, chunk rule at AGE, forecast)."""
    out = []
    for (t, q), (lohi, far) in zip(pairs, traces(orc, pairs, p)):
        ok = True
        for g in (G3, G4):
            ok = ok and bm.widest(lohi) <= bm.admission_window(g) and bm.rule_chunks(g, AGE, lohi, len(t), len(q)) and bm.rule_forecast(g, far, len(t), len(q))
        out.append(ok)
    return out


def group(orc, name: str):
    """[(t, q)] of a group, built once; every pair is finished by 512 x 3 and 512 x 4 (the candidates that are not are dropped here, the CPU test counts what is left)."""
    if name not in _groups:
        if name == "gaps":
            pairs = [(g.t, g.q) for g in gap_pairs()]
        elif name == "wrap":
            pairs = [(g.t, g.q) for g in wrap_pairs()]
        elif name == "adjacent":
            pairs = adjacent_pairs()
        elif name == "shrinks":
            cand = shrink_candidates()
            for cname in ("cross-shrink-nwk24", "cross-shrink-nwk32"):
                cand += [p for p in ec.case(orc, cname).pairs if p not in cand]
            keep = fits_both(orc, cand)
            pairs = [p for p, k, (lohi, _) in zip(cand, keep, traces(orc, cand)) if k and shrink_crossings(lohi, len(p[0]))]
        elif name == "climb":
            pairs = []
            for nwk in (24, 32):
                pairs += [p for p in ec.case(orc, f"climb-nwk{nwk}-fold1").pairs if p not in pairs]
            pairs = [p for p, k in zip(pairs, fits_both(orc, pairs)) if k]
        elif name == "fuzz":
            pairs = fuzz_pairs()
        else:
            raise KeyError(name)
        _groups[name] = pairs
    return _groups[name]


def expected(orc, name: str, p: dict = DEFAULT, **kw):
    """[(s, n_iter, cigar)] from the oracle, with CIGAR, computed once."""
    key = (name, tuple(sorted(p.items())), tuple(sorted(kw.items())))
    if key not in _expected:
        _expected[key] = orc.align_many(pen_pairs() if name == "pens" else stop_pairs(orc) if name == "stops" else group(orc, name), make_opt(flag=1, **p, **kw), threads=bm.ORACLE_THREADS)[0]
    return _expected[key]


# ---- penalty sets -----------------------------------------------------------------------------------------------------------------------
GOLDEN = "band_fold2.jsonl"
# (seed, tl, p, n_long, long_max) of the fixture's pairs: synth_pair specs, run through the compiled reference under every set of PENS (tests/golden/make_golden_band_fold2.py)
GOLDEN_SPECS = [(20257000 + i, (900, 1700, 2600)[i % 3], (0.03, 0.06)[i % 2], 2, (40, 80)[i % 2]) for i in range(4)]


def pen_pairs():
    """The fixture's pairs, gaps of every length of GAP_LENGTHS, and a few unrelated ones (shrinks under every set)."""
    if "pens" not in _groups:
        rng = np.random.default_rng(20258)
        _groups["pens"] = [synth_pair(*s) for s in GOLDEN_SPECS] + [(g.t, g.q) for g in gap_pairs() if g.kind in ("quad1", "edge")] + \
                          [(_rand(rng, 800), _rand(rng, 900)), (_rand(rng, 1500), _rand(rng, 700))]
    return _groups["pens"]


# ---- stops and end cells ----------------------------------------------------------------------------------------------------------------
def stop_pairs(orc):
    """Three pairs of the shrink group and two of the gaps: stopped by max_s in the middle of their run and by max_iter."""
    if "stops" not in _groups:
        _groups["stops"] = group(orc, "shrinks")[:3] + group(orc, "gaps")[:2]
    return _groups["stops"]


def stop_opts(orc):
    """{"max_s": ...} and {"max_iter": ...} that stop every pair of stop_pairs somewhere inside its run: half the smallest s, a third of the smallest n_iter."""
    full = orc.align_many(stop_pairs(orc), make_opt(flag=0, **DEFAULT), threads=bm.ORACLE_THREADS)[0]
    return dict(max_s=min(e[0] for e in full) // 2), dict(max_iter=min(e[1] for e in full) // 3)


def end_chunk_age(lohi: np.ndarray, tl: int, ql: int) -> int:
    """Penalties for which the chunk of the end cell's column (ql + 1) has met the window without a break when the pair ends."""
    g, n = (ql + 1) >> 8, 0
    for _, ga, gb in reversed(list(ec.keys(lohi, tl))):
        if not ga <= g <= gb:
            break
        n += 1
    return n


def tab2_kernel_notes():
    """{demangled kernel name: {field: int}} of mwf_band2_tab2.hip.o's kernels (band_matrix.device_kernels), and the names of every other kernel in it."""
    got = bm.device_kernels(TAB2_OBJ, "wfa_band2_tab2_kernel")
    assert not isinstance(got, str), got
    return got
