"""Inputs shared by tests/test_alpha16_cpu.py and tests/test_alpha16_gpu.py: the alphabet cases of the "alpha16" tunable (include/miniwfa.h), the rule restated in
Python, the batches the GPU tests align and the edge cases of the 4-bit band kernels (miniwfa_amd/csrc/mwf_band2_nib.hip: eight bases per dword, FULL = 8, four per-lane
trips of eight bases, whole-wave trips of 512).  Nothing here needs a device; expected answers always come from the oracle on the ORIGINAL bytes."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import synth_pair, spec_pair
from alpha_remap_cases import Packed, seq_buffer  # noqa: F401  (the same free-offset packing and in-place overwrite)
import band_matrix as bm

TAG = 0x40
DEFAULT = bm.PEN["default"]
FULL, LANE_TRIPS = 8, 4
WAVE_WALK_FROM = FULL + 8 * LANE_TRIPS   # 40: a run longer than this is finished by the whole wave, 512 bases per trip
SYM16 = b"ACGTNRYKMSWBDHVU"              # A C G T, N, and IUPAC codes: sixteen distinct bytes
SYM17 = SYM16 + b"-"
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 449, 450, 900, 3000, 6500)
CASES = ("plain", "lower", "acgtn", "mixed8", "sym16", "sym17", "n_last_q", "bytes_00_ff")
# the three geometries of the 4-bit form, as the tests force them: 512 x 3 and 512 x 4 by block (the 512 x 4 entry of band_matrix.GEOMS is its default-routing one)
G3 = bm.GEOMS[(512, 3, 0)]
G4 = bm.Geom(512, 4, 1, 0, "block", 0, 0, 0)
GSPAN = bm.GEOMS[(1024, 5, 0)]
GEOMS = {"512x3": G3, "512x4": G4, "span": GSPAN}


def tunables(geom: str, band_fold: int):
    """How the engine is brought to launch the 4-bit form of `geom` for every pair of an all-class-3 batch."""
    if geom == "span":
        return bm.COMMON_DEFAULT_ROUTING + (("band_span", 2), ("band_fold", band_fold))
    return (("force_kind", 2), ("block", 512), ("band_pack", 1), ("wide_slots", 3 if geom == "512x3" else 4), ("band_fold", band_fold))


def py_class16(t: bytes, q: bytes):
    """The rule, restated: (class, 256-byte map).  0 every byte is one of A C G T; 1 at most four distinct bytes and not class 0 — they map to "ACGT"[rank]; 3 five to
    sixteen — they map to 0x40 | rank, rank by ascending byte value; 2 seventeen or more.  Entries of bytes that do not occur, and every entry of classes 0 and 2: 0."""
    syms = sorted(set(t) | set(q))
    m = bytearray(256)
    if all(b in b"ACGT" for b in syms):
        return 0, bytes(m)
    if len(syms) > 16:
        return 2, bytes(m)
    for rank, b in enumerate(syms):
        m[b] = b"ACGT"[rank] if len(syms) <= 4 else TAG | rank
    return (1 if len(syms) <= 4 else 3), bytes(m)


def sprinkle(seq: bytes, symbols: bytes, seed: int, head: bool = True) -> bytes:
    """`seq` with every byte of `symbols` written once near its start (head) and then at ~1 % of its positions: the alphabet a case is named for, whatever the length allows."""
    s = bytearray(seq)
    rng = np.random.default_rng(seed)
    if head:
        for k, b in enumerate(symbols[:len(s)]):
            s[k] = b
    for p in np.nonzero(rng.random(len(s)) < 0.01)[0]:
        if p >= len(symbols) or not head:
            s[p] = symbols[int(rng.integers(0, len(symbols)))]
    return bytes(s)


def soft_mask(seq: bytes, seed: int) -> bytes:
    """Lower-case stretches of 20-200 bases over about a third of the sequence (soft-masked repeats)."""
    s = bytearray(seq)
    rng = np.random.default_rng(seed)
    at = 0
    while at < len(s):
        at += int(rng.integers(20, 400))
        n = int(rng.integers(20, 200))
        s[at:at + n] = bytes(s[at:at + n]).lower()
        at += n
    return bytes(s)


def recode(case: str, t: bytes, q: bytes, seed: int = 0):
    if case == "plain":
        return t, q
    if case == "lower":
        return t.lower(), q.lower()
    if case == "acgtn":
        return sprinkle(t, b"ACGTN", seed), sprinkle(q, b"N", seed + 1, head=False)
    if case == "mixed8":
        return sprinkle(soft_mask(t, seed), b"ACGTacgt", seed), soft_mask(q, seed + 1)
    if case == "sym16":
        return sprinkle(t, SYM16, seed), sprinkle(q, SYM16, seed + 1, head=False)
    if case == "sym17":
        return sprinkle(t, SYM17, seed), sprinkle(q, SYM17, seed + 1, head=False)
    if case == "n_last_q":   # the fifth symbol occurs only in the last byte of the query
        return t, q[:-1] + b"N"
    if case == "bytes_00_ff":   # bytes 0x00 and 0xff among six symbols: the lowest and the highest code a byte can have
        tr = bytes.maketrans(b"AT", b"\x00\xff")
        return sprinkle(t, b"ACGTNR", seed).translate(tr), sprinkle(q, b"NR", seed + 1, head=False).translate(tr)
    raise KeyError(case)


def base_pair(seed: int, length: int, p: float = 0.05):
    t, q = synth_pair(seed, length, p)
    k = min(4, len(t), len(q))
    return b"ACGT"[:k] + t[k:], b"ACGT"[:k] + q[k:]


def cpu_inputs():
    """[(name, t, q)]: every case at a short and a mid length; then exactly 4, 5, 16 and 17 distinct bytes; the empty ones."""
    out = []
    for k, case in enumerate(CASES):
        for length in (40, 450):
            t, q = base_pair(9300 + 10 * k + (length == 450), length)
            out.append((f"{case}-{length}", *recode(case, t, q, 9400 + k)))
    out.append(("exactly4", b"acgtacgt", b"tgca"))
    out.append(("exactly5", b"acgtacgt", b"tgcan"))
    out.append(("exactly16", bytes(range(100, 116)), bytes(range(108, 116))))
    out.append(("exactly17", bytes(range(100, 116)), bytes(range(108, 117))))
    out.append(("split16", bytes(range(0, 8)), bytes(range(248, 256))))
    out.append(("both_empty", b"", b""))
    out.append(("empty_t", b"", b"ACGTN"))
    out.append(("empty_q", b"ACGTNRYK", b""))
    return out


def gpu_pairs():
    """39 pairs: pair k has case k mod 8 and length LENGTHS[k mod 12] (every case at four or five lengths, every length three times), then the empty ones.  Packed back to
    back: most sequences start at odd byte offsets."""
    pairs, names = [], []
    for k in range(36):
        case, length = CASES[k % 8], LENGTHS[k % 12]
        t, q = base_pair(9100 + k, length)
        pairs.append(recode(case, t, q, 9200 + k)), names.append(f"{case}-{length}")
    pairs += [(b"", b""), (b"", b"ACGTN"), (b"ACGTNRYK", b"")]
    names += ["both_empty", "empty_t", "empty_q"]
    return pairs, names


def gpu_batch_a():
    """(Packed, names): gpu_pairs() plus three queries on the target range of the ACGT+N 3000-base pair — reversed (unrelated), with IUPAC codes, plain."""
    pairs, names = gpu_pairs()
    ti = names.index("acgtn-3000")
    t, q = pairs[ti]
    q1 = spec_pair({"kind": "fit", "seed": 9201, "tl": len(t), "ql": len(t) - 7, "p": 0.05})[1]
    extra = [(ti, q[::-1]), (ti, sprinkle(q, b"RYKM", 9202, head=False)), (ti, q1)]
    return Packed(pairs, extra), names + ["shared-rev", "shared-iupac", "shared-plain"]


def gpu_batch_short():
    """(Packed, names): the pairs of gpu_pairs() with target + query <= 2048 (the 64-thread form of the classify and copy kernels), two queries on a shared target."""
    pairs, names = gpu_pairs()
    keep = [i for i, (t, q) in enumerate(pairs) if len(t) + len(q) <= 2048]
    pairs, names = [pairs[i] for i in keep], [names[i] for i in keep]
    assert max(len(t) + len(q) for t, q in pairs) > 1024 and any(n.startswith("n_last_q-") for n in names)
    ti = names.index("acgtn-900") if "acgtn-900" in names else next(i for i, n in enumerate(names) if n.startswith("acgtn-"))
    extra = [(ti, pairs[ti][1][:100] + b"R" + pairs[ti][1][101:]), (ti, pairs[ti][1][5:])]
    return Packed(pairs, extra), names + ["shared-r", "shared-cut"]


def gpu_batch_long():
    """(Packed, names): three pairs of 34 kb at 1 % (target + query > 65 536: the 1024-thread form) — ACGT+N (class 3), seventeen symbols (class 2), plain with an N in
    the last byte of the query (class 3) — packed back to back."""
    base = [synth_pair(9300 + i, 34000 + i, 0.01) for i in range(3)]
    pairs = [recode("acgtn", *base[0], 9310), recode("sym17", *base[1], 9311), recode("n_last_q", *base[2])]
    assert all(len(t) + len(q) > 65536 for t, q in pairs)
    return Packed(pairs), ["acgtn-34k", "sym17-34k", "n_last_q-34k"]


def with_n(pairs, seed: int):
    """Every pair with one run of ten N in the target and three single N in the query (the shape of the measurements, profiles/alpha16_time.py)."""
    out = []
    for i, (t, q) in enumerate(pairs):
        rng = np.random.default_rng(seed + i)
        a = int(rng.integers(0, max(1, len(t) - 10)))
        t2 = t[:a] + b"N" * min(10, len(t) - a) + t[a + 10:]
        q2 = bytearray(q)
        for p in rng.integers(0, len(q), 3):
            q2[int(p)] = ord("N")
        out.append((t2[:len(t)], bytes(q2)))
    return out


def routing_pairs(n: int, length: int, p: float, seed: int):
    """n pairs of `length` bases at divergence p with N in every pair (class 3)."""
    return with_n([synth_pair(seed + i, length, p) for i in range(n)], seed + 5000)


# ---- (d) edge cases of the 4-bit probe and walks ---------------------------------------------------------------------------------------------------------
# a run the case is about: it starts at target position ti / query position qi behind a substitution, is exactly n bases long, and ends with `end`: "room" (a
# mismatch behind it), or exactly at the end of the "target", the "query", or "both"
Run = namedtuple("Run", "ti qi n end")
RUNS_SHORT = (0, 1, 7, 8, 9, 15, 16, 17, 39, 40, 41)   # around FULL, two FULL, and the end of the four per-lane trips
RUNS_LONG = (511, 512, 513, 1030)                      # whole-wave trips: one, one and a base, two and a bit
RUNS_END = (1, 7, 8, 9, 17, 40, 41, 513)
ENDS = ("target", "query", "both")
ALPHA5 = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _rand(rng, n: int, alpha=ALPHA5) -> bytes:
    return alpha[rng.integers(0, len(alpha), n)].tobytes()


def _other(rng, b: int, alpha=ALPHA5) -> bytes:
    k = int(np.nonzero(alpha == b)[0][0])
    return bytes([alpha[(k + int(rng.integers(1, len(alpha)))) % len(alpha)]])


def _sub_run(rng, t: bytearray, q: bytearray, n: int, alpha=ALPHA5):
    """Append a substitution and an exact run of n bases: returns the run's start (the caller appends what ends it)."""
    a = _rand(rng, 1, alpha)
    t += a
    q += _other(rng, a[0], alpha)
    r = _rand(rng, n, alpha)
    ti, qi = len(t), len(q)
    t += r
    q += r
    return ti, qi


def lce(t: bytes, q: bytes, i: int, j: int) -> int:
    n = 0
    while i + n < len(t) and j + n < len(q) and t[i + n] == q[j + n]:
        n += 1
    return n


def _head(rng, n: int) -> bytes:
    """n random bases of A C G T N that begin with all five (every edge pair is class 3 whatever the rest draws)."""
    return b"ACGTN" + _rand(rng, n - 5)


def edge_pairs():
    """[(name, t, q, [Run])] — every pair is class 3 (A C G T N drawn uniformly unless the name says otherwise)."""
    rng = np.random.default_rng(4016)
    out = []
    for lead in (301, 302, 303, 304):   # (column tl + 1 of the main diagonal: every position of a lane's quad)
        t = bytearray(_head(rng, lead))
        q, runs = bytearray(t), []
        for n in RUNS_SHORT:
            ti, qi = _sub_run(rng, t, q, n)
            runs.append(Run(ti, qi, n, "room"))
        _sub_run(rng, t, q, 150)
        out.append((f"runs-short-{lead}", bytes(t), bytes(q), runs))
    t = bytearray(_head(rng, 300))
    q, runs = bytearray(t), []
    for n in RUNS_LONG:
        ti, qi = _sub_run(rng, t, q, n)
        runs.append(Run(ti, qi, n, "room"))
    _sub_run(rng, t, q, 60)
    out.append(("runs-long", bytes(t), bytes(q), runs))
    k = 0
    for n in RUNS_END:
        for end in ENDS:
            t = bytearray(_head(rng, 300 + k % 4))
            q = bytearray(t)
            k += 1
            _sub_run(rng, t, q, 40)
            ti, qi = _sub_run(rng, t, q, n)
            if end == "target":
                q += _other(rng, t[ti] if n else ALPHA5[0]) + _rand(rng, 4)   # the query runs on: five more bases
            elif end == "query":
                t += _other(rng, q[qi] if n else ALPHA5[0]) + _rand(rng, 4)
            out.append((f"end-{end}-{n}", bytes(t), bytes(q), [Run(ti, qi, n, end)]))
    # sequence lengths with len % 8 in {0, 1, 7}, every combination of target and query
    for rt in (0, 1, 7):
        for rq in (0, 1, 7):
            t0, q0 = recode("acgtn", *synth_pair(4100 + 8 * rt + rq, 640, 0.06), 4200 + 8 * rt + rq)
            t1, q1 = t0[:600 + rt], q0[:608 + rq]
            out.append((f"len8-{rt}-{rq}", t1, q1, []))
    # sixteen symbols, nearly every base the one of code 0 or the one of code 15: neighbouring nibbles 0x0 and 0xf throughout
    s16 = np.frombuffer(bytes(sorted(SYM16)), dtype=np.uint8)
    ends = np.array([s16[0], s16[15]], dtype=np.uint8)
    t = bytearray(bytes(s16) + _rand(rng, 900, ends))
    q = bytearray(t)
    for n in (3, 8, 21, 64):
        _sub_run(rng, t, q, n, ends)
    for p in range(40, 900, 97):
        q[p] = int(s16[1 + (p % 14)])
    out.append(("codes-0-15", bytes(t), bytes(q) + _rand(rng, 3, ends), []))
    # the penalty-0 extension over a whole identical pair (2001 bases: four whole-wave trips less a few bases, len % 8 == 1)
    ident = _head(rng, 2001)
    out.append(("identical", ident, ident, [Run(0, 0, 2001, "both")]))
    # a CIGAR whose back-match crosses dword boundaries of the copy: '=' runs of 100-300 bases from odd positions, an insertion and a deletion between them
    t = bytearray(_head(rng, 133))
    q = bytearray(t)
    for n in (101, 203, 299):
        _sub_run(rng, t, q, n)
        t += _rand(rng, 3)   # a three-base deletion from the query ...
        r = _rand(rng, 77)
        t += r
        q += r
        q += _rand(rng, 5)   # ... and a five-base insertion
        r = _rand(rng, 91)
        t += r
        q += r
    out.append(("backmatch", bytes(t), bytes(q), []))
    return out


_edge = None


def edge():
    global _edge
    if _edge is None:
        _edge = edge_pairs()
    return _edge


_expected: dict = {}


def expected(orc, key: str, pairs, flag: int = 1, **pen):
    """[(s, n_iter, cigar)] from the oracle on the original bytes, computed once per (key, penalties) and left alone (s and n_iter of a score-only run are the same)."""
    from oracle.pyoracle import make_opt
    p = dict(DEFAULT)
    p.update(pen)
    k = (key, flag, tuple(sorted(p.items())))
    if k not in _expected:
        _expected[k] = orc.align_many(list(pairs), make_opt(flag=flag, **p), threads=bm.ORACLE_THREADS)[0]
    return _expected[k]


NIB_OBJ = os.path.join(bm.ROOT, "miniwfa_amd", "csrc", "build", "mwf_band2_nib.hip.o")


def nib_object_kernels():
    """The wfa_band2_nib_kernel<...> instantiations in mwf_band2_nib.hip.o's gfx950 code object (band_matrix.Inst), and every other kernel of that object."""
    got = bm.device_kernels(NIB_OBJ, "wfa_band2_nib_kernel")
    assert not isinstance(got, str), got
    return set(got[0]), {re.search(r"(\w+)<", name).group(1) for name in got[1]}
