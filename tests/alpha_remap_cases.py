"""Inputs shared by tests/test_alpha_remap_cpu.py and tests/test_alpha_remap_gpu.py: the alphabet cases of the "alpha_remap" tunable, the rule
restated in Python, and the batches the GPU tests align.  Nothing here needs a device."""
import numpy as np

from miniwfa_amd.synth import synth_pair, spec_pair

LENGTHS = (1, 15, 16, 17, 63, 64, 65, 449, 450, 900, 3000, 6500)
# bytes -> bytes recodings of a plain pair (case name -> what happens to target and query)
_T_U = bytes.maketrans(b"T", b"U")
_TWO = bytes.maketrans(b"ACGT", bytes([0, 0, 1, 1]))
_FOUR = bytes.maketrans(b"ACGT", bytes([0x00, 0x7f, 0x80, 0xff]))
_CODE03 = bytes.maketrans(b"ACGT", bytes([0, 1, 2, 3]))
CASES = ("plain", "lower", "acgu", "one", "two", "four_bytes", "five", "fifth_last_q", "fifth_in_t")


def py_class(t: bytes, q: bytes):
    """The rule, restated: (class, 256-byte map).  Class 0 every byte is one of A C G T, 1 at most four distinct bytes and not class 0, 2 five or
    more; for class 1 the distinct bytes in ascending byte value map to "ACGT"[rank], every other entry (and every entry of classes 0 and 2) is 0."""
    syms = sorted(set(t) | set(q))
    m = bytearray(256)
    if all(b in b"ACGT" for b in syms):
        return 0, bytes(m)
    if len(syms) > 4:
        return 2, bytes(m)
    for rank, b in enumerate(syms):
        m[b] = b"ACGT"[rank]
    return 1, bytes(m)


def base_pair(seed: int, length: int, p: float = 0.05):
    """A plain pair of about `length` bases whose first bases spell ACGT in both sequences (so that a case has the symbols its name says)."""
    t, q = synth_pair(seed, length, p)
    k = min(4, len(t), len(q))
    return b"ACGT"[:k] + t[k:], b"ACGT"[:k] + q[k:]


def recode(case: str, t: bytes, q: bytes):
    if case == "plain":
        return t, q
    if case == "lower":
        return t.lower(), q.lower()
    if case == "acgu":
        return t.translate(_T_U), q.translate(_T_U)
    if case == "one":
        return b"x" * len(t), b"x" * len(q)
    if case == "two":
        return t.translate(_TWO), q.translate(_TWO)
    if case == "four_bytes":
        return t.translate(_FOUR), q.translate(_FOUR)
    if case == "five":
        return t[:len(t) // 2] + b"N" + t[len(t) // 2 + 1:], q[:len(q) // 3] + b"N" + q[len(q) // 3 + 1:]
    if case == "fifth_last_q":
        return t, q[:-1] + b"N"
    if case == "fifth_in_t":
        return t[:len(t) // 2] + b"N" + t[len(t) // 2 + 1:], q
    raise KeyError(case)


def cpu_inputs():
    """[(name, t, q)]: every case at a short and a mid length, then the empty ones."""
    out = []
    for k, case in enumerate(CASES):
        for length in (17, 450):
            t, q = base_pair(7300 + 10 * k + (length == 450), length)
            out.append((f"{case}-{length}", *recode(case, t, q)))
    out.append(("both_empty", b"", b""))
    out.append(("empty_t", b"", b"acgtacgt"))
    out.append(("empty_q", b"ACGU", b""))
    return out


def gpu_pairs():
    """The pairs of GPU test (a) without the shared-target ones, 39: every case four times and every length of LENGTHS three times (pair k: case k mod 9,
    length k mod 12), then the empty ones.  Packed back to back, so most sequences start at odd byte offsets."""
    pairs, names = [], []
    for k in range(36):
        case, length = CASES[k % 9], LENGTHS[k % 12]
        t, q = base_pair(8100 + k, length)
        pairs.append(recode(case, t, q)), names.append(f"{case}-{length}")
    pairs += [(b"", b""), (b"", b"acgtacgt"), (b"ACGU", b"")]
    names += ["both_empty", "empty_t", "empty_q"]
    return pairs, names


class Packed:
    """What miniwfa_amd.synth.PackedBatch is to Engine.upload / wrap_packed, with free offsets: `extra` appends pairs (t_index, q) whose target is
    the byte range of pair t_index's target."""

    def __init__(self, pairs, extra=()):
        from miniwfa_amd.synth import PackedBatch
        pk = PackedBatch(list(pairs) + [(b"", q) for _, q in extra])
        self.n, self.total, self.seqs, self.q_off, self.ql = pk.n, pk.total, pk.seqs, pk.q_off, pk.ql
        self.t_off, self.tl = pk.t_off.copy(), pk.tl.copy()
        for j, (ti, _) in enumerate(extra):
            self.t_off[len(pairs) + j], self.tl[len(pairs) + j] = pk.t_off[ti], pk.tl[ti]

    def pair(self, i):
        s = self.seqs.tobytes()
        return s[self.t_off[i]:self.t_off[i] + self.tl[i]], s[self.q_off[i]:self.q_off[i] + self.ql[i]]


def gpu_batch_a():
    """(Packed, names): gpu_pairs() plus three queries — lower case as their target, an N in one, upper case in one — on the target of the
    lower-case 3000-base pair."""
    pairs, names = gpu_pairs()
    ti = names.index("lower-3000")
    t = pairs[ti][0]
    q1 = spec_pair({"kind": "fit", "seed": 8201, "tl": len(t), "ql": len(t) - 7, "p": 0.05})[1]
    extra = [(ti, pairs[ti][1][::-1]), (ti, pairs[ti][1][:400] + b"N" + pairs[ti][1][401:]), (ti, q1)]
    return Packed(pairs, extra), names + ["shared-rev", "shared-n", "shared-upper"]


def gpu_batch_short():
    """(Packed, names): the pairs of gpu_batch_a() of at most 900 bases (target + query <= 2048: the launches of mwf_alphabet.hip take their 64-thread
    form), the empty ones and a fifth symbol in the last byte of a query among them, plus two queries on one shared lower-case target."""
    pairs, names = gpu_pairs()
    keep = [i for i, (t, q) in enumerate(pairs) if len(t) + len(q) <= 2048]
    pairs, names = [pairs[i] for i in keep], [names[i] for i in keep]
    assert max(len(t) + len(q) for t, q in pairs) > 1024 and any(n.startswith("fifth_last_q-") for n in names)
    ti = names.index("lower-449")
    extra = [(ti, pairs[ti][1][:100] + b"N" + pairs[ti][1][101:]), (ti, pairs[ti][1][5:])]
    return Packed(pairs, extra), names + ["shared-n", "shared-cut"]


def gpu_batch_long():
    """(Packed, names): three pairs of 34 kb at 1 % (target + query > 65 536: the 1024-thread form) — lower case, plain with a fifth symbol in the last
    byte of the query, bases coded 0..3 — packed back to back, so the later ones start at whatever offset the lengths before them leave."""
    base = [synth_pair(8300 + i, 34000 + i, 0.01) for i in range(3)]
    pairs = [(base[0][0].lower(), base[0][1].lower()), (base[1][0], base[1][1][:-1] + b"N"), (base[2][0].translate(_CODE03), base[2][1].translate(_CODE03))]
    assert all(len(t) + len(q) > 65536 for t, q in pairs)
    return Packed(pairs), ["lower-34k", "fifth_last_q-34k", "code03-34k"]


def routing_pairs(n: int, length: int, p: float, seed: int):
    """n plain pairs of `length` bases at divergence p (upper case: the twin); .lower() of both gives the batch under test."""
    return [synth_pair(seed + i, length, p) for i in range(n)]


def lower(pairs):
    return [(t.lower(), q.lower()) for t, q in pairs]


def other_same_lengths(pairs, seed: int, coding: bytes = _CODE03):
    """Other sequences of the same lengths as `pairs`, in another four-letter coding (default: bases as bytes 0..3)."""
    out = []
    for i, (t, q) in enumerate(pairs):
        t2, q2 = spec_pair({"kind": "fit", "seed": seed + i, "tl": len(t), "ql": len(q), "p": 0.05})
        assert (len(t2), len(q2)) == (len(t), len(q))
        out.append((t2.translate(coding), q2.translate(coding)))
    return out


def seq_buffer(pk, pairs) -> np.ndarray:
    """The bytes of `pairs` laid out as pk (a PackedBatch of pairs of the same lengths) holds its own: what overwrites a wrapped batch's sequence tensor."""
    buf = np.zeros(len(pk.seqs), dtype=np.uint8)
    for i, (t, q) in enumerate(pairs):
        assert (len(t), len(q)) == (int(pk.tl[i]), int(pk.ql[i]))
        buf[pk.t_off[i]:pk.t_off[i] + len(t)] = np.frombuffer(t, dtype=np.uint8)
        buf[pk.q_off[i]:pk.q_off[i] + len(q)] = np.frombuffer(q, dtype=np.uint8)
    return buf
