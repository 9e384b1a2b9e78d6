"""The device-side alignment text (csrc/mwf_cigar_text.hip) through Batch.text(), Batch.texts(), Batch.text_fetch() and Batch.dev_text().  Bar: byte
equality of all six kinds (CIGAR, SAM M-form, cs, MD, the two gapped rows), per pair, with the host twin (mwf_cigar_text) and with an independent
Python restatement of the rules (tests/cigar_text_ref.py), on the words the align produced; the offsets must be the prefix sums of the lengths.
Shapes: those tests/test_cigar_ops_gpu.py runs — one-wave, 256- and 1024-thread workgroups, one and many passes over the words (the 64-bit carries
of the positions, of SAM's open M run and of MD's open count), single words of thousands of bases (the per-byte spread), every decimal width from
1 to 5 digits at its boundary, empty sequences, stopped pairs, unrenderable foreign CIGARs.

long_pairs() is taken from tests/test_cigar_ops_gpu.py unchanged: under the default penalties its fixed seeds give, at multiples of 256 words, both
an = / X run and an MD count that span the pass boundary (asserted below on the actual words), so no other seed was needed."""
import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import synth_pair, fuzz_pairs, skewed_pairs, random_seq, PackedBatch
from conftest import load_golden, golden_inputs
from cigar_ops_ref import OP_I, OP_D, OP_EQ, OP_X, malformed_variants
from cigar_text_ref import KINDS, py_texts, digit_pair
from test_cigar_ops_gpu import PEN_SETS, PEN_KEYS, cigar_opt, own_words, long_pairs, _to_device

pytestmark = pytest.mark.gpu

EMPTY = [b""] * len(KINDS)


@pytest.fixture(scope="module")
def engine():
    e = mw.Engine(0)
    yield e
    e.close()


def expected(pairs, words, s):
    """[pair][kind]: the restatement's text of the pair's words (empty for a stopped pair), which the host twin must give too."""
    out = []
    for i, (t, q) in enumerate(pairs):
        if s[i] < 0:
            out.append(EMPTY)
            continue
        ref = py_texts(words[i], t, q)
        assert ref is not None, i
        assert [mw.cigar_text(kind, t, q, words[i]) for kind in KINDS] == ref, i
        out.append(ref)
    return out


def check_texts(b, want, cigars=None, kinds=KINDS):
    for kind in kinds:
        b.text(kind, cigars)
        raw, off = b.text_fetch(kind)
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(w[kind]) for w in want], dtype=np.int64)]).tolist(), kind
        assert len(raw) == off[-1]
        for i, w in enumerate(want):
            assert raw[off[i]:off[i + 1]] == w[kind], (kind, i)
        ptr, off_ptr, total = b.dev_text(kind)
        assert ptr and off_ptr and total == off[-1]


def aligned(engine, pairs, opt):
    b = engine.upload(PackedBatch(pairs))
    b.align(opt)
    s, it, nc = b.results()
    return b, s, nc, own_words(b, nc)


@pytest.mark.parametrize("pen", PEN_SETS)
def test_mixed_batch(engine, pen):
    """160 pairs, two of them empty on both sides (MD "0"), up to 549 words: the 256-thread geometry, one to three passes."""
    pairs = fuzz_pairs(5, 120, 1500) + skewed_pairs(9, 40, 200, 1200)
    empty = [i for i, (t, q) in enumerate(pairs) if not t and not q]
    assert len(pairs) == 160 and len(empty) == 2
    b, s, nc, words = aligned(engine, pairs, cigar_opt(pen))
    assert (s >= 0).all() and int(nc.max()) > 512
    want = expected(pairs, words, s)
    for i in empty:
        assert want[i] == [b"", b"", b"", b"0", b"", b""]
    check_texts(b, want)
    assert b.texts(mw.MWF_TXT_MD) == [w[mw.MWF_TXT_MD] for w in want]
    b.free()


def spans_of(words, every):
    """Pass boundaries p (multiples of `every`) that (an = / X run, an MD count) spans: words p - 1 and p both = or X; a count that is open in front
    of word p (bases under = since the last X / D) AND grows behind it before the next X / D or the end."""
    ops, lens = [int(w) & 15 for w in words], [int(w) >> 4 for w in words]
    run, md = [], []
    for p in range(every, len(words), every):
        if ops[p - 1] in (OP_EQ, OP_X) and ops[p] in (OP_EQ, OP_X):
            run.append(p)
        c_front, k = 0, p - 1
        while k >= 0 and ops[k] not in (OP_X, OP_D):
            c_front += lens[k] if ops[k] == OP_EQ else 0
            k -= 1
        c_behind, k = 0, p
        while k < len(words) and ops[k] not in (OP_X, OP_D):
            c_behind += lens[k] if ops[k] == OP_EQ else 0
            k += 1
        if c_front > 0 and c_behind > 0:
            md.append(p)
    return run, md


def test_many_passes_and_degenerate_words(engine):
    """1840 and 3729 words (8 and 15 passes of 256), `5000=`, `300I`, `300D`; a run and an MD count across a pass boundary come out as one number."""
    pairs = long_pairs()
    b, s, nc, words = aligned(engine, pairs, cigar_opt(PEN_SETS[0]))
    assert nc.tolist() == [1840, 3729, 1, 281, 1, 1]
    assert words[2].tolist() == [5000 << 4 | 7] and words[4].tolist() == [300 << 4 | 1] and words[5].tolist() == [300 << 4 | 2]
    # a condition on the inputs: the carries of the SAM run and of the MD count are exercised
    run, md = [], []
    for i in (0, 1):
        r, m = spans_of(words[i], 256)
        run += r
        md += m
    print("pass boundaries spanned by an =/X run:", run, "by an MD count:", md)
    assert run and md
    want = expected(pairs, words, s)
    assert want[2] == [b"5000=", b"5000M", b":5000", b"5000", pairs[2][0], pairs[2][1]]
    assert want[4] == [b"300I", b"300I", b"+" + pairs[4][1].lower(), b"0", b"-" * 300, pairs[4][1]]
    assert want[5] == [b"300D", b"300D", b"-" + pairs[5][0].lower(), b"0^" + pairs[5][0] + b"0", pairs[5][0], b"-" * 300]
    check_texts(b, want)
    b.free()


def test_one_wave_per_pair(engine):
    """No pair above 2048 bases of target + query: 64 threads per pair; the pair of ~2 kb at 15 % has more than 64 words — several passes of one wave."""
    pairs = [synth_pair(40 + i, 100 + 25 * i, 0.05) for i in range(10)] + [synth_pair(61, 990, 0.15), (b"", b""), (b"ACGT", b"")]
    assert max(len(t) + len(q) for t, q in pairs) <= 2048 and len(pairs[10][0]) + len(pairs[10][1]) > 1900
    b, s, nc, words = aligned(engine, pairs, cigar_opt(PEN_SETS[0]))
    assert (s >= 0).all() and int(nc[10]) > 128
    run, md = spans_of(words[10], 64)
    print("one wave: pass boundaries spanned by an =/X run:", run, "by an MD count:", md)
    assert run and md
    check_texts(b, expected(pairs, words, s))
    b.free()


def test_one_long_pair_beside_reads(engine):
    """The 150 kb golden pair and a few reads: every pair runs at 1024 threads."""
    v = next(v for v in load_golden("long_pairs.jsonl") if v["id"] == "c4-cigar")
    t, q = golden_inputs(v)
    assert len(t) + len(q) > 65536
    pen = tuple(v["opt"][k] for k in PEN_KEYS)
    pairs = [synth_pair(70, 150, 0.05), (t, q), synth_pair(71, 151, 0.1), (b"", b"")]
    b, s, nc, words = aligned(engine, pairs, cigar_opt(pen))
    assert (s >= 0).all() and int(nc[1]) == v["expect"]["n_cigar"] > 1024
    check_texts(b, expected(pairs, words, s))
    b.free()


def test_digit_boundaries(engine):
    """'=' runs of exactly 9, 10, 99, 100, 999 and 1000 bases (the widths of every number change from word to word) and `10000=`."""
    t, q, dwords = digit_pair()
    ident = random_seq(79, 10000)
    pairs = [(t, q), (ident, ident)]
    b, s, nc, words = aligned(engine, pairs, cigar_opt(PEN_SETS[0]))
    assert words[0].tolist() == dwords and words[1].tolist() == [10000 << 4 | 7]
    want = expected(pairs, words, s)
    assert want[0][0] == b"9=1X10=1X99=1X100=1X999=1X1000=" and want[0][1] == b"2222M" and want[0][3] == b"9A10N99\x80100t999G1000"
    assert want[1] == [b"10000=", b"10000M", b":10000", b"10000", ident, ident]
    check_texts(b, want)
    b.free()


def test_stopped_pairs(engine):
    """max_s = 100: the diverged pairs stop; every kind has empty text for them (MD too), the offsets do not move, the identical pair stays rendered."""
    pairs = long_pairs()
    b, s, nc, words = aligned(engine, pairs, cigar_opt(PEN_SETS[0], max_s=100))
    assert s[3] == -1 and s[0] == -1 and s[2] == 0
    want = expected(pairs, words, s)
    assert want[3] == EMPTY and want[2][0] == b"5000="
    check_texts(b, want)
    b.free()


def test_foreign_cigars(engine):
    import torch
    dev = torch.device("cuda:0")
    pairs = [synth_pair(110 + i, 300 + 60 * i, 0.06) for i in range(6)]   # (seeds whose CIGARs end in an "=": malformed_variants needs that)
    b, s, nc, words = aligned(engine, pairs, cigar_opt(PEN_SETS[0]))
    words = [w.tolist() for w in words]
    want = expected(pairs, words, s)
    check_texts(b, want)

    def upload(per_pair, order):
        """per_pair[i]: pair i's words; laid into one pool in `order`, with a few words of padding between the CIGARs."""
        pool, off = [], [0] * len(per_pair)
        for i in order:
            pool += [0xDEAD0] * 3
            off[i] = len(pool)
            pool += per_pair[i]
        d = (_to_device(np.array(pool + [0], dtype=np.uint32).view(np.int32), torch, dev), _to_device(np.array(off, dtype=np.int64), torch, dev),
             _to_device(np.array([len(w) for w in per_pair], dtype=np.int32), torch, dev))
        torch.cuda.synchronize(dev)
        return d

    # the batch's own words, re-laid in another order: the same text
    d = upload(words, [3, 0, 5, 1, 4, 2])
    check_texts(b, want, cigars=tuple(int(x.data_ptr()) for x in d))
    # every unrenderable variant of pair 2 (not the last in the buffer): its text is empty, its neighbours' text is unchanged
    variants = {k: v[0] for k, v in malformed_variants(words[2]).items()}
    assert {"op15", "eq_plus7", "dropped", "huge"} <= set(variants)
    m = len(words[2]) // 2
    variants["len0"] = words[2][:m] + [0 << 4 | OP_I] + words[2][m:]
    variants["huge_run"] = [0x0FFFFFFF << 4 | OP_EQ] * 20
    for name, bad in variants.items():
        per_pair = [list(w) for w in words]
        per_pair[2] = bad
        assert py_texts(bad, *pairs[2]) is None and mw.cigar_text(0, pairs[2][0], pairs[2][1], bad) is None, name
        d = upload(per_pair, [1, 4, 2, 0, 5, 3])
        check_texts(b, [EMPTY if i == 2 else w for i, w in enumerate(want)], cigars=tuple(int(x.data_ptr()) for x in d))
    # n_words == 0 (and below): a foreign pair without a CIGAR
    per_pair = [list(w) for w in words]
    per_pair[5] = []
    d = list(upload(per_pair, [1, 4, 0, 5, 3, 2]))
    check_texts(b, [EMPTY if i == 5 else w for i, w in enumerate(want)], cigars=tuple(int(x.data_ptr()) for x in d))
    cnt = [len(w) for w in per_pair]
    cnt[0] = -3
    d[2] = _to_device(np.array(cnt, dtype=np.int32), torch, dev)
    torch.cuda.synchronize(dev)
    check_texts(b, [EMPTY if i in (0, 5) else w for i, w in enumerate(want)], cigars=tuple(int(x.data_ptr()) for x in d))
    b.free()


def test_lifetimes(engine):
    import torch
    dev = torch.device("cuda:0")
    pairs = [synth_pair(500 + i, 200 + 30 * i, 0.07) for i in range(12)]
    pk = PackedBatch(pairs)
    b = engine.upload(pk)
    assert all(b.dev_text(kind) is None for kind in KINDS)
    b.align(cigar_opt(PEN_SETS[0]))
    s0, _, nc0 = b.results()
    assert all(b.dev_text(kind) is None for kind in KINDS)
    want0 = expected(pairs, own_words(b, nc0), s0)
    before = engine.stats().dev_bytes
    b.text(mw.MWF_TXT_CS)
    with_cs = engine.stats().dev_bytes
    total_cs = sum(len(w[mw.MWF_TXT_CS]) for w in want0)
    assert with_cs - before >= total_cs + 8 * (b.n + 1)            # the pool and its offsets are accounted
    b.text(mw.MWF_TXT_MD)
    # two kinds live at once, each at its own pointer, read zero-copy as torch tensors
    cs, md = b.dev_text(mw.MWF_TXT_CS), b.dev_text(mw.MWF_TXT_MD)
    assert cs and md and cs[0] != md[0] and b.dev_text(mw.MWF_TXT_SAM) is None
    for (ptr, off_ptr, total), kind in ((cs, mw.MWF_TXT_CS), (md, mw.MWF_TXT_MD)):
        off = torch.as_tensor(mw.DevArray(off_ptr, b.n + 1, "<i8"), device=dev).cpu().numpy()
        raw = torch.as_tensor(mw.DevArray(ptr, total, "|u1"), device=dev).cpu().numpy().tobytes()
        assert [raw[off[i]:off[i + 1]] for i in range(b.n)] == [w[kind] for w in want0]
    # a re-align makes them stale; the next text follows the new CIGARs
    b.align(cigar_opt(PEN_SETS[1]))
    assert all(b.dev_text(kind) is None for kind in KINDS)
    s1, _, nc1 = b.results()
    want1 = expected(pairs, own_words(b, nc1), s1)
    assert want1 != want0
    check_texts(b, want1)
    # the same batch wrapped (sequences only in device memory): the same text
    wb = engine.wrap_packed(pk, dev)
    wb.align(cigar_opt(PEN_SETS[1]))
    wb.results()
    check_texts(wb, want1)
    wb.free()
    # score-only: there are no CIGARs to render
    b.align(mw.opt_init())
    b.results()
    for kind in KINDS:
        with pytest.raises(RuntimeError, match="score-only"):
            b.text(kind)
        assert b.dev_text(kind) is None
    with pytest.raises(RuntimeError):
        b.text(mw.MWF_TXT_KINDS)
    held = engine.stats().dev_bytes
    b.free()
    assert engine.stats().dev_bytes <= held - (with_cs - before)   # the pools go with the batch
