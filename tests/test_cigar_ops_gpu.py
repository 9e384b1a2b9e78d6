"""The device-side summary / self-check and coordinate-map kernels (csrc/mwf_cigar_ops.hip) through Batch.summary(), Batch.coord_map() and
Batch.dev_cigars().  Bar: integer equality, field by field, with the host twin (mwf_cigar_summary), with an independent Python / numpy
restatement of the rule (tests/cigar_ops_ref.py) and with mwf_cigar2score / the batch's own s.  Shapes: the smallest that reach every path of
the kernels — one-wave, 256- and 1024-thread workgroups, one and several passes over the words (the 64-bit carry), a single 5000-base word
(the per-base spread), empty sequences, stopped pairs, corrupted sequences and malformed foreign CIGARs."""
import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import synth_pair, fuzz_pairs, skewed_pairs, random_seq, PackedBatch
from conftest import load_golden, golden_inputs
from cigar_ops_ref import FIELDS, NO_CIGAR, INT32_MIN, OP_EQ, OP_X, py_summary, py_maps, rec, malformed_variants

pytestmark = pytest.mark.gpu

PEN_SETS = ((4, 4, 2, 15, 1), (4, 6, 3, 26, 1))
PEN_KEYS = ("x", "o1", "e1", "o2", "e2")


def cigar_opt(pen, **kw):
    return mw.opt_init(flag=mw.MWF_F_CIGAR, **dict(zip(PEN_KEYS, pen)), **kw)


@pytest.fixture(scope="module")
def engine():
    e = mw.Engine(0)
    yield e
    e.close()


def own_words(b, nc):
    b.fetch_cigars()
    return [b.cigar(i, int(nc[i])) for i in range(b.n)]


def check_batch(b, pairs, pen, s, nc, expect_all_valid=True):
    """Every record against the host twin, the restatement and s; both maps against the numpy expansion of the batch's CIGARs."""
    o = cigar_opt(pen)
    words = own_words(b, nc)
    got = b.summary()
    assert got.dtype == mw.SUMMARY_DTYPE and len(got) == len(pairs)
    stopped = []
    for i, (t, q) in enumerate(pairs):
        r = rec(got[i])
        if s[i] < 0:
            assert r == NO_CIGAR, (i, r)
            stopped.append(i)
            continue
        assert r == rec(mw.cigar_summary(t, q, o, words[i])), (i, r)
        assert r == py_summary(pen, words[i], t, q), (i, r)
        assert r[10] == -1 and r[11] == 1 and r[0] == int(s[i]) and r[9] == int(nc[i]), (i, r, int(s[i]))
        assert r[:3] == mw.cigar2score(o, words[i].tolist()), i
    assert not (expect_all_valid and stopped), stopped
    for which in (0, 1):
        vals, off = b.coord_map(which)
        lens = [len(p[1 - which]) for p in pairs]
        assert off.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        for i, (t, q) in enumerate(pairs):
            sl = vals[off[i]:off[i + 1]]
            if s[i] < 0:
                assert (sl == INT32_MIN).all(), (which, i)
            else:
                assert np.array_equal(sl, py_maps(words[i], len(t), len(q))[which]), (which, i)
    return got, words


@pytest.fixture(scope="module")
def mixed_pairs():
    return fuzz_pairs(5, 120, 1500) + skewed_pairs(9, 40, 200, 1200)


@pytest.mark.parametrize("pen", PEN_SETS)
def test_mixed_batch(engine, mixed_pairs, pen):
    """160 pairs on the 16 / 64 / 256 granularities, unrelated pairs, two pairs empty on both sides, up to 549 words: the 256-thread geometry,
    one to three passes."""
    pairs = mixed_pairs
    assert len(pairs) == 160 and sum(1 for t, q in pairs if not t and not q) == 2
    b = engine.upload(PackedBatch(pairs))
    b.align(cigar_opt(pen))
    s, it, nc = b.results()
    assert (s >= 0).all()
    if pen == PEN_SETS[0]:
        assert int(nc.max()) == 549
    check_batch(b, pairs, pen, s, nc)
    b.free()


def long_pairs():
    ident = random_seq(77, 5000)
    q300 = random_seq(78, 300)
    return [synth_pair(7, 6000, 0.2), synth_pair(7, 12000, 0.2), (ident, ident), synth_pair(11, 3000, 0.05), (b"", q300), (q300, b"")]


def test_long_and_degenerate_cigars(engine):
    """1840 and 3729 words (8 and 15 passes of 256: the pass-to-pass carry), `5000=` (one word, 5000 bases spread over the lanes), 300I, 300D."""
    pairs = long_pairs()
    pen = PEN_SETS[0]
    b = engine.upload(PackedBatch(pairs))
    b.align(cigar_opt(pen))
    s, it, nc = b.results()
    assert s.tolist() == [5296, 10640, 0, 744, 315, 315]       # (300I / 300D: min(4 + 2 * 300, 15 + 300))
    assert nc.tolist() == [1840, 3729, 1, 281, 1, 1]
    got, words = check_batch(b, pairs, pen, s, nc)
    assert words[2].tolist() == [5000 << 4 | 7] and words[4].tolist() == [300 << 4 | 1] and words[5].tolist() == [300 << 4 | 2]
    assert rec(got[2]) == (0, 5000, 5000, 5000, 0, 0, 0, 0, 0, 1, -1, 1)
    assert rec(got[4]) == (315, 0, 300, 0, 0, 300, 0, 1, 0, 1, -1, 1)
    assert rec(got[5]) == (315, 300, 0, 0, 0, 0, 300, 0, 1, 1, -1, 1)
    b.free()


def test_stopped_pairs(engine):
    """max_s = 100: the diverged pairs stop (s == -1): all-zero records with flags == 0, maps of INT32_MIN; the identical pair stays valid."""
    pairs = long_pairs()
    pen = PEN_SETS[0]
    b = engine.upload(PackedBatch(pairs))
    b.align(cigar_opt(pen, max_s=100))
    s, it, nc = b.results()
    assert s[3] == -1 and s[2] == 0
    got, _ = check_batch(b, pairs, pen, s, nc, expect_all_valid=False)
    assert rec(got[3]) == NO_CIGAR and rec(got[2])[10:] == (-1, 1)
    b.free()


def test_detection_through_a_wrapped_batch(engine):
    """Sequences a torch program owns: corrupt one base under an '=' and one under an 'X' after the align; first_bad names exactly those words."""
    import torch
    dev = torch.device("cuda:0")
    pairs = [synth_pair(300 + i, 350 + 40 * i, 0.08) for i in range(8)]
    pk = PackedBatch(pairs)
    pen = PEN_SETS[0]
    b = engine.wrap_packed(pk, dev)
    seqs = b._keep[0]
    b.align(cigar_opt(pen))
    s, it, nc = b.results()
    clean = b.summary()
    assert (clean["first_bad"] == -1).all() and (clean["score"] == s).all()
    words = own_words(b, nc)

    def locate(i, want_op, min_len):
        ti = qj = 0
        for w, word in enumerate(words[i].tolist()):
            op, ln = word & 15, word >> 4
            if op == want_op and ln >= min_len:
                return w, ti + ln // 2, qj + ln // 2
            ti += ln if op != 1 else 0
            qj += ln if op != 2 else 0
        raise AssertionError("no such word")

    a_pair, b_pair = 2, 5
    wa, ta, qa = locate(a_pair, OP_EQ, 3)
    wb, tb, qb = locate(b_pair, OP_X, 1)
    old = pairs[a_pair][1][qa]
    seqs[int(pk.q_off[a_pair]) + qa] = next(c for c in b"ACGT" if c != old)               # '=' now covers a mismatch
    seqs[int(pk.q_off[b_pair]) + qb] = pairs[b_pair][0][tb]                              # 'X' now covers a match
    torch.cuda.synchronize(dev)
    after = b.summary()
    want_bad = np.full(len(pairs), -1)
    want_bad[a_pair], want_bad[b_pair] = wa, wb
    assert after["first_bad"].tolist() == want_bad.tolist()
    for f in FIELDS:
        if f != "first_bad":
            assert (after[f] == clean[f]).all(), f
    b.free()


def _to_device(arr, torch, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def test_foreign_cigars(engine):
    import torch
    dev = torch.device("cuda:0")
    pairs = [synth_pair(110 + i, 300 + 60 * i, 0.06) for i in range(6)]   # (seeds whose CIGARs end in an "=": malformed_variants needs that)
    pen = PEN_SETS[0]
    o = cigar_opt(pen)
    b = engine.upload(PackedBatch(pairs))
    b.align(o)
    s, it, nc = b.results()
    own = b.summary()
    words = [w.tolist() for w in own_words(b, nc)]

    def summarize_foreign(per_pair, order):
        """per_pair[i]: pair i's words; laid into one pool in `order`, with a few words of padding between the CIGARs."""
        pool, off = [], [0] * len(per_pair)
        for i in order:
            pool += [0xDEAD0] * 3
            off[i] = len(pool)
            pool += per_pair[i]
        d = (_to_device(np.array(pool + [0], dtype=np.uint32).view(np.int32), torch, dev), _to_device(np.array(off, dtype=np.int64), torch, dev),
             _to_device(np.array([len(w) for w in per_pair], dtype=np.int32), torch, dev))
        torch.cuda.synchronize(dev)
        out = b.summary(o, cigars=tuple(int(x.data_ptr()) for x in d))
        del d
        return out

    # the batch's own words, re-laid in another order: identical records
    again = summarize_foreign(words, [3, 0, 5, 1, 4, 2])
    assert again.tobytes() == own.tobytes()
    # malformed words on pairs that are not the last in the buffer (an unclipped overrun would read the next pair's bases, not fault)
    names = ["op15", "eq_plus7", "dropped", "huge", "eq_plus7_mid"]
    per_pair, want_bad = [list(w) for w in words], [-1] * 6
    for i, name in enumerate(names):
        per_pair[i], want_bad[i] = malformed_variants(words[i])[name]
    per_pair[5] = []                                                   # n_words == 0: a foreign pair without a CIGAR
    got = summarize_foreign(per_pair, [1, 4, 0, 5, 3, 2])
    for i in range(5):
        t, q = pairs[i]
        assert rec(got[i]) == rec(mw.cigar_summary(t, q, o, per_pair[i])) == py_summary(pen, per_pair[i], t, q), (names[i], rec(got[i]))
        assert int(got[i]["first_bad"]) == want_bad[i], (names[i], rec(got[i]))
    assert rec(got[5]) == NO_CIGAR
    # (the host twin, which has no "no CIGAR" notion, calls zero words for a non-empty pair bad at word 0)
    assert rec(mw.cigar_summary(pairs[5][0], pairs[5][1], o, []))[9:] == (0, 0, 1)
    b.free()


def test_lifetimes_and_dev_cigars(engine):
    import torch
    dev = torch.device("cuda:0")
    pairs = [synth_pair(500 + i, 200 + 30 * i, 0.07) for i in range(12)]
    b = engine.upload(PackedBatch(pairs))
    assert not b.dev_summary_ptr() and not b.dev_map_ptr(0) and not b.dev_map_ptr(1)
    b.align(cigar_opt(PEN_SETS[0]))
    s0, _, nc0 = b.results()
    assert not b.dev_summary_ptr()
    first = b.summary()
    assert b.dev_summary_ptr()
    # the records, zero-copy, as a torch tensor: identity without leaving the device
    r = torch.as_tensor(mw.DevArray(b.dev_summary_ptr(), b.n * 12, "<i4"), device=dev).view(b.n, 12)
    ident = (r[:, 3].double() / (r[:, 3] + r[:, 4] + r[:, 5] + r[:, 6]).double()).cpu().numpy()
    cols = first["n_eq"] + first["n_x"] + first["n_ins"] + first["n_del"]
    assert np.array_equal(ident, first["n_eq"] / cols) and (ident > 0.8).all()
    # dev_cigars(): pool, offsets and counts through DevArray equal Batch.cigar(i)
    pool_ptr, off_ptr, nw_ptr, pool_words = b.dev_cigars()
    pool = torch.as_tensor(mw.DevArray(pool_ptr, pool_words, "<i4"), device=dev).cpu().numpy().view(np.uint32)
    off = torch.as_tensor(mw.DevArray(off_ptr, b.n, "<i8"), device=dev).cpu().numpy()
    nw = torch.as_tensor(mw.DevArray(nw_ptr, b.n, "<i4"), device=dev).cpu().numpy()
    assert nw.tolist() == nc0.tolist()
    for i in range(b.n):
        assert pool[off[i]:off[i] + nw[i]].tolist() == b.cigar(i, int(nc0[i])).tolist(), i
    b.map(0)
    assert b.dev_map_ptr(0) and not b.dev_map_ptr(1)
    # a re-align makes everything stale; the next summary follows the new CIGARs
    b.align(cigar_opt(PEN_SETS[1]))
    assert not b.dev_summary_ptr() and not b.dev_map_ptr(0)
    s1, _, nc1 = b.results()
    second = b.summary()
    assert (second["score"] == s1).all() and (second["n_words"] == nc1).all() and (second["first_bad"] == -1).all()
    assert (s1 != s0).any()
    for i, (t, q) in enumerate(pairs):
        assert rec(second[i]) == py_summary(PEN_SETS[1], b.cigar(i, int(nc1[i])), t, q), i
    # score-only: there are no CIGARs to summarise
    b.align(mw.opt_init())
    b.results()
    for call in (b.summary, lambda: b.coord_map(0), b.dev_cigars):
        with pytest.raises(RuntimeError, match="score-only"):
            call()
    assert not b.dev_summary_ptr()
    b.free()


def test_one_long_pair_on_the_whole_device_kernel(engine):
    """The 150 kb golden pair: the 1024-thread geometry behind the whole-device kernel's CIGAR."""
    v = next(v for v in load_golden("long_pairs.jsonl") if v["id"] == "c4-cigar")
    t, q = golden_inputs(v)
    pen = tuple(v["opt"][k] for k in PEN_KEYS)
    b = engine.upload(PackedBatch([(t, q)]))
    b.align(cigar_opt(pen))
    s, it, nc = b.results()
    assert engine.stats().kernel_kind == 1
    words = b.cigar(0, int(nc[0]))
    got = rec(b.summary()[0])
    assert got == rec(mw.cigar_summary(t, q, cigar_opt(pen), words)) == py_summary(pen, words, t, q)
    assert got[10] == -1 and got[0] == v["expect"]["s"] == int(s[0]) and got[9] == v["expect"]["n_cigar"]
    vals, off = b.coord_map(0)
    assert off.tolist() == [0, len(q)]
    if int(words[-1]) & 15 != 2:   # the last query base lies under the last word unless that is a deletion: paired with the last target base, or inserted behind it
        assert int(vals[-1]) == (len(t) - 1 if int(words[-1]) & 15 in (OP_EQ, OP_X) else -1 - len(t))
    assert np.array_equal(vals, py_maps(words, len(t), len(q))[0])
    b.free()
