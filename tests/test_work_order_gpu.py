"""Deal order of the band classes on the shared work counter (mwf_plan.cpp): a scheduling choice only.

Bar: every order the test hook "work_order" selects (length, predicted work, previous n_iter, shortest first) gives bit-identical s, n_iter
and CIGAR words on a batch with more pairs than the 512-thread geometry has workgroups; the per-pair 8-mer sketch the order is predicted from
equals a numpy count of the same statistic, pairs shorter than one 8-mer and bytes outside A/C/G/T included."""
import numpy as np
import pytest
import torch

import miniwfa_amd as mw
from miniwfa_amd.synth import synth_pair, PackedBatch

pytestmark = pytest.mark.gpu

ORDERS = (0, 1, 2, 3)  # length, predicted, oracle (the previous align's n_iter), reversed


def sketch_numpy(t: bytes, q: bytes, k: int = 8) -> int:
    """8-mers of q (2-bit code (byte >> 1) & 3 per base, as the kernels read it) that occur in t."""
    def kmers(s):
        c = (np.frombuffer(s, dtype=np.uint8) >> 1) & 3
        if len(c) < k:
            return np.zeros(0, dtype=np.int64)
        w = np.lib.stride_tricks.sliding_window_view(c.astype(np.int64), k)
        return (w << (2 * np.arange(k - 1, -1, -1))).sum(axis=1)
    return int(np.isin(kmers(q), np.unique(kmers(t))).sum())


@pytest.fixture(scope="module")
def wide_batch():
    # (the headline shape: 10 kb pairs at 5 % run on the 512-thread class, two workgroups per CU)
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 64
    return [synth_pair(77000 + i, 10000, 0.05) for i in range(n)]


@pytest.mark.parametrize("flag", [0, mw.MWF_F_CIGAR])
def test_orders_give_identical_results(wide_batch, flag):
    eng = mw.Engine(0)
    b = eng.upload(PackedBatch(wide_batch))
    o = mw.opt_init(flag=flag)
    ref = None
    try:
        for mode in (0,) + ORDERS:  # (length first: the oracle order reads the n_iter of an earlier align)
            eng.set("work_order", mode)
            b.align(o)
            s, it, nc = b.results()
            cig = None
            if flag:
                b.fetch_cigars()
                cig = [b.cigar(i, int(nc[i])).tolist() for i in range(len(wide_batch))]
            if ref is None:
                ref = (s.copy(), it.copy(), nc.copy(), cig)
                assert (s >= 0).all()
                continue
            assert np.array_equal(s, ref[0]), f"order {mode}: s differs"
            assert np.array_equal(it, ref[1]), f"order {mode}: n_iter differs"
            if flag:
                assert np.array_equal(nc, ref[2]), f"order {mode}: CIGAR lengths differ"
                bad = [i for i in range(len(cig)) if cig[i] != ref[3][i]]
                assert not bad, f"order {mode}: CIGAR words differ for pairs {bad[:8]}"
    finally:
        b.free()
        eng.close()


def test_pair_sketch_matches_numpy():
    rng = np.random.default_rng(5)
    pairs = [synth_pair(88000 + i, int(n), 0.05) for i, n in enumerate((1, 3, 7, 8, 9, 15, 16, 200, 1000, 10000))]
    pairs += [(b"ACGTACG", b"ACGTACGT"), (b"ACGTACGTAC", b"ACG"), (b"A", b"ACGTACGTACGT")]
    # bytes outside A/C/G/T (N, lowercase, IUPAC codes, anything): the sketch reads every byte through the same 2-bit code
    for i in range(4):
        t, q = synth_pair(89000 + i, 3000, 0.08)
        noisy = []
        for seq, alphabet in ((t, b"NnRYacgtX*"), (q, b"Nn-acgtWS")):
            a = np.frombuffer(seq, dtype=np.uint8).copy()
            at = rng.choice(len(a), size=len(a) // 20, replace=False)
            a[at] = rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=len(at))
            noisy.append(a.tobytes())
        pairs.append(tuple(noisy))
    eng = mw.Engine(0)
    b = eng.upload(PackedBatch(pairs))
    try:
        got = b.work_sketch()
        for i, (t, q) in enumerate(pairs):
            assert int(got[i]) == sketch_numpy(t, q), (i, len(t), len(q), int(got[i]), sketch_numpy(t, q))
    finally:
        b.free()
        eng.close()
