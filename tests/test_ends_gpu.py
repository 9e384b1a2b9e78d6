"""Ends-free alignment on the device (mwf_gpu_batch_align_ends, kernel mwf_ends.hip) against the yardsticks of tests/ends_ref.py: the DP optimum,
the CIGAR checker, the restated pass for n_iter, and — with four zero allowances — the library's own global alignment and the reference's vectors."""
import collections
import ctypes as C

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, fuzz_pairs, mutate, random_seq, synth_pair
from conftest import golden_inputs, load_golden

import ends_ref as er
from test_ends_cpu import FIXED, rand_pair

pytestmark = pytest.mark.gpu

FREE = er.FREE
PEN_A, PEN_B = (4, 4, 2, 15, 1), (4, 6, 3, 26, 1)


def opt_of(pen, cigar, **kw):
    x, o1, e1, o2, e2 = pen
    return mw.opt_init(flag=mw.MWF_F_CIGAR if cigar else 0, x=x, o1=o1, e1=e1, o2=o2, e2=e2, **kw)


@pytest.fixture(scope="module")
def eng():
    e = mw.Engine(0)
    yield e
    e.close()


def collect(b, cigar):
    s, it, nc = b.results()
    cig = None
    if cigar:
        b.fetch_cigars()
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(b.n)]
    return s.tolist(), it.tolist(), nc.tolist(), cig


def run_ends(eng, pairs, opt, ends):
    """-> (s, n_iter, n_cigar, CIGAR words or None, ranges) of one ends-free align of `pairs`."""
    b = eng.upload(PackedBatch(pairs))
    try:
        b.align_ends(opt, *ends)
        return collect(b, bool(opt.flag & mw.MWF_F_CIGAR)) + (b.ranges().tolist(),)
    finally:
        b.free()


def check_all(pairs, opt, ends, res, dp=True):
    """Every pair: s is the DP optimum (dp) and the CIGAR aligns the reported ranges at that cost."""
    s, it, nc, cig, rng = res
    pen = er.pen_of(opt)
    for i, (t, q) in enumerate(pairs):
        if dp:
            assert s[i] == er.dp_score(t, q, pen, ends), (i, ends, s[i])
        assert len(cig[i]) == nc[i]
        er.check_cigar(mw, opt, t, q, cig[i], rng[i], ends, s[i])


# ---- zero allowances: the global alignment, bit for bit

@pytest.fixture(scope="module")
def fuzz64():
    pairs = fuzz_pairs(611, 64, max_len=700)
    pairs[5] = synth_pair(9005, 600, 0.15)  # penalty beyond 256: the pass crosses a shrink
    return pairs


@pytest.mark.parametrize("pen", [PEN_A, PEN_B])
@pytest.mark.parametrize("cigar", [False, True])
def test_zero_allowances_equal_global(eng, fuzz64, pen, cigar):
    opt = opt_of(pen, cigar)
    b = eng.upload(PackedBatch(fuzz64))
    try:
        b.align(opt)
        want = collect(b, cigar)
        assert want[0][5] >= 257
        b.align_ends(opt)
        assert eng.stats().kernel_kind == 3
        got = collect(b, cigar)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
        assert got[3] == want[3]
        rng = b.ranges().tolist()
        for i, (t, q) in enumerate(fuzz64):
            assert rng[i] == ([0, len(t), 0, len(q)] if cigar else [-1, len(t), -1, len(q)]), i
    finally:
        b.free()


def test_zero_allowances_equal_reference_vectors(eng):
    """The reference's stored answers.  Every vector is aligned in high-memory mode (there is no other here): s of all hundred, the CIGAR of all
    but the chain-mode vector (a heuristic's), n_iter of those the reference also ran in high-memory mode (a low-memory run counts its second pass)."""
    groups = collections.defaultdict(list)
    for v in load_golden("exact_small.jsonl")[:100]:
        o = v["opt"]
        groups[(o["flag"] & 1, o["x"], o["o1"], o["e1"], o["o2"], o["e2"], o["max_s"], o["max_iter"])].append(v)
    n_it = 0
    for (cigar, x, o1, e1, o2, e2, max_s, max_iter), vs in groups.items():
        pairs = [golden_inputs(v) for v in vs]
        opt = mw.opt_init(flag=cigar, x=x, o1=o1, e1=e1, o2=o2, e2=e2, max_s=max_s, max_iter=max_iter)
        s, it, nc, cig, rng = run_ends(eng, pairs, opt, (0, 0, 0, 0))
        for i, v in enumerate(vs):
            e = v["expect"]
            assert s[i] == e["s"], v["id"]
            if v["entry"] != "chain" and cigar:
                assert mw.cigar_str(cig[i]) == (e["cigar"] or ""), v["id"]
            if v["entry"] == "exact" and v["opt"]["step"] == 0:
                assert it[i] == e["n_iter"], v["id"]
                n_it += 1
    assert n_it >= 49


# ---- read in window: origin windows wider than the workgroup

def window_pairs(seed, n, t_lo, t_hi, q_lo, q_hi, p_lo, p_hi):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(n):
        tl = int(rng.integers(t_lo, t_hi + 1))
        t = random_seq(seed * 1000 + k, tl)
        m = int(rng.integers(q_lo, min(q_hi, tl) + 1))
        a = int(rng.integers(0, tl - m + 1))
        q = mutate(t[a:a + m], seed * 1000 + 500 + k, float(rng.uniform(p_lo, p_hi)))
        pairs.append((t, q))
    return pairs


def test_read_in_window(eng):
    pairs = window_pairs(31, 48, 400, 900, 100, 300, 0.05, 0.10)
    pairs[0] = (random_seq(77, 900), pairs[0][1])  # (at least one window beyond 512 columns, whatever the draw)
    assert sum(len(t) >= 700 for t, _ in pairs) >= 4
    opt = opt_of(PEN_A, True)
    ends = (FREE, FREE, 0, 0)
    res = run_ends(eng, pairs, opt, ends)
    check_all(pairs, opt, ends, res)
    for (t, q), r in zip(pairs, res[4]):
        assert r[2] == 0 and r[3] == len(q)


# ---- allowance grid, ties, n_iter, symmetry

def test_allowance_grid(eng):
    rng = np.random.default_rng(5)
    pairs = [rand_pair(rng, 80, two_letter=k % 2 == 1) for k in range(12)]
    swapped = [(q, t) for t, q in pairs]
    allow = (0, 1, 7, 1000)
    opt = opt_of(PEN_A, True)
    pen = er.pen_of(opt)
    sets = [tuple(int(allow[v]) for v in rng.integers(0, 4, 4)) for _ in range(12)] + [(0, 0, 0, 0), (1000, 1000, 1000, 1000), (1000, 0, 0, 1000), (0, 1000, 1000, 0)]
    assert len(sets) == 16
    n_checked = 0
    for ends in sets:
        res = run_ends(eng, pairs, opt, ends)
        check_all(pairs, opt, ends, res)
        for i, (t, q) in enumerate(pairs):
            want = er.wfa_ends(t, q, pen, ends)
            assert (res[0][i], res[1][i], res[4][i][1], res[4][i][3]) == want, (i, ends)
            n_checked += 1
        mirror = (ends[2], ends[3], ends[0], ends[1])
        assert run_ends(eng, swapped, opt_of(PEN_A, False), mirror)[0] == res[0], ends
    assert n_checked >= 150


# ---- edges

def test_edges(eng):
    opt = opt_of(PEN_A, True)
    t40 = random_seq(1, 40)
    a, bq = random_seq(2, 60), random_seq(3, 25)
    cases = [
        (b"", b"ACGT", (0, 0, 0, 0)), (b"ACGTAC", b"", (0, 0, 0, 0)), (b"", b"", (0, 0, 0, 0)), (b"", b"", (3, 3, 3, 3)),
        (b"", b"ACGT", (0, 0, 2, 1)), (b"ACGTAC", b"", (1, 2, 0, 0)),
        (t40, t40, (0, 0, 0, 0)), (t40, t40, (5, 5, 5, 5)),
        (random_seq(4, 300), random_seq(4, 300)[120:200], (FREE, FREE, 0, 0)),       # an exact substring
        (a + bq, bq + random_seq(5, 30), (0, 0, 0, 0)),
        (a + bq, bq + random_seq(5, 30), (70, 0, 0, 40)),                            # a dovetail: the query hangs off the target's end
        (bq + a, random_seq(6, 30) + bq, (0, FREE, FREE, 0)),                        # ... and off its begin: q_beg and t_end free
        (random_seq(7, 12), random_seq(8, 9), (FREE, FREE, FREE, FREE)),             # allowances beyond the sequences: an empty alignment wins
    ]
    by_ends = collections.defaultdict(list)
    for t, q, ends in cases:
        by_ends[ends].append((t, q))
    out = {}
    for ends, pairs in by_ends.items():
        res = run_ends(eng, pairs, opt, ends)
        check_all(pairs, opt, ends, res)
        for i, p in enumerate(pairs):
            out[(p, ends)] = (res[0][i], res[3][i], tuple(res[4][i]))
    assert out[((t40, t40), (0, 0, 0, 0))] == (0, [40 << 4 | 7], (0, 40, 0, 40))
    s, cig, r = out[((cases[8][0], cases[8][1]), cases[8][2])]
    assert (s, cig, r) == (0, [80 << 4 | 7], (120, 200, 0, 80))
    s, cig, r = out[((cases[10][0], cases[10][1]), cases[10][2])]
    assert (s, cig, r) == (0, [25 << 4 | 7], (60, 85, 0, 25))
    s, cig, r = out[((cases[11][0], cases[11][1]), cases[11][2])]
    assert (s, cig, r) == (0, [25 << 4 | 7], (0, 25, 30, 55))
    s, cig, r = out[((cases[12][0], cases[12][1]), cases[12][2])]
    assert (s, cig, r) == (0, [], (12, 12, 0, 0))
    assert out[((b"", b""), (3, 3, 3, 3))] == (0, [], (0, 0, 0, 0))


def test_fixed_answers(eng):
    opt = opt_of(PEN_A, True)
    for t, q, ends, s, words, rng in FIXED:
        res = run_ends(eng, [(t, q)], opt, ends)
        assert (res[0][0], res[3][0], tuple(res[4][0])) == (s, words, rng)


# ---- stop rules, score-only against CIGAR

def test_stops(eng):
    pairs = [synth_pair(4400 + k, 300, 0.10) for k in range(6)]
    full = run_ends(eng, pairs, opt_of(PEN_A, True), (0, 0, 0, 0))
    assert min(full[0]) > 20
    for kw in (dict(max_s=10), dict(max_iter=200)):
        for cigar in (False, True):
            s, it, nc, cig, rng = run_ends(eng, pairs, opt_of(PEN_A, cigar, **kw), (3, 3, 3, 3))
            assert s == [-1] * 6 and nc == [0] * 6 and rng == [[-1] * 4] * 6, kw


def test_score_only_equals_cigar(eng):
    pairs = window_pairs(47, 24, 200, 600, 80, 200, 0.05, 0.15) + fuzz_pairs(3, 8, max_len=300)
    for ends in ((FREE, FREE, 0, 0), (7, 0, 0, 1000)):
        a = run_ends(eng, pairs, opt_of(PEN_B, False), ends)
        b = run_ends(eng, pairs, opt_of(PEN_B, True), ends)
        assert a[0] == b[0] and a[1] == b[1]
        assert [(r[1], r[3]) for r in a[4]] == [(r[1], r[3]) for r in b[4]]
        assert all(r[0] == -1 and r[2] == -1 for r in a[4]) and a[2] == [0] * len(pairs)


# ---- the traceback arena: re-runs on fewer workgroups

def arena_pairs():
    return window_pairs(59, 8, 2600, 2600, 2000, 2000, 0.15, 0.15)


PEN_UNIT = (1, 1, 1, 1, 1)
ARENA_SLACK = 600  # window - read: the bases a read can have in front of it, or behind it, in its window


def arena_run(eng, pen, ends, budget_mb):
    """The eight pairs under the default budget and under `budget_mb` (a fresh engine) -> (default result, budget result, re-runs under the budget)."""
    pairs = arena_pairs()
    opt = opt_of(pen, True)
    want = run_ends(eng, pairs, opt, ends)
    print("penalties:", want[0], "traceback bytes per pair (n_iter):", want[1])
    e2 = mw.Engine(0)
    try:
        e2.set("tb_budget_mb", budget_mb(want) if callable(budget_mb) else budget_mb)
        got = run_ends(e2, pairs, opt, ends)
        return pairs, opt, want, got, e2.stats().n_retries
    finally:
        e2.close()


def test_arena_rerun(eng):
    """tb_budget_mb = 1: eight slots of 128 KB on the first launch, one slot of 1 MB on the re-run.  A pair's traceback rows are one byte per cell (n_iter bytes)
    and the arena must hold one pair's on one slot, so penalties and allowances — which the arena test is free to choose — are the ones that make the rows
    of a 2 kb read at 15 % fit 1 MB: unit penalties (the penalty is then about the number of edits, 0.15 x 2000 x ~1.4 bases per event = 400 ... 460) and begin / end
    allowances equal to the window's slack, 600 (what a mapper that knows its window sets).  A row is at most 601 + 2s columns wide, so a pair needs at
    most 601 s + s^2 < 480 KB and, the origin window alone being 601 wide for s >= 400 penalties, more than 128 KB: every pair overflows its first slot and
    fits the re-run's.  (Under the default penalties, s = 1360 ... 1564 and fully free target ends the same pairs need 3.9 ... 4.5 MB each:
    test_arena_fitting_budget_rerun, test_arena_too_small.)"""
    ends = (ARENA_SLACK, ARENA_SLACK, 0, 0)
    pairs, opt, want, got, retries = arena_run(eng, PEN_UNIT, ends, 1)
    assert all((128 << 10) < n < (1 << 20) - 16 * 1024 for n in want[1]), want[1]
    assert retries > 0
    assert got == want
    check_all(pairs, opt, ends, got)


def test_arena_fitting_budget_rerun(eng):
    """Default penalties, target ends fully free: the smallest whole number of MB that holds the largest pair's rows on one slot — but not on eight."""
    ends = (FREE, FREE, 0, 0)
    pairs, opt, want, got, retries = arena_run(eng, PEN_A, ends, lambda w: ((max(w[1]) + 16 * max(w[0]) + 8192) >> 20) + 1)
    assert retries > 0
    assert got == want


def test_arena_too_small(eng):
    """... and 1 MB, which holds none of them: after the re-run on one slot the align fails with the existing message, and the engine's next align is unharmed."""
    pairs = arena_pairs()
    e2 = mw.Engine(0)
    try:
        e2.set("tb_budget_mb", 1)
        with pytest.raises(RuntimeError, match="traceback of pair .* do not fit in device memory"):
            run_ends(e2, pairs, opt_of(PEN_A, True), (FREE, FREE, 0, 0))
        t, q, ends, s, words, rng = FIXED[1]
        res = run_ends(e2, [(t, q)], opt_of(PEN_A, True), ends)
        assert (res[0][0], res[3][0], tuple(res[4][0])) == (s, words, rng)
    finally:
        e2.close()


# ---- refusals

def test_refusals(eng):
    b = eng.upload(PackedBatch([(b"ACGT", b"ACGT")]))
    L = mw.lib()
    try:
        for opt, ends, word in ((mw.opt_init(flag=mw.MWF_F_CIGAR, step=5), (0, 0, 0, 0), "step"),
                                (mw.opt_init(), (0, -1, 0, 0), "allowance"),
                                (mw.opt_init(o2=300), (0, 0, 0, 0), "256")):
            rc = L.mwf_gpu_batch_align_ends(eng.h, b.h, C.byref(opt), C.byref(mw.MwfEnds(*ends)))
            assert rc == -2 and word in eng.error(), (rc, eng.error())
        b.align_ends(mw.opt_init(step=5))  # score-only: the step is not used
        assert b.results()[0].tolist() == [0]
    finally:
        b.free()


# ---- products after the align, and the plain align after it

def test_after_the_align(eng):
    pairs = window_pairs(71, 16, 150, 400, 60, 150, 0.05, 0.10) + [(b"ACGT", b"TTTT")]
    opt = opt_of(PEN_A, True)
    ends = (FREE, FREE, 0, 0)
    b = eng.upload(PackedBatch(pairs))
    try:
        b.align(opt)
        plain = collect(b, True)
        with pytest.raises(RuntimeError):
            b.ranges()
        assert not b.dev_ranges_ptr()
        b.align_ends(opt, *ends)
        s, it, nc, cig = collect(b, True)
        rng = b.ranges().tolist()
        assert b.dev_ranges_ptr()
        sm = b.summary()
        for i in range(b.n):
            assert sm["first_bad"][i] == -1 and sm["score"][i] == s[i], i
            assert sm["t_len"][i] == rng[i][1] - rng[i][0] and sm["q_len"][i] == rng[i][3] - rng[i][2], i
        assert b.texts(mw.MWF_TXT_CIGAR) == [mw.cigar_str(c).encode() for c in cig]
        rows = b.texts(mw.MWF_TXT_ROW_T)
        for i, (t, q) in enumerate(pairs):
            assert rows[i].replace(b"-", b"") == t[rng[i][0]:rng[i][1]], i
        with pytest.raises(RuntimeError):
            b.map(0)
        b.align(opt)
        assert collect(b, True) == plain
        with pytest.raises(RuntimeError):
            b.ranges()
        b.map(0)
    finally:
        b.free()


# ---- host-buffer calls

def test_host_buffer_calls(eng):
    pairs = window_pairs(83, 16, 150, 400, 60, 150, 0.05, 0.10)
    opt = opt_of(PEN_A, True)
    ends = (FREE, 5, 0, 1000)
    s, it, nc, cig, rng = run_ends(eng, pairs, opt, ends)
    got = mw.wfa_ends_batch(pairs, opt, *ends)
    for i in range(len(pairs)):
        assert got[i] == (s[i], it[i], cig[i] or None, tuple(rng[i])), i
    L = mw.lib()
    km = L.km_init()
    try:
        t, q = pairs[3]
        assert mw.wfa_ends(t, q, opt, *ends, km=km) == got[3]
        assert mw.wfa_ends(t, q, opt, *ends) == got[3]
        assert mw.wfa_ends(t, q, opt_of(PEN_A, False), *ends)[:3] == (s[3], it[3], None)
    finally:
        L.km_destroy(km)
