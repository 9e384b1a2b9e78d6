"""Extension alignment on the device (mwf_gpu_batch_align_ext, the EXT form of mwf_ends.hip's kernel) against the restated rule of tests/ext_ref.py on the
shared case list of tests/ext_cases.py, bit for bit: s, n_iter, ranges, info, and the CIGAR through the checker."""
import ctypes as C

import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch

import ext_cases as xc
import ext_ref as xr

pytestmark = pytest.mark.gpu

FREE = mw.ENDS_FREE
RUNS = xc.runs()
BY_NAME = {c.name: c for c in xc.cases()}


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


def collect_ext(b, cigar):
    """-> (s, n_iter, n_cigar, CIGAR words or None, ranges, info) of the batch's extension align."""
    return collect(b, cigar) + (b.ranges().tolist(), b.ext_info().tolist())


def run_ext(eng, pairs, opt, A, Z):
    b = eng.upload(PackedBatch(pairs))
    try:
        b.align_ext(opt, A, Z)
        return collect_ext(b, bool(opt.flag & mw.MWF_F_CIGAR))
    finally:
        b.free()


def check_against_restatement(case, pen, opt, res):
    s, it, nc, cig, rng, info = res
    for i, ((t, q), w) in enumerate(zip(case.pairs, xc.want(case, pen))):
        got = (s[i], it[i], tuple(rng[i]), tuple(info[i]))
        assert got == (w.s, w.n_iter, (0, w.te, 0, w.qe), (w.V, w.s_stop, w.why, w.F)), (case.name, pen, i)
        if cig is None:
            assert nc[i] == 0
        else:
            assert len(cig[i]) == nc[i]
            xr.check_ext_cigar(mw, opt, t, q, cig[i], rng[i], s[i])


@pytest.mark.parametrize("cigar", [True, False], ids=["cigar", "score"])
@pytest.mark.parametrize("run", range(len(RUNS)), ids=[f"{c.name}-o{pen[1]}" for c, pen in RUNS])
def test_case_equals_restatement(eng, run, cigar):
    case, pen = RUNS[run]
    opt = opt_of(pen, cigar)
    res = run_ext(eng, case.pairs, opt, case.A, case.Z)
    assert eng.stats().kernel_kind == 3
    check_against_restatement(case, pen, opt, res)


@pytest.mark.parametrize("name", ["i-mixed-z40", "f-junk200-z100", "g-4200-junk300-z80", "b-empty"])
def test_score_only_equals_cigar(eng, name):
    case = BY_NAME[name]
    a = run_ext(eng, case.pairs, opt_of(xc.PEN_A, False), case.A, case.Z)
    b = run_ext(eng, case.pairs, opt_of(xc.PEN_A, True), case.A, case.Z)
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4] and a[5] == b[5]
    assert a[2] == [0] * len(case.pairs) and a[3] is None


@pytest.mark.parametrize("cigar", [True, False], ids=["cigar", "score"])
def test_no_drop_rule_sweeps_what_the_ends_free_extension_sweeps(eng, cigar):
    """Z = -1: the pass ends where align_ends(0, FREE, 0, FREE) ends — same s_stop, same n_iter — and where the best cell is that end cell, s is equal too."""
    pairs = [p for name in ("a-identical", "b-empty", "c-unrelated-end", "d-related-A1", "e-long-target", "f-junk40-end", "g-4200") for p in BY_NAME[name].pairs]
    pairs += [p for c in xc.cases() if c.name.startswith("h-") for p in c.pairs]
    n_same = n_earlier = 0
    for pen in xc.BOTH:
        opt = opt_of(pen, cigar)
        b = eng.upload(PackedBatch(pairs))
        try:
            b.align_ends(opt, 0, FREE, 0, FREE)
            s0, it0, nc0, cig0 = collect(b, cigar)
            rng0 = b.ranges().tolist()
            b.align_ext(opt, 1, -1)
            s, it, nc, cig, rng, info = collect_ext(b, cigar)
        finally:
            b.free()
        assert [v[1] for v in info] == s0 and it == it0 and all(v[2] == 0 for v in info)
        for i in range(len(pairs)):
            if s[i] == info[i][1]:
                assert s[i] == s0[i], i
                n_same += 1
            else:
                assert s[i] < s0[i] and rng[i][1] <= len(pairs[i][0]) and rng[i][3] <= len(pairs[i][1]), i
                n_earlier += 1
    assert n_same >= 8 and n_earlier >= 4, (n_same, n_earlier)


# ---- the traceback arena: the re-run keeps the mode

def arena_run(eng, pairs, pen, A, Z):
    """The pairs under the default budget and, on a fresh engine, under tb_budget_mb = 1 -> (default result, budget result, re-runs under the budget)."""
    opt = opt_of(pen, True)
    want = run_ext(eng, pairs, opt, A, Z)
    e2 = mw.Engine(0)
    try:
        e2.set("tb_budget_mb", 1)
        got = run_ext(e2, pairs, opt, A, Z)
        return want, got, e2.stats().n_retries
    finally:
        e2.close()


def test_arena_rerun_keeps_the_mode(eng):
    """tb_budget_mb = 1.  A pair's traceback rows are n_iter bytes (12 ... 25 KB for the (f) pairs) and a first launch of S pairs gives each workgroup
    max(4096, 1 MB / S) bytes.  The two (f) pairs 64 times over are 128 slots of 8 KB: every pair overflows its slot and is re-run on fewer workgroups — by the
    EXT form again, or info, ranges and s would be those of the ends-free extension (s 131 ... 170 instead of 78).  The same pairs eight times over — 16 slots of 64 KB —
    fit their first slots: same results, no re-run."""
    f = [BY_NAME["f-junk40-end"].pairs[0], BY_NAME["f-junk200-z100"].pairs[0]]
    ref = (xr.wfa_ext(*f[0], xc.PEN_A, 1, 100), xr.wfa_ext(*f[1], xc.PEN_A, 1, 100))
    assert [(r.s, r.s_stop, r.why) for r in ref] == [(78, 131, 0), (78, 170, 1)] and min(r.n_iter for r in ref) > 8192 and max(r.n_iter for r in ref) < 65536
    for copies, rerun in ((64, True), (8, False)):
        pairs = f * copies
        want, got, retries = arena_run(eng, pairs, xc.PEN_A, 1, 100)
        assert got == want
        assert retries >= len(pairs) if rerun else retries == 0, retries
        for i in range(len(pairs)):
            r = ref[i % 2]
            assert (got[0][i], got[1][i], tuple(got[4][i]), tuple(got[5][i])) == (r.s, r.n_iter, (0, r.te, 0, r.qe), (r.V, r.s_stop, r.why, r.F)), i


# ---- refusals

def test_refusals_leave_a_usable_engine(eng):
    case = BY_NAME["f-junk200-z50"]
    b = eng.upload(PackedBatch(case.pairs))
    L = mw.lib()
    try:
        for opt, ext, word in ((mw.opt_init(), (0, -1), "match"),
                               (mw.opt_init(), (1, -2), "zdrop"),
                               (mw.opt_init(), (1 << 22, -1), "2^31"),  # (1002 bases: 2^22 x 1002 >= 2^31)
                               (mw.opt_init(flag=mw.MWF_F_CIGAR, step=5), (1, -1), "step"),
                               (mw.opt_init(o2=300), (1, -1), "256")):
            rc = L.mwf_gpu_batch_align_ext(eng.h, b.h, C.byref(opt), C.byref(mw.MwfExt(*ext)))
            assert rc == -2 and word in eng.error(), (rc, eng.error())
        with pytest.raises(RuntimeError):
            b.ext_info()  # (nothing was aligned)
        opt = opt_of(xc.PEN_A, True)
        b.align_ext(opt, case.A, case.Z)
        check_against_restatement(case, xc.PEN_A, opt, collect_ext(b, True))
    finally:
        b.free()


def test_stopped_pairs(eng):
    case = BY_NAME["f-junk200-z100"]
    for kw in (dict(max_s=60), dict(max_iter=3000)):
        for cigar in (False, True):
            s, it, nc, cig, rng, info = run_ext(eng, case.pairs, opt_of(xc.PEN_A, cigar, **kw), 1, 100)
            assert s == [-1] and nc == [0] and rng == [[-1] * 4] and info == [[-1] * 4], kw


# ---- products after the align, and the other aligns after it

def test_after_the_align(eng):
    case = BY_NAME["i-mixed-z40"]
    pairs = case.pairs
    opt = opt_of(xc.PEN_A, True)
    b = eng.upload(PackedBatch(pairs))
    try:
        b.align_ext(opt, case.A, case.Z)
        s, it, nc, cig, rng, info = collect_ext(b, True)
        assert b.dev_ranges_ptr() and b.dev_ext_info_ptr()
        sm = b.summary()
        for i in range(b.n):
            assert sm["first_bad"][i] == -1 and sm["score"][i] == s[i], i
            assert sm["t_len"][i] == rng[i][1] and sm["q_len"][i] == rng[i][3], i
        assert b.texts(mw.MWF_TXT_CIGAR) == [mw.cigar_str(c).encode() for c in cig]
        rows = b.texts(mw.MWF_TXT_ROW_T)
        for i, (t, q) in enumerate(pairs):
            assert rows[i].replace(b"-", b"") == t[:rng[i][1]], i
        with pytest.raises(RuntimeError):
            b.map(0)
    finally:
        b.free()


def test_align_sequence_on_one_batch(eng):
    """align, align_ends, align_ext, and back: each gives what a fresh batch gives, and each forgets what only the previous kind of align has."""
    case = BY_NAME["i-mixed-z40"]
    pairs = case.pairs
    opt = opt_of(xc.PEN_A, True)
    ends = (0, FREE, 0, FREE)

    def fresh(do):
        b = eng.upload(PackedBatch(pairs))
        try:
            return do(b)
        finally:
            b.free()

    def plain(b):
        b.align(opt)
        return collect(b, True)

    def ends_free(b):
        b.align_ends(opt, *ends)
        return collect(b, True) + (b.ranges().tolist(),)

    def ext(b):
        b.align_ext(opt, case.A, case.Z)
        return collect_ext(b, True)

    want_plain, want_ends, want_ext = fresh(plain), fresh(ends_free), fresh(ext)
    b = eng.upload(PackedBatch(pairs))
    try:
        assert plain(b) == want_plain
        assert not b.dev_ext_info_ptr()
        assert ends_free(b) == want_ends
        with pytest.raises(RuntimeError):
            b.ext_info()
        assert not b.dev_ext_info_ptr()
        assert ext(b) == want_ext
        assert ends_free(b) == want_ends
        with pytest.raises(RuntimeError):
            b.ext_info()
        assert ext(b) == want_ext
        assert plain(b) == want_plain
        with pytest.raises(RuntimeError):
            b.ext_info()
        with pytest.raises(RuntimeError):
            b.ranges()
        b.map(0)
        assert ext(b) == want_ext
    finally:
        b.free()
    check_against_restatement(case, xc.PEN_A, opt, want_ext)


# ---- host-buffer calls

def test_host_buffer_calls(eng):
    case = BY_NAME["i-mixed-z40"]
    pairs = case.pairs[:24]
    opt = opt_of(xc.PEN_A, True)
    s, it, nc, cig, rng, info = run_ext(eng, pairs, opt, case.A, case.Z)
    got = mw.wfa_ext_batch(pairs, opt, case.A, case.Z)
    for i in range(len(pairs)):
        assert got[i] == (s[i], it[i], cig[i] or None, tuple(rng[i]), tuple(info[i])), i
    L = mw.lib()
    km = L.km_init()
    try:
        t, q = pairs[0]
        assert mw.wfa_ext(t, q, opt, case.A, case.Z, km=km) == got[0]
        assert mw.wfa_ext(t, q, opt, case.A, case.Z) == got[0]
        assert mw.wfa_ext(t, q, opt_of(xc.PEN_A, False), case.A, case.Z) == (s[0], it[0], None, tuple(rng[0]), tuple(info[0]))
    finally:
        L.km_destroy(km)
