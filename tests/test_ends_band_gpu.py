"""Per-pair allowances and diagonal bands on the device (mwf_gpu_batch_align_ends_pp / mwf_gpu_batch_align_ext_band, the four kernels of mwf_ends.hip) against the
yardsticks of tests/ends_band_ref.py: bit for bit the banded restatement of the pass (s, n_iter, te, qe, info), the banded DP for s, ends_ref.check_cigar /
ext_ref.check_ext_cigar for the CIGAR, and every CIGAR column's diagonal inside the pair's band.  The references of a pair list are computed once per penalty set."""
import functools
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, mutate, random_seq

import ends_band_ref as br
import ends_ref as er
import ext_ref as xr
from ends_matrix import pen_tuple

pytestmark = pytest.mark.gpu

FREE = er.FREE
I32_MIN, I32_MAX = -0x80000000, 0x7fffffff
DEFAULT = (4, 4, 2, 15, 1)
PEN_UNIT = (1, 1, 1, 1, 1)
# four of the twelve shapes of tests/ends_matrix.py: the default, o == 0, e1 == e2, and a nine-row E / F history (e1 == e2 == 8)
SETS = ("default", "o1zero", "a22", "e88")
ENDS_LINE = re.compile(r"\[libmwf_hip\] (ends-free|extension) launch: T (\d+), (\d+) pairs, grid (\d+), .* per-pair allowances (\d), band (\d)")
STOPPED = [-1, -1, -1, -1]


def opt_of(pen, cigar, **kw):
    x, o1, e1, o2, e2 = pen
    return mw.opt_init(flag=mw.MWF_F_CIGAR if cigar else 0, x=x, o1=o1, e1=e1, o2=o2, e2=e2, **kw)


@pytest.fixture(scope="module")
def eng():
    e = mw.Engine(0)
    yield e
    e.close()


def collect(b, cigar, ext=False):
    """-> dict(s, it, nc, cig, rng, info) of the batch's last align."""
    s, it, nc = b.results()
    cig = None
    if cigar:
        b.fetch_cigars()
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(b.n)]
    return dict(s=s.tolist(), it=it.tolist(), nc=nc.tolist(), cig=cig, rng=b.ranges().tolist(), info=b.ext_info().tolist() if ext else None)


def run_pp(eng, pairs, opt, ends, band):
    b = eng.upload(PackedBatch(list(pairs)))
    try:
        b.align_ends_pp(opt, ends, band)
        assert eng.stats().kernel_kind == 3
        return collect(b, bool(opt.flag & mw.MWF_F_CIGAR))
    finally:
        b.free()


def run_ext(eng, pairs, opt, A, Z, band):
    b = eng.upload(PackedBatch(list(pairs)))
    try:
        b.align_ext(opt, A, Z, band=band)
        return collect(b, bool(opt.flag & mw.MWF_F_CIGAR), ext=True)
    finally:
        b.free()


def launch_lines(err: str):
    return [(m.group(1),) + tuple(int(v) for v in m.groups()[1:]) for m in map(ENDS_LINE.search, err.splitlines()) if m]


def check_ends(got, pairs, opt, ends, bands, want, label=""):
    """Every pair against the restatement (want[i]: (s, n_iter, te, qe) or None), the CIGAR checker and the band.  (The restatement's s is compared with the
    banded DP where `want` is built: once per list, not once per mode.)"""
    cigar = bool(opt.flag & mw.MWF_F_CIGAR)
    per_pair = not np.isscalar(ends[0])
    for i, (t, q) in enumerate(pairs):
        e = ends[i] if per_pair else ends
        if want[i] is None:  # nothing inside the band: the stopped record
            assert (got["s"][i], got["it"][i], got["nc"][i], got["rng"][i]) == (-1, 0, 0, STOPPED), (label, i, got["s"][i], got["it"][i], got["rng"][i])
            continue
        s, n_iter, te, qe = want[i]
        assert (got["s"][i], got["it"][i], got["rng"][i][1], got["rng"][i][3]) == (s, n_iter, te, qe), (label, i, e, bands[i])
        if not cigar:
            assert got["nc"][i] == 0 and got["rng"][i][0] == -1 and got["rng"][i][2] == -1
            continue
        assert len(got["cig"][i]) == got["nc"][i]
        er.check_cigar(mw, opt, t, q, got["cig"][i], got["rng"][i], e, s)
        lo, hi = br.clamp_band(len(t), len(q), bands[i])
        dlo, dhi = br.cigar_diagonals(got["cig"][i], got["rng"][i][0], got["rng"][i][2])
        assert lo <= dlo and dhi <= hi, (label, i, "the CIGAR leaves the band", (dlo, dhi), (lo, hi))


# ---- 1. band geometry on 256 threads: every pair with its own band and its own allowances in one launch -------------------------------------------

ALLOW = ((FREE, FREE, 0, 0), (0, 0, 0, 0), (7, 0, 0, 1000), (20, 20, 20, 20), (FREE, 30, 0, 0), (0, FREE, 0, FREE))


def widen(tl, ql, ends, lo, hi):
    """The band [lo, hi] widened until it reaches the origin and the end diagonals the allowances give: feasible by construction."""
    t_beg, t_end, q_beg, q_end = br.clamp_ends(tl, ql, ends)
    return min(lo, q_beg, ql - tl + t_end), max(hi, -t_beg, ql - tl - q_end)


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """-> (pairs, ends, bands, kinds): 30 pairs of at most 420 + 200 bases.  A read in a window has its true diagonal at -at; the band kinds are
    'w1', 'w3' (width 1 and 3 under read-in-window allowances, not widened), 'edgeNN' (an edge on a multiple of 64 columns or one column either side),
    'sub' (narrower than a wave), 'wide' (wider than 256 columns, tl >= 300 with a free t_beg: an origin window of more than one trip) and 'junk' (unrelated
    sequences under a narrow band: beyond penalty 256 inside the band)."""
    pairs, ends, bands, kinds = [], [], [], []

    def add(t, q, e, lo, hi, kind, keep=False):
        b = (lo, hi) if keep else widen(len(t), len(q), e, lo, hi)
        assert br.feasible(len(t), len(q), e, b), (kind, e, b)
        pairs.append((t, q)), ends.append(e), bands.append(b), kinds.append(kind)

    def window(seed, tl, at, m, p):
        t = random_seq(seed, tl)
        return t, mutate(t[at:at + m], seed + 500, p)

    # width 1 and 3, exactly on the true diagonal (substitutions only keep the read on it) and beside it
    for k, (tl, at, m) in enumerate(((300, 120, 100), (333, 0, 150), (350, 200, 150), (400, 37, 201))):
        t = random_seq(700 + k, tl)
        q = bytearray(t[at:at + m])
        for j in range(5 + k, m, 17):
            q[j] = ord("A") if q[j] != ord("A") else ord("C")
        w = (0, 1)[k % 2]
        add(t, bytes(q), (FREE, FREE, 0, 0), -at - w, -at + w, "w1" if w == 0 else "w3", keep=True)
    add(*window(710, 320, 100, 120, 0.06), (FREE, FREE, 0, 0), -99, -99, "w1", keep=True)     # one diagonal beside the truth, indels in the read
    add(*window(711, 320, 60, 150, 0.08), (FREE, FREE, 0, 0), -61, -59, "w3", keep=True)
    # an edge on a multiple of 64 columns (column = diagonal + tl + 1), and one column either side of it: low edge, then high edge
    for k, off in enumerate((-1, 0, 1)):
        tl, at = 300 + 7 * k, 150
        t, q = window(720 + k, tl, at, 110, 0.05)
        blo = 128 + off                                  # the true diagonal's column is tl + 1 - at = 151 + 7 k
        add(t, q, ALLOW[k % 2 * 4], blo - tl - 1, blo - tl - 1 + 40, f"edge{blo}")
        t, q = window(730 + k, tl, at, 110, 0.05)
        bhi = 192 + off
        add(t, q, ALLOW[0], bhi - tl - 1 - 55, bhi - tl - 1, f"edge{bhi}")
    # narrower than a wave, under every allowance set
    for k, e in enumerate(ALLOW + ALLOW[:2]):
        tl, at, m = 260 + 20 * k, 40 + 11 * k, 120 + 10 * k
        t, q = window(740 + k, tl, at, m, 0.07)
        add(t, q, e, -at - 9 - k, -at + 6 + k, "sub")
    # wider than 256 columns: an origin window of more than one trip of 256 threads
    for k, (tl, at, m) in enumerate(((420, 200, 180), (400, 30, 200), (380, 150, 160), (415, 215, 200))):
        t, q = window(750 + k, tl, at, m, 0.06)
        add(t, q, (FREE, FREE, 0, 0) if k < 3 else (FREE, 40, 0, 0), -at - 140 - 10 * k, -at + 135 + 3 * k, "wide", keep=True)
    # unrelated sequences under a narrow band: the pass crosses the shrink at 256 inside the band
    for k, (tl, ql, w) in enumerate(((150, 150, 0), (140, 160, 1), (200, 190, 2), (130, 170, 20), (170, 170, 4), (190, 200, 3))):
        add(random_seq(760 + k, tl), random_seq(770 + k, ql), (0, 0, 0, 0), -w, w, "junk")
    return tuple(pairs), tuple(ends), tuple(bands), tuple(kinds)


def test_geometry_cases_cover_what_they_claim():
    pairs, ends, bands, kinds = geometry_cases()
    assert 28 <= len(pairs) <= 32
    width = [br.clamp_band(len(t), len(q), b)[1] - br.clamp_band(len(t), len(q), b)[0] + 1 for (t, q), b in zip(pairs, bands)]
    cols = [br.band_columns(len(t), len(q), b) for (t, q), b in zip(pairs, bands)]
    assert sum(w == 1 for w in width) >= 2 and sum(w == 3 for w in width) >= 2
    for edge in (127, 128, 129, 191, 192, 193):
        assert any(edge in c for c in cols), edge
    assert sum(w < 64 for w in width) >= 8
    wide = [i for i, k in enumerate(kinds) if k == "wide"]
    assert all(width[i] > 256 and len(pairs[i][0]) >= 300 and ends[i][0] == FREE for i in wide) and len(wide) >= 3
    assert len(set(ends)) >= 5 and len(set(bands)) == len(bands)
    assert max(len(t) + len(q) + 1 for t, q in pairs) < 8192


@functools.lru_cache(maxsize=None)
def geometry_want(name):
    """The restatement's answers under penalty set `name`, each checked against the banded DP."""
    pairs, ends, bands, kinds = geometry_cases()
    pen = pen_tuple(name)
    want = tuple(br.wfa_ends_band(t, q, pen, e, b) for (t, q), e, b in zip(pairs, ends, bands))
    for (t, q), e, b, w in zip(pairs, ends, bands, want):
        assert w[0] == br.dp_score_band(t, q, pen, e, b), (name, e, b)
    return want


@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
@pytest.mark.parametrize("name", SETS)
def test_band_geometry_256(eng, monkeypatch, capfd, name, cigar):
    pairs, ends, bands, kinds = geometry_cases()
    want = geometry_want(name)
    if name == "default":
        assert sum(w[0] > 256 for w in want) >= 3  # (the junk pairs: beyond a shrink)
        plain = [er.wfa_ends(t, q, pen_tuple(name), e) for (t, q), e in zip(pairs, ends)]
        assert sum(w[:2] != p[:2] for w, p in zip(want, plain)) >= 20  # (the bands bite: another penalty or another n_iter)
    monkeypatch.setenv("MWF_DEBUG", "1")
    opt = opt_of(pen_tuple(name), cigar)
    capfd.readouterr()
    got = run_pp(eng, pairs, opt, ends, bands)
    lines = launch_lines(capfd.readouterr().err)
    assert lines == [("ends-free", 256, len(pairs), lines[0][3], 1, 1)], lines
    check_ends(got, pairs, opt, ends, bands, want, name)


# ---- 2. the 512-thread form: bands at least 8192 diagonals wide that still cut something off; the same pairs under +-100 on 256 threads ----------------

@functools.lru_cache(maxsize=None)
def wide_cases():
    """Three 2 kb reads at 5 % in windows of 8.3 - 8.5 kb (tl + ql + 1 >= 8192) -> (pairs, true diagonals, wide bands): each band removes the outermost few hundred to two thousand
    diagonals of one or both sides and keeps at least 8192; the read's own diagonal stays inside, so the penalty stays and n_iter falls."""
    spec = ((8400, 6350, 2000), (8300, 30, 2100), (8500, 4000, 1900))
    pairs = []
    for k, (tl, at, m) in enumerate(spec):
        t = random_seq(900 + k, tl)
        pairs.append((t, mutate(t[at:at + m], 950 + k, 0.05)))
    diag = tuple(-at for _, at, _ in spec)
    bands = ((-spec[0][0] + 1500, len(pairs[0][1]) - 600), (-spec[1][0] + 2000, I32_MAX), (-spec[2][0] + 100, len(pairs[2][1]) - 100))
    for (t, q), b in zip(pairs, bands):
        lo, hi = br.clamp_band(len(t), len(q), b)
        assert hi - lo + 1 >= 8192 and hi - lo + 1 < len(t) + len(q) + 1
    return tuple(pairs), diag, bands


WIDE_ENDS = (FREE, FREE, 0, 0)


@functools.lru_cache(maxsize=None)
def wide_want(narrow: bool):
    pairs, diag, bands = wide_cases()
    if narrow:
        bands = tuple((d - 100, d + 100) for d in diag)
    want = tuple(br.wfa_ends_band(t, q, DEFAULT, WIDE_ENDS, b) for (t, q), b in zip(pairs, bands))
    for (t, q), b, w in zip(pairs, bands, want):
        assert w[0] == br.dp_score_band(t, q, DEFAULT, WIDE_ENDS, b), b
    return bands, want


@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
@pytest.mark.parametrize("narrow", [False, True], ids=["wide512", "pm100-256"])
def test_block_follows_the_band(eng, monkeypatch, capfd, narrow, cigar):
    pairs, diag, _ = wide_cases()
    bands, want = wide_want(narrow)
    if not narrow:  # the bands cut something off: cells, not the optimum
        plain = [er.wfa_ends(t, q, DEFAULT, WIDE_ENDS) for t, q in pairs]
        assert all(w[0] == p[0] and w[1] < p[1] for w, p in zip(want, plain)), (want, plain)
    monkeypatch.setenv("MWF_DEBUG", "1")
    opt = opt_of(DEFAULT, cigar)
    capfd.readouterr()
    got = run_pp(eng, pairs, opt, WIDE_ENDS, bands)
    lines = launch_lines(capfd.readouterr().err)
    assert len(lines) == 1 and lines[0][:3] == ("ends-free", 256 if narrow else 512, 3) and lines[0][4:] == (0, 1), lines
    check_ends(got, pairs, opt, WIDE_ENDS, bands, want)


# ---- 3. extension under a band ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ext_cases():
    """-> (pairs, bands, (A, Z)): related prefixes (END), related prefixes with unrelated tails (DROP under Z = 60), an ungapped band {0}, bands that exclude
    diagonal 0 (the stopped record), an indel the band is too narrow for."""
    pairs, bands = [], []
    for k in range(4):   # related from the origin on, a few indels: ends at an edge
        t = random_seq(800 + k, 200 + 30 * k)
        pairs.append((t, mutate(t[:180 + 20 * k], 810 + k, 0.06))), bands.append((-6 - k, 5 + k))
    for k in range(4):   # ... with junk tails: the drop rule ends the pass
        t = random_seq(820 + k, 150)
        pairs.append((t + random_seq(830 + k, 150), mutate(t, 840 + k, 0.04) + random_seq(850 + k, 160))), bands.append((-8, 8 + k))
    for k in range(3):   # d_lo == d_hi == 0: an ungapped extension
        t = random_seq(860 + k, 180)
        q = bytearray(t[:150 + 10 * k])
        for j in range(9, len(q), 23):
            q[j] = ord("G") if q[j] != ord("G") else ord("T")
        pairs.append((t, bytes(q) + (random_seq(865 + k, 90) if k else b""))), bands.append((0, 0))
    t = random_seq(870, 200)
    pairs.append((t, t[:80] + t[92:200])), bands.append((-5, 5))      # a 12-base deletion under a band of +-5: the band decides
    pairs.append((t, t[:80] + t[92:200])), bands.append((-20, 5))     # ... and under one that holds it
    for b in ((1, 40), (-40, -1), (3, 2), (I32_MAX, I32_MAX)):       # diagonal 0 excluded
        pairs.append((t, t[:150])), bands.append(b)
    pairs.append((b"", b"")), bands.append((0, 0))
    pairs.append((b"", b"ACGT")), bands.append((-3, 0))
    return tuple(pairs), tuple(bands), (1, 60)


@functools.lru_cache(maxsize=None)
def ext_want(Z):
    pairs, bands, (A, _) = ext_cases()
    want = tuple(br.wfa_ext_band(t, q, DEFAULT, A, Z, b) for (t, q), b in zip(pairs, bands))
    for (t, q), b, w in zip(pairs, bands, want):
        if w is not None:  # the remembered cell's penalty is the banded DP's for that cell
            assert int(br.dp_matrix_band(t, q, DEFAULT, b)[w.qe][w.te]) == w.s, b
    return want


def check_ext(got, pairs, opt, bands, want, label=""):
    cigar = bool(opt.flag & mw.MWF_F_CIGAR)
    for i, (t, q) in enumerate(pairs):
        w = want[i]
        if w is None:
            assert (got["s"][i], got["it"][i], got["nc"][i], got["rng"][i], got["info"][i]) == (-1, 0, 0, STOPPED, STOPPED), (label, i)
            continue
        assert (got["s"][i], got["it"][i], got["rng"][i][1], got["rng"][i][3]) == (w.s, w.n_iter, w.te, w.qe), (label, i, bands[i])
        assert got["info"][i] == [w.V, w.s_stop, w.why, w.F], (label, i, bands[i])
        assert got["rng"][i][0] == 0 and got["rng"][i][2] == 0
        if cigar:
            xr.check_ext_cigar(mw, opt, t, q, got["cig"][i], got["rng"][i], w.s)
            dlo, dhi = br.cigar_diagonals(got["cig"][i], 0, 0)
            assert bands[i][0] <= dlo and dhi <= bands[i][1], (label, i, "the CIGAR leaves the band")


@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
@pytest.mark.parametrize("Z", [60, -1], ids=["drop60", "nodrop"])
def test_extension_under_a_band(eng, Z, cigar):
    pairs, bands, (A, _) = ext_cases()
    want = ext_want(Z)
    whys = [w.why for w in want if w is not None]
    assert sum(w is None for w in want) == 4
    if Z >= 0:
        assert whys.count(mw.MWF_EXT_DROP) >= 4 and whys.count(mw.MWF_EXT_END) >= 4
        assert want[11].s != want[12].s or want[11].te != want[12].te  # (the narrow band changes that pair's answer)
    opt = opt_of(DEFAULT, cigar)
    check_ext(run_ext(eng, pairs, opt, A, Z, bands), pairs, opt, bands, want, Z)


# ---- 4. infeasible pairs among feasible ones -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
def test_infeasible_pairs_in_a_batch(eng, cigar):
    pairs, ends, bands, kinds = (list(v) for v in geometry_cases())
    want = list(geometry_want("default"))
    keep = list(range(0, len(pairs), 3))
    pairs, ends, bands, want = ([v[i] for i in keep] for v in (pairs, ends, bands, want))
    t, q = pairs[0]
    bad = (((FREE, FREE, 0, 0), (3, 2)), ((FREE, FREE, 0, 0), (len(q) + 1, I32_MAX)), ((0, FREE, 0, 0), (-40, -1)), ((FREE, 0, 0, 0), (len(q) - len(t) + 1, 5)),
           ((0, 0, 0, 0), (I32_MIN, -len(t) - 1)))
    opt = opt_of(DEFAULT, cigar)
    alone = run_pp(eng, pairs, opt, ends, bands)
    check_ends(alone, pairs, opt, ends, bands, want)
    for at, (e, b) in zip((0, 2, 5, 7, len(pairs) + 4), bad):  # the first, some in the middle, the last
        assert not br.feasible(len(t), len(q), e, b)
        pairs.insert(at, (t, q)), ends.insert(at, e), bands.insert(at, b), want.insert(at, None)
    got = run_pp(eng, pairs, opt, ends, bands)
    check_ends(got, pairs, opt, ends, bands, want)
    ok = [i for i, w in enumerate(want) if w is not None]
    for key in ("s", "it", "nc", "cig", "rng"):  # the neighbours: what they give without the infeasible pairs
        if got[key] is not None:
            assert [got[key][i] for i in ok] == alone[key], key
    # ... and a batch of nothing but infeasible pairs
    only = run_pp(eng, [(t, q)] * 3, opt, [e for e, _ in bad[:3]], [b for _, b in bad[:3]])
    check_ends(only, [(t, q)] * 3, opt, [e for e, _ in bad[:3]], [b for _, b in bad[:3]], [None] * 3)


# ---- 5. identity: one allowance set and no band, or an all-covering band, is align_ends / align_ext -----------------------------------------------------

@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
def test_identity_with_the_plain_calls(eng, cigar):
    pairs = list(geometry_cases()[0]) + [(b"", b"ACGT"), (b"", b""), (random_seq(5, 300), random_seq(6, 280))]
    n = len(pairs)
    opt = opt_of(DEFAULT, cigar)
    b = eng.upload(PackedBatch(pairs))
    try:
        for e in ((FREE, FREE, 0, 0), (7, 0, 0, 1000), (0, 0, 0, 0)):
            b.align_ends(opt, *e)
            want = collect(b, cigar)
            for ends, band in ((e, None), ([e] * n, None), (e, [(-len(t), len(q)) for t, q in pairs]), ([e] * n, [(I32_MIN, I32_MAX)] * n)):
                b.align_ends_pp(opt, ends, band)
                assert collect(b, cigar) == want, (e, band is None)
        for A, Z in ((1, -1), (2, 40)):
            b.align_ext(opt, A, Z)
            want = collect(b, cigar, ext=True)
            for band in ([(-len(t), len(q)) for t, q in pairs], [(I32_MIN, I32_MAX)] * n, [(-len(t) - 3, len(q) + 9) for t, q in pairs]):
                b.align_ext(opt, A, Z, band=band)
                assert collect(b, cigar, ext=True) == want, (A, Z)
    finally:
        b.free()


# ---- 6. no leak: after a banded align the other aligns of the same batch are those of a fresh batch -----------------------------------------------------

def test_band_does_not_leak_into_later_aligns(eng):
    pairs, ends, bands, kinds = geometry_cases()
    opt = opt_of(DEFAULT, True)

    def plain(b):
        s, it, nc = b.results()
        b.fetch_cigars()
        return s.tolist(), it.tolist(), [b.cigar(i, int(nc[i])).tolist() for i in range(b.n)]

    def fresh(align, read):
        b = eng.upload(PackedBatch(list(pairs)))
        try:
            align(b)
            return read(b)
        finally:
            b.free()

    want_align = fresh(lambda b: b.align(opt), plain)
    want_ends = fresh(lambda b: b.align_ends(opt, FREE, FREE, 0, 0), lambda b: collect(b, True))
    want_ext = fresh(lambda b: b.align_ext(opt, 1, 50), lambda b: collect(b, True, ext=True))
    b = eng.upload(PackedBatch(list(pairs)))
    try:
        b.align_ends_pp(opt, ends, bands)
        banded = collect(b, True)
        assert banded["s"] != want_ends["s"]
        b.align_ends(opt, FREE, FREE, 0, 0)
        assert collect(b, True) == want_ends
        b.align_ends_pp(opt, ends, bands)
        b.align(opt)
        assert plain(b) == want_align
        with pytest.raises(RuntimeError):
            b.ranges()
        b.align_ext(opt, 1, 50, band=[(0, 0)] * len(pairs))
        b.align_ext(opt, 1, 50)
        assert collect(b, True, ext=True) == want_ext
        b.align_ends_pp(opt, ends, bands)
        assert collect(b, True) == banded
        with pytest.raises(RuntimeError):
            b.ext_info()
    finally:
        b.free()


# ---- 7. the bound: a banded penalty beyond gap(tl) + gap(ql) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
def test_penalty_beyond_the_plain_bound(eng, cigar):
    pairs = [(random_seq(40 + k, L), random_seq(60 + k, L)) for k, L in enumerate((100, 160, 257))]
    bands = [(0, 0), (0, 0), (-1, 1)]
    ends = (0, 0, 0, 0)
    want = [br.wfa_ends_band(t, q, DEFAULT, ends, b) for (t, q), b in zip(pairs, bands)]
    for (t, q), b, w in zip(pairs, bands, want):
        assert w[0] > br.penalty_bound_plain(DEFAULT, len(t), len(q)) and w[0] <= br.penalty_bound_band(DEFAULT, len(t), len(q))
        assert w[0] == br.dp_score_band(t, q, DEFAULT, ends, b)
    opt = opt_of(DEFAULT, cigar)
    got = run_pp(eng, pairs, opt, ends, bands)   # (results() raises for a pair whose status is not 0 or 1)
    check_ends(got, pairs, opt, ends, bands, want)
    assert min(got["s"]) > 0 and eng.stats().n_retries == 0  # (sized by the banded bound: no rows overflow, nothing run again)


# ---- 8. a re-run on fewer workgroups repeats the per-pair parameters ---------------------------------------------------------------------------------------

def test_arena_rerun_keeps_the_bands(eng):
    """The setting of test_ends_gpu.py::test_arena_rerun — eight 2 kb reads at 15 % in 2.6 kb windows, unit penalties, tb_budget_mb = 1: eight slots of 128 KB on
    the first launch, one of 1 MB on the re-run — under per-pair bands of +-250 ... +-285 around each read's diagonal and per-pair allowances.  A row is
    then at most 501 ... 571 columns wide and the penalty is at least the unbanded one, 400 or more: more than 128 KB and less than 571 x 700 = 400 KB per pair."""
    rng = np.random.default_rng(59)
    pairs, bands, ends = [], [], []
    for k in range(8):
        at = int(rng.integers(0, 601))
        t = random_seq(59000 + k, 2600)
        pairs.append((t, mutate(t[at:at + 2000], 59500 + k, 0.15)))
        bands.append((-at - 250 - 5 * k, -at + 250 + 5 * k))
        ends.append((600 + k, 600 - k if k % 2 else FREE, 0, 0))
    opt = opt_of(PEN_UNIT, True)
    want = run_pp(eng, pairs, opt, ends, bands)
    print("penalties:", want["s"], "traceback bytes per pair (n_iter):", want["it"])
    assert all((128 << 10) < n < (400 << 10) for n in want["it"]), want["it"]
    e2 = mw.Engine(0)
    try:
        e2.set("tb_budget_mb", 1)
        got = run_pp(e2, pairs, opt, ends, bands)
        assert e2.stats().n_retries >= len(pairs)
    finally:
        e2.close()
    assert got == want
    ref = [br.wfa_ends_band(t, q, PEN_UNIT, e, b) for (t, q), e, b in zip(pairs, ends, bands)]
    check_ends(got, pairs, opt, ends, bands, ref)
    plain = run_pp(eng, pairs, opt_of(PEN_UNIT, False), ends, None)
    assert got["s"] != plain["s"] or got["it"] != plain["it"]  # (a re-run without the bands would have given these)


# ---- 9. the host-buffer twins ---------------------------------------------------------------------------------------------------------------------------

def test_host_buffer_twins():
    pairs, ends, bands, kinds = geometry_cases()
    pick = [0, 9, 20]
    p3, e3, b3 = [pairs[i] for i in pick], [ends[i] for i in pick], [bands[i] for i in pick]
    want = [geometry_want("default")[i] for i in pick]
    opt = opt_of(DEFAULT, True)
    for i, (s, n_iter, cig, rng) in enumerate(mw.wfa_ends_pp_batch(p3, opt, e3, b3)):
        assert (s, n_iter, rng[1], rng[3]) == want[i], i
        er.check_cigar(mw, opt, p3[i][0], p3[i][1], cig, rng, e3[i], s)
    one = mw.wfa_ends_pp_batch(p3, opt_of(DEFAULT, False), e3[0], None)
    assert [(r[0], r[1]) for r in one] == [er.wfa_ends(t, q, DEFAULT, e3[0])[:2] for t, q in p3]
    xp, xb, (A, Z) = ext_cases()
    pick = [0, 5, 13]
    p3, b3 = [xp[i] for i in pick], [xb[i] for i in pick]
    want = [ext_want(Z)[i] for i in pick]
    for i, (s, n_iter, cig, rng, info) in enumerate(mw.wfa_ext_band_batch(p3, opt, b3, A, Z)):
        w = want[i]
        if w is None:
            assert (s, n_iter, list(rng), list(info)) == (-1, 0, STOPPED, STOPPED)
        else:
            assert (s, n_iter, rng, info) == (w.s, w.n_iter, (0, w.te, 0, w.qe), (w.V, w.s_stop, w.why, w.F)), i


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals(eng):
    import ctypes as C
    pairs = [(b"ACGTACGT", b"ACGT")] * 4
    L = mw.lib()
    opt = opt_of(DEFAULT, False)
    b = eng.upload(PackedBatch(pairs))
    try:
        ends = np.zeros((4, 4), dtype=np.int32)
        for n_ends in (0, 2, 3, 5, -1):
            assert L.mwf_gpu_batch_align_ends_pp(eng.h, b.h, C.byref(opt), ends.ctypes.data, n_ends, None) == -2
            assert "n_ends" in eng.error()
        ends[2, 3] = -1
        ends[3, 0] = -5
        assert L.mwf_gpu_batch_align_ends_pp(eng.h, b.h, C.byref(opt), ends.ctypes.data, 4, None) == -2
        assert "pair 2" in eng.error()
        band = np.zeros((4, 2), dtype=np.int32)
        assert L.mwf_gpu_batch_align_ext_band(eng.h, b.h, C.byref(opt), C.byref(mw.MwfExt(0, -1)), band.ctypes.data) == -2
        assert L.mwf_gpu_batch_align_ends_pp(eng.h, b.h, C.byref(opt_of(DEFAULT, True, step=5)), ends.ctypes.data, 1, None) == -2
        with pytest.raises(ValueError):
            b.align_ends_pp(opt, [[0, 0, 0, 0]] * 3)
        with pytest.raises(ValueError):
            b.align_ends_pp(opt, (0, 0, 0, 0), [(0, 0)] * 3)
        b.align_ends_pp(opt, (FREE, FREE, 0, 0), [(-4, 0)] * 4)   # the batch is unharmed
        assert b.results()[0].tolist() == [0] * 4
    finally:
        b.free()
