"""Per-pair allowances and diagonal bands without a GPU: the ABI is there; the banded restatement of the pass (tests/ends_band_ref.py), the banded DP, the
feasibility rule and the banded penalty bound agree with each other on fuzzed pairs; the pure C++ rules (miniwfa_amd/csrc/mwf_ends_band.h) agree with the
Python ones and run clean under sanitizers in a stand-alone program (tests/host/ends_band_sanitize.cpp; nothing is loaded into python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd import api

import ends_band_ref as br
import ends_ref as er
import ext_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mwf_gpu_batch_align_ends_pp", "mwf_gpu_batch_align_ext_band", "mwf_wfa_ends_pp_batch", "mwf_wfa_ext_band_batch")
DEFAULT = (4, 4, 2, 15, 1)
PENS = (DEFAULT, (4, 6, 3, 26, 1), (2, 3, 1, 9, 1), (3, 0, 2, 6, 1), (1, 1, 1, 1, 1))
FREE = er.FREE
I32_MIN, I32_MAX = -0x80000000, 0x7fffffff
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def related_pair(rng, max_len):
    """(t, q, true diagonal): q is a mutated piece t[a, b), so the alignment of q's first base with t[a] lies on diagonal -a."""
    t = ALPHA[rng.integers(0, 4, int(rng.integers(1, max_len + 1)))]
    a = int(rng.integers(0, len(t)))
    b = int(rng.integers(a + 1, len(t) + 1))
    q = np.array([c if rng.random() > 0.12 else ALPHA[rng.integers(0, 4)] for c in t[a:b] if rng.random() > 0.04], dtype=np.uint8)
    return t.tobytes(), q.tobytes(), -a


def unrelated_pair(rng, lo, hi):
    return (ALPHA[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))].tobytes(), ALPHA[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))].tobytes())


def feasible_band(rng, tl, ql, ends, around, max_w):
    """A band of random width around diagonal `around`, widened until the rule admits it: every drawn band is feasible by construction."""
    lo = around - int(rng.integers(0, max_w + 1))
    hi = around + int(rng.integers(0, max_w + 1))
    t_beg, t_end, q_beg, q_end = br.clamp_ends(tl, ql, ends)
    # reach the origin diagonals [-t_beg, q_beg] and the end diagonals [ql - tl - q_end, ql - tl + t_end]
    lo = min(lo, q_beg, ql - tl + t_end)
    hi = max(hi, -t_beg, ql - tl - q_end)
    return lo, hi


def test_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in api.ABI_SYMBOLS and hasattr(L, name), name
    assert "mwf_band_t" in header
    assert C.sizeof(mw.MwfBand) == 8
    assert [f for f, _ in mw.MwfBand._fields_] == ["d_lo", "d_hi"]
    assert hasattr(mw.Batch, "align_ends_pp")
    import inspect
    assert list(inspect.signature(mw.Batch.align_ext).parameters) == ["self", "opt", "match", "zdrop", "band"]
    assert inspect.signature(mw.Batch.align_ext).parameters["band"].default is None
    assert list(inspect.signature(mw.Batch.align_ends).parameters) == ["self", "opt", "t_beg", "t_end", "q_beg", "q_end"]
    for name in ("wfa_ends_pp_batch", "wfa_ext_band_batch"):
        assert hasattr(mw, name), name


def test_restatement_dp_rule_and_bound_agree_on_feasible_bands():
    """Bands drawn around the pair's true diagonal, feasible by construction: no case is skipped, and every one is checked four ways."""
    rng = np.random.default_rng(20241021)
    allow = (0, 1, 7, FREE)
    n_checked = n_cut = 0
    for k in range(240):
        t, q, d0 = related_pair(rng, 48)
        tl, ql = len(t), len(q)
        pen = PENS[k % len(PENS)]
        ends = tuple(int(allow[v]) for v in rng.integers(0, 4, 4))
        band = feasible_band(rng, tl, ql, ends, d0, 6)
        assert br.feasible(tl, ql, ends, band), (k, ends, band)
        want = br.dp_score_band(t, q, pen, ends, band)
        assert want < er.INF, (k, "the rule admits the band, the DP finds nothing", ends, band)
        got = br.wfa_ends_band(t, q, pen, ends, band)
        assert got is not None
        s, n_iter, te, qe = got
        assert s == want, (k, pen, ends, band, t, q)
        assert s <= br.penalty_bound_band(pen, tl, ql), (k, s)
        assert want >= er.dp_score(t, q, pen, ends)  # a band can only cost
        n_cut += want > er.dp_score(t, q, pen, ends)
        assert te == tl or qe == ql
        assert tl - te <= ends[1] and ql - qe <= ends[3]
        lo, hi = br.clamp_band(tl, ql, band)
        assert lo <= qe - te <= hi
        n_checked += 1
    assert n_checked == 240
    assert n_cut >= 20, n_cut  # (the bands bite)


INFEASIBLE = (
    # (t, q, allowances, band, what)
    (b"ACGTACGTAC", b"ACGTAC", (0, FREE, 0, 0), (3, 2), "d_lo > d_hi"),
    (b"ACGTACGTAC", b"ACGTAC", (FREE, FREE, FREE, FREE), (I32_MAX, I32_MIN), "d_lo > d_hi at the limits"),
    (b"ACGTACGTAC", b"ACGTAC", (FREE, FREE, 0, 0), (7, 20), "empty after the clamp: above ql"),
    (b"ACGTACGTAC", b"ACGTAC", (FREE, FREE, 0, 0), (-40, -11), "empty after the clamp: below -tl"),
    (b"ACGTACGTAC", b"ACGTAC", (0, FREE, 0, 0), (-9, -1), "misses the origin set {0}"),
    (b"ACGTACGTAC", b"ACGTAC", (2, FREE, 0, 0), (-9, -3), "misses the origin set [-2, 0]"),
    (b"ACGTACGTAC", b"ACGTAC", (0, FREE, 2, 0), (3, 6), "misses the origin set [0, 2]"),
    (b"ACGTACGTAC", b"ACGTAC", (FREE, 0, 0, 0), (-3, 6), "misses the end set {-4}"),
    (b"ACGTACGTAC", b"ACGTAC", (FREE, 1, 0, 0), (-2, 6), "misses the end set [-4, -3]"),
    (b"ACGTAC", b"ACGTACGTAC", (0, 0, FREE, 2), (-6, 1), "misses the end set [2, 4]"),
    (b"", b"", (0, 0, 0, 0), (1, 5), "empty sequences, band above 0"),
    (b"", b"", (FREE, FREE, FREE, FREE), (-5, -1), "empty sequences, band below 0"),
    (b"", b"ACGT", (0, 0, 0, 0), (0, 3), "empty target: the end diagonal 4 is outside"),
    (b"ACGT", b"", (0, 0, 0, 0), (-3, 0), "empty query: the end diagonal -4 is outside"),
)


@pytest.mark.parametrize("case", INFEASIBLE, ids=[c[4] for c in INFEASIBLE])
def test_infeasible_bands(case):
    t, q, ends, band, _ = case
    assert not br.feasible(len(t), len(q), ends, band)
    assert br.dp_score_band(t, q, DEFAULT, ends, band) >= er.INF
    assert br.wfa_ends_band(t, q, DEFAULT, ends, band) is None


def test_rule_agrees_with_the_dp_on_random_bands():
    """Uniformly random bands, most of them infeasible: the rule and the DP say the same."""
    rng = np.random.default_rng(77)
    allow = (0, 1, 5, FREE)
    n_feasible = 0
    for k in range(300):
        t, q = unrelated_pair(rng, 0, 14)
        tl, ql = len(t), len(q)
        ends = tuple(int(allow[v]) for v in rng.integers(0, 4, 4))
        band = (int(rng.integers(-tl - 3, ql + 4)), int(rng.integers(-tl - 3, ql + 4)))
        ok = br.feasible(tl, ql, ends, band)
        assert ok == (br.dp_score_band(t, q, DEFAULT, ends, band) < er.INF), (k, t, q, ends, band)
        n_feasible += ok
    assert 30 <= n_feasible <= 270, n_feasible


def test_narrow_bands_past_penalties_256_and_512():
    """Unrelated sequences of 120 - 160 bases under the default penalties and a narrow band: the pass crosses the shrink at 256 (and some at 512) inside
    the band and still finds the DP's penalty, beyond the plain bound gap(tl) + gap(ql) where the band forces it there."""
    rng = np.random.default_rng(512)
    past256 = past512 = beyond_plain = 0
    for k in range(10):
        if k < 5:
            t, q = unrelated_pair(rng, 120, 160)
        else:  # (three mismatches in four at x = 4: about 3 L, past 512 from L = 180 on under a band of one or three diagonals)
            L = 180 + 5 * (k - 5)
            t, q = unrelated_pair(rng, L, L)
        tl, ql = len(t), len(q)
        w = (0, 1, 2, 4, 0, 0, 1, 0, 1, 0)[k]
        band = (min(0, ql - tl) - w, max(0, ql - tl) + w)
        ends = (0, 0, 0, 0)
        assert br.feasible(tl, ql, ends, band)
        shrinks = []
        s, n_iter, te, qe = br.wfa_ends_band(t, q, DEFAULT, ends, band, shrinks=shrinks)
        assert s == br.dp_score_band(t, q, DEFAULT, ends, band), (k, band)
        assert s <= br.penalty_bound_band(DEFAULT, tl, ql)
        assert len(shrinks) == s // 256
        past256 += s > 256
        past512 += s > 512
        beyond_plain += s > br.penalty_bound_plain(DEFAULT, tl, ql)
    assert past256 >= 8 and past512 >= 3 and beyond_plain >= 1, (past256, past512, beyond_plain)


def test_all_covering_band_is_the_unbanded_pass():
    rng = np.random.default_rng(99)
    allow = (0, 1, 7, FREE)
    for k in range(60):
        t, q, _ = related_pair(rng, 60)
        tl, ql = len(t), len(q)
        pen = PENS[k % len(PENS)]
        ends = tuple(int(allow[v]) for v in rng.integers(0, 4, 4))
        for band in ((-tl, ql), (I32_MIN, I32_MAX), None):
            assert br.wfa_ends_band(t, q, pen, ends, band) == er.wfa_ends(t, q, pen, ends), (k, band)
        A, Z = (1, -1) if k % 2 else (2, 30)
        assert br.wfa_ext_band(t, q, pen, A, Z, (-tl - 5, ql + 5)) == xr.wfa_ext(t, q, pen, A, Z), k
    # ... and past a shrink
    t, q = unrelated_pair(rng, 150, 160)
    assert br.wfa_ends_band(t, q, DEFAULT, (0, 0, 0, 0), (-len(t), len(q))) == er.wfa_ends(t, q, DEFAULT, (0, 0, 0, 0))


def test_banded_extension_against_the_banded_matrix():
    """Z = -1: the pass ends at the cheapest in-band cell of the far edges, and its V is the best among the in-band cells no dearer than that."""
    rng = np.random.default_rng(4242)
    for k in range(60):
        t, q, _ = related_pair(rng, 50)
        q = t[:3] + q  # (an extension starts at the origin)
        tl, ql = len(t), len(q)
        pen = PENS[k % len(PENS)]
        band = (-int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        got = br.wfa_ext_band(t, q, pen, 1, -1, band)
        D = br.dp_matrix_band(t, q, pen, band)
        s_end = int(min(D[-1].min(), D[:, -1].min()))
        assert s_end < xr.DP_INF
        ij = np.add.outer(np.arange(ql + 1, dtype=np.int64), np.arange(tl + 1, dtype=np.int64))
        V = int(np.where(D <= s_end, ij - 2 * D, -1).max())
        assert (got.s_stop, got.V, got.why) == (s_end, V, 0), (k, band)
        assert int(D[got.qe][got.te]) == got.s
        assert band[0] <= got.qe - got.te <= band[1]
    assert br.wfa_ext_band(b"ACGT", b"ACGT", DEFAULT, 1, -1, (1, 3)) is None
    assert br.wfa_ext_band(b"ACGT", b"ACGT", DEFAULT, 1, -1, (-3, -1)) is None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("ends_band") / "ends_band_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "miniwfa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ends_band_sanitize.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(out)


def test_pure_rules_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ends_band_sanitize OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_cpp_rules_equal_the_python_rules(exe):
    rng = np.random.default_rng(5)
    allow = (0, 1, 9, FREE)
    cases = []
    for k in range(400):
        tl, ql = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        ends = tuple(int(allow[v]) for v in rng.integers(0, 4, 4))
        band = (int(rng.integers(-tl - 4, ql + 5)), int(rng.integers(-tl - 4, ql + 5))) if k % 7 else (I32_MIN, I32_MAX)
        cases.append((tl, ql, ends, band, PENS[k % len(PENS)]))
    lines = "".join(f"{tl} {ql} {e[0]} {e[1]} {e[2]} {e[3]} {b[0]} {b[1]} {p[0]} {p[1]} {p[2]} {p[3]} {p[4]} 0\n" for tl, ql, e, b, p in cases)
    r = subprocess.run([exe, "rule"], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases)
    for (tl, ql, e, b, p), (ok, width, bound) in zip(cases, out):
        lo, hi = br.clamp_band(tl, ql, b)
        assert (bool(ok), width, bound) == (br.feasible(tl, ql, e, b), max(0, hi - lo + 1), br.penalty_bound_band(p, tl, ql)), (tl, ql, e, b, p)
