"""CPU-side checks of the "alpha16" tunable (include/miniwfa.h): the host twin mwf_alphabet_class16 against the rule restated in Python (tests/alpha16_cases.py), the
premise — a class-3 pair and its image under the map have the same s, n_iter and CIGAR — on the oracle, the exports, the nine gfx950 kernels of mwf_band2_nib.hip.o, the
twin under AddressSanitizer / UBSan in a stand-alone program, and a self-check of every GPU case from the oracle alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd import api
from miniwfa_amd import build as mwbuild
import alpha16_cases as c16
import band_matrix as bm
import band_tab_cases as bt
from conftest import ROOT

INPUTS = c16.cpu_inputs()


@pytest.mark.parametrize("name", [n for n, _, _ in INPUTS])
def test_host_twin_equals_the_rule(name):
    t, q = next((t, q) for n, t, q in INPUTS if n == name)
    cls, m = mw.alphabet_class16(t, q)
    assert (cls, m) == c16.py_class16(t, q), name
    syms = sorted(set(t) | set(q))
    if cls == 3:
        # a bijection of the bytes that occur onto the codes 0 ... n - 1 under the tag, in ascending byte order
        assert 5 <= len(syms) <= 16 and [m[b] for b in syms] == [c16.TAG | k for k in range(len(syms))] and sum(1 for x in m if x) == len(syms)
    # classes 0 and 1: class and map of mwf_alphabet_class; 2 and 3 are its class 2
    cls4, m4 = mw.alphabet_class(t, q)
    assert cls4 == (2 if cls == 3 else cls)
    if cls <= 1:
        assert m == m4
    if cls in (0, 2):
        assert m == bytes(256)


def test_the_named_cases_have_the_classes_their_names_say():
    want = {"plain": 0, "lower": 1, "acgtn": 3, "mixed8": 3, "sym16": 3, "sym17": 2, "n_last_q": 3, "bytes_00_ff": 3,
            "exactly4": 1, "exactly5": 3, "exactly16": 3, "exactly17": 2, "split16": 3, "both_empty": 0, "empty_t": 3, "empty_q": 3}
    for name, t, q in INPUTS:
        case = name.rsplit("-", 1)[0] if name.rsplit("-", 1)[-1].isdigit() else name
        assert mw.alphabet_class16(t, q)[0] == want[case], name
    n16 = {name: len(set(t) | set(q)) for name, t, q in INPUTS}
    assert n16["exactly4"] == 4 and n16["exactly5"] == 5 and n16["exactly16"] == 16 and n16["exactly17"] == 17 and n16["sym16-450"] == 16 and n16["sym17-450"] == 17
    t, q = next((t, q) for n, t, q in INPUTS if n == "n_last_q-450")
    assert q.index(b"N") == len(q) - 1 and b"N" not in t
    t, q = next((t, q) for n, t, q in INPUTS if n == "bytes_00_ff-450")
    m = mw.alphabet_class16(t, q)[1]
    assert 0 in t and 255 in t and m[0] == c16.TAG and m[255] == c16.TAG | (len(set(t) | set(q)) - 1)
    # the GPU batch: every class, every case at least four times, every length three times, odd offsets, three queries on one target range
    pk, names = c16.gpu_batch_a()
    assert pk.n == len(names) == 42
    cls = [mw.alphabet_class16(*pk.pair(i))[0] for i in range(pk.n)]
    assert {0, 1, 2, 3} <= set(cls) and cls.count(3) >= 15
    for case in c16.CASES:
        assert sum(n.startswith(case + "-") for n in names) >= 4, case
    for length in c16.LENGTHS:
        assert sum(n.endswith(f"-{length}") for n in names) >= 3, length
    assert sum(int(o) & 1 for o in pk.t_off) >= 10 and len({int(o) for o in pk.t_off[-3:]}) == 1
    for which, block in ((c16.gpu_batch_short, 64), (c16.gpu_batch_a, 256), (c16.gpu_batch_long, 1024)):
        pk, names = which()
        longest = max(int(pk.tl[i]) + int(pk.ql[i]) for i in range(pk.n))
        assert (64 if longest <= 2048 else 256 if longest <= 65536 else 1024) == block   # mwf_alphabet.hip alphabet_block
        cls = [mw.alphabet_class16(*pk.pair(i))[0] for i in range(pk.n)]
        assert {2, 3} <= set(cls) and any(n.startswith("n_last_q") for n in names), which.__name__


@pytest.mark.parametrize("pen", ["default", "a22"])
def test_premise_image_aligns_like_the_original(oracle, pen):
    """(s, n_iter, CIGAR) of the oracle on a class-3 pair equal those on its image under the map: six pairs of 150-900 bases, under the default penalties and under
    the -a-like set (o2, e2) = (4, 2)."""
    from oracle.pyoracle import make_opt
    kw = {} if pen == "default" else dict(o2=4, e2=2)
    for k, (case, length) in enumerate([("acgtn", 150), ("mixed8", 300), ("sym16", 450), ("bytes_00_ff", 600), ("n_last_q", 750), ("sym16", 900)]):
        t, q = c16.recode(case, *c16.base_pair(9700 + k, length, 0.06), 9800 + k)
        cls, m = mw.alphabet_class16(t, q)
        assert cls == 3
        ti, qi = t.translate(m), q.translate(m)
        assert all(b >> 4 == c16.TAG >> 4 for b in ti + qi)
        for flag in (0, 1):
            o = make_opt(flag=flag, **kw)
            assert oracle.align(ti, qi, o) == oracle.align(t, q, o), (case, length, flag)


def test_symbols_exported_and_declared():
    L = mw.lib()
    text = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    for name in ("mwf_alphabet_class16", "mwf_gpu_batch_alphabet"):
        assert hasattr(L, name) and name in api.ABI_SYMBOLS and re.search(r"\b" + name + r"\s*\(", text), name
    assert '"alpha16"' in text and "MWF_ALPHA16_TAG 0x40" in text and "MWF_ALPHA16=1" in text
    assert "mwf_band2_nib.hip" in mwbuild.SOURCES and os.path.join(mwbuild.CSRC, "mwf_band2_kernel.h") in mwbuild.HEADERS
    # the files kernel_fingerprint hashes for the 4-bit kernel: the shared header (the template) and the unit that instantiates it
    assert mwbuild.KERNEL_FILES["wfa_band2_nib_kernel"] == "mwf_band2_kernel.h" and "mwf_band2_nib.hip" in mwbuild.KERNEL_HEADERS["mwf_band2_kernel.h"]


def test_new_object_holds_exactly_the_nine_kernels():
    """mwf_band2_nib.hip.o: 512 x 3, 512 x 4 and the span geometry, (2,1), 2-bit flag set (the S2 paths are what the macro turns into 4 bits), never BI4, each with
    traceback (unfolded), score-only folded and score-only unfolded — and no kernel of another name."""
    mw.lib()
    nib, others = c16.nib_object_kernels()
    want = {bm.Inst(T, K, 2, 1, tb, 1, 0, fold) for T, K in ((512, 3), (512, 4), (1024, 5)) for tb, fold in ((1, 0), (0, 1), (0, 0))}
    assert nib == want, (sorted(nib - want), sorted(want - nib))
    assert others == set(), others


def test_host_twin_under_sanitizers(tmp_path):
    """tests/host/alphabet_class16_sanitize.cpp + csrc/mwf_dbg.cpp built with -fsanitize=address,undefined: host code only, nothing loaded into python.  The sequences
    are heap blocks of exactly their length, flush against the end of their allocations."""
    exe = tmp_path / "alphabet_class16_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "alphabet_class16_sanitize.cpp"),
           os.path.join(ROOT, "miniwfa_amd", "csrc", "mwf_dbg.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "alphabet_class16_sanitize OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


# ---- self-check of the GPU edge cases: sized from the oracle alone ------------------------------------------------------------------------------------------
def test_edge_cases_are_what_their_names_say(oracle):
    """Every pair of group (d) is class 3, 300 to 3 300 bases long; every run it is named for starts behind a mismatch on the oracle's alignment path, is exactly as long
    as it says and ends where it says; the run lengths cover FULL, the end of the four per-lane trips and the whole-wave trips."""
    cases = c16.edge()
    exp = c16.expected(oracle, "edge", [(t, q) for _, t, q, _ in cases])
    seen, ends = set(), set()
    for (name, t, q, runs), (s, it, cig) in zip(cases, exp):
        assert mw.alphabet_class16(t, q)[0] == 3, name
        assert 300 <= len(t) <= 3300 and 300 <= len(q) <= 3300, (name, len(t), len(q))
        cells = {(i, j) for i, j, _ in bt.path_cells(t, q, cig)} if runs else set()
        for r in runs:
            assert c16.lce(t, q, r.ti, r.qi) == r.n, (name, r)
            if r.ti > 0:
                assert t[r.ti - 1] != q[r.qi - 1] and (r.ti - 1, r.qi - 1) in cells, (name, r)
            at_t, at_q = r.ti + r.n == len(t), r.qi + r.n == len(q)
            assert (at_t, at_q) == {"room": (False, False), "target": (True, False), "query": (False, True), "both": (True, True)}[r.end], (name, r)
            seen.add(r.n), ends.add(r.end)
    assert {0, 1, 7, 8, 9, 15, 16, 17, 39, 40, 41, 511, 512, 513, 1030} <= seen and ends == {"room", "target", "query", "both"}
    assert c16.WAVE_WALK_FROM == 40 and c16.FULL == 8
    names = {n for n, _, _, _ in cases}
    for rt in (0, 1, 7):
        for rq in (0, 1, 7):
            t, q = next((t, q) for n, t, q, _ in cases if n == f"len8-{rt}-{rq}")
            assert (len(t) % 8, len(q) % 8) == (rt, rq)
    # codes 0 and 15 side by side: in the image of the pair the nibbles 0x0 and 0xf are neighbours hundreds of times
    t, q = next((t, q) for n, t, q, _ in cases if n == "codes-0-15")
    m = mw.alphabet_class16(t, q)[1]
    im = t.translate(m)
    assert len(set(t) | set(q)) == 16 and sum(1 for a, b in zip(im, im[1:]) if {a & 15, b & 15} == {0, 15}) > 200
    # the back-match case: '=' words of 9 or more bases that start at a target position off a dword boundary of the copy
    k = [n for n, _, _, _ in cases].index("backmatch")
    t, q = cases[k][1], cases[k][2]
    pos, long_eq = 0, 0
    for w in exp[k][2]:
        n, op = int(w) >> 4, api.CIGAR_CHARS[int(w) & 0xf]
        long_eq += op == "=" and n >= 9 and pos % 8 != 0
        pos += n if op in "=XMD" else 0
    assert long_eq >= 6 and {api.CIGAR_CHARS[int(w) & 0xf] for w in exp[k][2]} >= {"=", "X", "I", "D"}
    assert "identical" in names and exp[[n for n, _, _, _ in cases].index("identical")][0] == 0


@pytest.mark.parametrize("geom", list(c16.GEOMS))
def test_no_edge_case_is_handed_back(oracle, geom):
    """Condition of the issue: no pair of the edge group is one the geometry hands back — the host admits it by its lengths, and its oracle band trace fits the
    geometry's chunks, forecasts and 16-bit range, folded and unfolded (band_matrix.fits / host_admits)."""
    from oracle.pyoracle import make_opt
    g = c16.GEOMS[geom]
    o = make_opt(**c16.DEFAULT)
    for name, t, q, _ in c16.edge():
        assert bm.host_admits(g, c16.DEFAULT, len(t), len(q)), (geom, name)
        lohi, far = oracle.band_trace_far(t, q, o, cap=bm.penalty_bound(c16.DEFAULT, len(t), len(q)) + 2)
        for fold in (0, 1):
            assert bm.fits(g, fold, c16.DEFAULT, lohi, far, len(t), len(q)) == (True, True), (geom, name, fold)


def test_routing_batches_fit_their_geometries(oracle):
    """GPU test (c): the 64 x 3 kb pairs fit 512 x 3 (and so the 768 x 2 they take with the tunable off: the same 24 chunks), the 4 x 16 kb pairs are admitted to
    the biased 512-thread class by their lengths (host_class 14) and fit the span geometry the 4-bit form runs them on; all are class 3."""
    from oracle.pyoracle import make_opt
    o = make_opt(**c16.DEFAULT)
    small, long_ = c16.routing_pairs(64, 3000, 0.05, 71000), c16.routing_pairs(4, 16000, 0.03, 72000)
    for pairs, g, cls in ((small, c16.G3, (1, 2)), (long_, c16.GSPAN, (14,))):
        for t, q in pairs[:8] if pairs is small else pairs:
            assert mw.alphabet_class16(t, q)[0] == 3 and mw.alphabet_class(t, q)[0] == 2
            assert bm.host_class(c16.DEFAULT, len(t), len(q)) in cls
            lohi, far = oracle.band_trace_far(t, q, o, cap=bm.penalty_bound(c16.DEFAULT, len(t), len(q)) + 2)
            assert bm.fits(g, 1, c16.DEFAULT, lohi, far, len(t), len(q)) == (True, True)
