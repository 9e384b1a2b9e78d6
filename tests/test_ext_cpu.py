"""Extension alignment without a GPU: the ABI and the kernels are there, and the yardsticks of tests/ext_ref.py agree with each other on the shared case
list (tests/ext_cases.py) and on fuzzed pairs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import miniwfa_amd as mw
from miniwfa_amd import api

import ext_cases as xc
import ext_ref as xr
from test_ends_cpu import PENS, rand_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENDS_OBJ = os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_ends.hip.o")
ENDS_KERNELS = {(b, e) for b in (256, 512) for e in ("true", "false")}  # wfa_ends_kernel<T, EXT>: what the object must hold (tests/ends_matrix.py has an entry for each)
NEW_SYMBOLS = ("mwf_gpu_batch_align_ext", "mwf_gpu_batch_ext_info", "mwf_gpu_batch_dev_ext_info", "mwf_wfa_ext", "mwf_wfa_ext_batch")


def test_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in api.ABI_SYMBOLS and hasattr(L, name), name
    assert "mwf_ext_t" in header and "MWF_EXT_END" in header and "MWF_EXT_DROP" in header
    assert C.sizeof(mw.MwfExt) == 8
    assert [f for f, _ in mw.MwfExt._fields_] == ["match", "zdrop"]
    assert (mw.MWF_EXT_END, mw.MWF_EXT_DROP) == (0, 1)
    for name in ("align_ext", "ext_info", "dev_ext_info_ptr"):
        assert hasattr(mw.Batch, name), name
    assert callable(mw.wfa_ext) and callable(mw.wfa_ext_batch)


def test_object_holds_the_ext_kernels():
    """The gfx950 code object of mwf_ends.hip holds the kernel in both forms at both workgroup sizes."""
    mw.lib()
    assert os.path.exists(ENDS_OBJ), "no " + os.path.relpath(ENDS_OBJ, ROOT) + " (the library was not built from this tree)"
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    tools = {t: (os.path.join(llvm, t) if os.path.exists(os.path.join(llvm, t)) else shutil.which(t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    assert all(tools.values()) and cxxfilt, "llvm-objcopy, clang-offload-bundler, llvm-readelf or c++filt not found"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fb, ENDS_OBJ, os.path.join(d, "copy.o")], check=True, capture_output=True)
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co],
                       check=True, capture_output=True)
        syms = subprocess.run([tools["llvm-readelf"], "-sW", co], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run([cxxfilt], input=syms, check=True, capture_output=True, text=True).stdout
    got = {(int(m.group(1)), m.group(2)) for ln in dem.splitlines() for m in [re.search(r"\bFUNC\b.*wfa_ends_kernel<(\d+), (true|false)>", ln)] if m}
    assert got == ENDS_KERNELS, got


def check_against_dp(t, q, pen, A, r, what):
    V, s_end, D = xr.dp_best(t, q, pen, A)
    assert (r.V, r.s_stop, r.why) == (V, s_end, 0), (what, tuple(r), V, s_end)
    assert int(D[r.qe][r.te]) == r.s and A * (r.te + r.qe) - 2 * r.s == r.V, (what, tuple(r))


def test_every_case_is_in_the_restatements_domain():
    """Every case of the list ends below penalty 256, before the first shrink (the restatement itself goes on beyond it: tests/test_ends_matrix_cpu.py)."""
    n = 0
    for case, pen in xc.runs():
        for (t, q), r in zip(case.pairs, xc.want(case, pen)):
            assert 0 <= r.s <= r.s_stop < 256 and r.why in (0, 1) and (case.Z >= 0 or r.why == 0), (case.name, pen)
            assert r.V == case.A * (r.te + r.qe) - 2 * r.s and 0 <= r.V <= case.A * r.F, (case.name, pen)
            n += 1
    assert n >= 150


def test_restatement_equals_dp_on_the_list():
    n = 0
    for case, pen in xc.runs():
        if case.Z != -1:
            continue
        for (t, q), r in zip(case.pairs, xc.want(case, pen)):
            check_against_dp(t, q, pen, case.A, r, (case.name, pen))
            n += 1
    assert n >= 30


def test_restatement_equals_dp_on_fuzzed_pairs():
    rng = np.random.default_rng(20250314)
    n_drop = n_inner = n_far = 0
    for k in range(300):
        t, q = rand_pair(rng, 60, two_letter=k % 2 == 1)
        pen = PENS[k % len(PENS)]
        A = 1 + k % 3 % 2  # 1, 2, 1, 1, 2, 1, ...
        free = xr.wfa_ext(t, q, pen, A, -1)
        check_against_dp(t, q, pen, A, free, (k, pen, A, t, q))
        n_inner += free.s < free.s_stop
        # A drop no pass can reach is no drop rule.  B <= A F at every penalty, so the drop B - (A F - 2 s) is at most 2 s <= 2 s_end: Z >= 2 s_end is never
        # exceeded.  Z = A (tl + ql) is such a Z wherever 2 s_end <= A (tl + ql) — every pair whose edits cost less than its matches earn, not an
        # unrelated one, whose pass the rule does end early under that Z — and is the Z used there.
        Z_far = max(A * (len(t) + len(q)), 2 * free.s_stop)
        n_far += Z_far == A * (len(t) + len(q))
        assert xr.wfa_ext(t, q, pen, A, Z_far) == free, k
        # a drop rule only ever ends the pass earlier: what it found is what the free pass had found by then
        for Z in (0, 5, 20):
            r = xr.wfa_ext(t, q, pen, A, Z)
            assert r.V <= free.V and r.s_stop <= free.s_stop and r.n_iter <= free.n_iter and r.F <= free.F, (k, Z)
            assert (r.why == 1) == (r.s_stop < free.s_stop), (k, Z)
            n_drop += r.why
    print("drops", n_drop, "answers before the end", n_inner, "Z = A (tl + ql)", n_far)
    assert n_drop >= 100 and n_inner >= 50 and n_far >= 100, (n_drop, n_inner, n_far)


def test_list_keeps_its_promises():
    by_name = {c.name: c for c in xc.cases()}
    want = lambda name, pen=xc.PEN_A: xc.want(by_name[name], pen)  # noqa: E731
    # (a) - (e)
    assert tuple(want("a-identical")[0])[:8] == (0, 0, 200, 200, 400, 0, 0, 400)
    assert all(tuple(r)[:8] == (0, 0, 0, 0, 0, 0, 0, 0) for r in want("b-empty"))
    r = want("c-unrelated-drop")[0]
    assert (r.te, r.qe, r.V, r.why) == (0, 0, 0, 1)
    r = want("c-unrelated-end")[0]
    assert (r.te, r.qe, r.V, r.why) == (0, 0, 0, 0)
    for name in ("d-related-A1", "d-related-A2"):
        r = want(name)[0]
        assert r.s == r.s_stop and r.why == 0
    t, q = by_name["e-long-target"].pairs[0]
    r = want("e-long-target")[0]
    assert len(t) == 450 and r.qe == len(q) and r.te < len(t) - 100
    # (f): the figures of the specification's prototype
    assert [(r.s, r.s_stop, r.why) for name in ("f-junk40-end", "f-junk200-z50", "f-junk200-z100") for r in want(name)] == [(78, 131, 0), (78, 123, 1), (78, 170, 1)]
    assert want("f-junk40-end")[0].s_stop >= 130
    # (g): the 512-thread form
    for name, s_stop in (("g-4200", 156), ("g-4200-junk300-z80", 226)):
        t, q = by_name[name].pairs[0]
        assert len(t) + len(q) + 1 >= 8192 and want(name)[0].s_stop == s_stop
    # (h): both kinds of tie, at least twice each
    assert sum(want(c.name)[0].tie_cols >= 2 for c in xc.cases() if c.name.startswith("h-tie-cols")) >= 2
    assert sum(want(c.name)[0].tie_later >= 1 for c in xc.cases() if c.name.startswith("h-tie-later")) >= 2
    for c in xc.cases():
        if c.name.startswith("h-"):
            assert all(20 <= len(t) <= 120 for t, _ in c.pairs)
    # (i)
    for name in ("i-mixed-z40", "i-mixed-A2-z25"):
        c = by_name[name]
        assert len(c.pairs) == 64 and max(max(len(t), len(q)) for t, q in c.pairs) <= 600
        w = xc.want(c, c.pens[0])
        assert 10 <= sum(r.why for r in w) <= 54 and any(r.te == 0 and r.qe == 0 for r in w) and any(0 < r.s < r.s_stop for r in w)


def test_checker_rejects_wrong_alignments():
    opt = mw.opt_init(flag=mw.MWF_F_CIGAR)
    t, q = b"ACGTACGTAC" + b"TTTT", b"ACGTCCGTAC" + b"GGGGGG"
    words, rng, s = [4 << 4 | 7, 1 << 4 | 8, 5 << 4 | 7], (0, 10, 0, 10), 4
    xr.check_ext_cigar(mw, opt, t, q, words, rng, s)
    xr.check_ext_cigar(mw, opt, t, q, [], (0, 0, 0, 0), 0)
    for bad in (dict(rng=(1, 10, 0, 10)),                      # does not begin at the origin
                dict(rng=(0, 15, 0, 10)),                      # beyond the target
                dict(words=[10 << 4 | 7]),                     # = over unequal bases
                dict(words=[4 << 4 | 7, 1 << 4 | 8, 4 << 4 | 7]),  # does not consume the ranges
                dict(words=[4 << 4 | 7, 1 << 4 | 8, 2 << 4 | 7, 3 << 4 | 7]),  # unmerged runs
                dict(s=3)):                                    # another score
        kw = dict(words=words, rng=rng, s=s)
        kw.update(bad)
        try:
            xr.check_ext_cigar(mw, opt, t, q, kw["words"], kw["rng"], kw["s"])
        except AssertionError:
            continue
        raise AssertionError(f"the checker accepted {bad}")
