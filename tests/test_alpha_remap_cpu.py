"""CPU-side checks of the "alpha_remap" tunable (include/miniwfa.h): the host twin mwf_alphabet_class against the rule restated in Python
(tests/alpha_remap_cases.py), the premise — a class-1 pair and its image under the map have the same s, n_iter and CIGAR — on the oracle, the
export, the gfx950 kernels of the new unit's object, and the twin under AddressSanitizer / UBSan in a stand-alone program."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import miniwfa_amd as mw
from miniwfa_amd import api
from miniwfa_amd import build as mwbuild
import alpha_remap_cases as ac
from conftest import ROOT

INPUTS = ac.cpu_inputs()
ALPHA_OBJ = os.path.join(os.path.dirname(mwbuild.LIB), "build", "mwf_alphabet.hip.o")


@pytest.mark.parametrize("name", [n for n, _, _ in INPUTS])
def test_host_twin_equals_the_rule(name):
    t, q = next((t, q) for n, t, q in INPUTS if n == name)
    cls, m = mw.alphabet_class(t, q)
    assert (cls, m) == ac.py_class(t, q), name
    if cls == 1:
        # a bijection of the bytes that occur onto a prefix of ACGT, in ascending byte order
        syms = sorted(set(t) | set(q))
        assert [m[b] for b in syms] == list(b"ACGT"[:len(syms)]) and sum(1 for x in m if x) == len(syms)
    else:
        assert m == bytes(256)


def test_the_named_cases_have_the_classes_their_names_say():
    want = {"plain": 0, "lower": 1, "acgu": 1, "one": 1, "two": 1, "four_bytes": 1, "five": 2, "fifth_last_q": 2, "fifth_in_t": 2}
    for name, t, q in INPUTS:
        case = name.rsplit("-", 1)[0]
        if case in want:
            assert mw.alphabet_class(t, q)[0] == want[case], name
    assert mw.alphabet_class(b"", b"")[0] == 0 and mw.alphabet_class(b"", b"acgtacgt")[0] == 1 and mw.alphabet_class(b"ACGU", b"")[0] == 1
    assert mw.alphabet_class(b"\x00\x7f", b"\x80\xff")[1][0x80] == ord("G")
    # the GPU batch covers every case and every length at least three times, and has pairs at odd byte offsets
    pk, names = ac.gpu_batch_a()
    assert pk.n == len(names) == 42
    for case in ac.CASES:
        assert sum(n.startswith(case + "-") for n in names) >= 3, case
    for length in ac.LENGTHS:
        assert sum(n.endswith(f"-{length}") for n in names) >= 3, length
    assert sum(int(o) & 1 for o in pk.t_off) >= 10 and len({int(o) for o in pk.t_off[-3:]}) == 1


@pytest.mark.parametrize("pen", ["default", "unit"])
def test_premise_remapped_pair_aligns_like_the_original(oracle, pen):
    """(s, n_iter, CIGAR) of the oracle on the pair equal those on its image under the map: six pairs of 150-900 bases, under the default penalties
    and under (x, o1, e1, o2, e2) = (1, 0, 1, 0, 1)."""
    from oracle.pyoracle import make_opt
    kw = {} if pen == "default" else dict(x=1, o1=0, e1=1, o2=0, e2=1)
    for k, (case, length) in enumerate([("lower", 150), ("acgu", 300), ("two", 450), ("four_bytes", 600), ("one", 750), ("lower", 900)]):
        t, q = ac.recode(case, *ac.base_pair(7700 + k, length, 0.06))
        cls, m = mw.alphabet_class(t, q)
        assert cls == 1
        for flag in (0, 1):
            o = make_opt(flag=flag, **kw)
            assert oracle.align(t.translate(m), q.translate(m), o) == oracle.align(t, q, o), (case, length, flag)


def test_symbols_exported_and_declared():
    L = mw.lib()
    text = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    for name in ("mwf_alphabet_class", "mwf_gpu_batch_alphabet"):
        assert hasattr(L, name) and name in api.ABI_SYMBOLS and re.search(r"\b" + name + r"\s*\(", text), name
    assert '"alpha_remap"' in text
    assert "mwf_alphabet.hip" in mwbuild.SOURCES


def test_new_object_holds_gfx950_kernels():
    """The unit's object is the library's own: once mw.lib() has built it, it is there (a tree without the unit fails here), and its gfx950 code
    object holds the six kernels: three workgroup sizes x (classify, copy)."""
    mw.lib()
    assert os.path.exists(ALPHA_OBJ), "no " + os.path.relpath(ALPHA_OBJ, ROOT) + " (the library was not built from this tree)"
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    tools = {t: (os.path.join(llvm, t) if os.path.exists(os.path.join(llvm, t)) else shutil.which(t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    assert all(tools.values()) and cxxfilt, "llvm-objcopy, clang-offload-bundler, llvm-readelf or c++filt not found"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fb, ALPHA_OBJ, os.path.join(d, "copy.o")], check=True, capture_output=True)
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co],
                       check=True, capture_output=True)
        syms = subprocess.run([tools["llvm-readelf"], "-sW", co], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run([cxxfilt], input=syms, check=True, capture_output=True, text=True).stdout
    got = {(int(m.group(1)), int(m.group(2))) for ln in dem.splitlines() for m in [re.search(r"\bFUNC\b.*alphabet_kernel<(\d+), (\d+)>", ln)] if m}
    assert got == {(b, mode) for b in (64, 256, 1024) for mode in (0, 1)}, got


def test_host_twin_under_sanitizers(tmp_path):
    """tests/host/alphabet_class_sanitize.cpp + csrc/mwf_dbg.cpp built with -fsanitize=address,undefined: host code only, nothing loaded into
    python.  The sequences are heap blocks of exactly their length, flush against the end of their allocations."""
    exe = tmp_path / "alphabet_class_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "alphabet_class_sanitize.cpp"),
           os.path.join(ROOT, "miniwfa_amd", "csrc", "mwf_dbg.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "alphabet_class_sanitize OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
