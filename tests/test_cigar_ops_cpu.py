"""CPU-side checks of the alignment-summary layer (include/miniwfa.h, mwf_aln_summary_t): the record's layout, the exported symbols and the
host twin mwf_cigar_summary — on the reference's golden CIGARs, on malformed words with hand-stated answers, and the same malformed words in a
stand-alone program under AddressSanitizer / UBSan.  All comparisons are integer equality.  The device kernels are checked against the same
references in tests/test_cigar_ops_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import miniwfa_amd as mw
from miniwfa_amd import api
from conftest import load_golden, golden_inputs, ROOT
from cigar_ops_ref import (FIELDS, HAND_T, HAND_Q, HAND_CASES, EMPTY_PAIR_RECORD, DEFAULT_PEN, py_summary, py_maps, rec)

NEW_SYMBOLS = ("mwf_cigar_summary", "mwf_gpu_batch_dev_cigars", "mwf_gpu_batch_summarize", "mwf_gpu_batch_dev_summary", "mwf_gpu_batch_summary",
               "mwf_gpu_batch_map", "mwf_gpu_batch_dev_map", "mwf_gpu_batch_map_fetch")


def test_summary_struct_layout_and_symbols():
    assert C.sizeof(api.AlnSummary) == 48 and api.SUMMARY_DTYPE.itemsize == 48
    assert tuple(name for name, _ in api.AlnSummary._fields_) == FIELDS == api.SUMMARY_DTYPE.names
    for k, name in enumerate(FIELDS):
        assert getattr(api.AlnSummary, name).offset == 4 * k == api.SUMMARY_DTYPE.fields[name][1], name
    L = mw.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in api.ABI_SYMBOLS, name
    # ... and the header declares the struct with those fields in that order
    text = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mwf_aln_summary_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for part in re.findall(r"int32_t ([^;]*);", body) for n in part.split(",")]
    assert tuple(declared) == FIELDS


def test_dev_array_interface():
    a = api.DevArray(0x1000, 7, "<i4").__cuda_array_interface__
    assert a["shape"] == (7,) and a["typestr"] == "<i4" and a["data"] == (0x1000, False) and a["version"] == 2


def _parse(cig):
    return [int(n) << 4 | api.CIGAR_CHARS.index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=XBid])", cig)]


def test_host_twin_on_golden_cigars():
    n = 0
    for v in load_golden("exact_small.jsonl"):
        if v["kind"] != "literal" or v["expect"].get("cigar") is None:
            continue
        words = _parse(v["expect"]["cigar"])
        pen = tuple(v["opt"][k] for k in ("x", "o1", "e1", "o2", "e2"))
        o = mw.opt_init(**dict(zip(("x", "o1", "e1", "o2", "e2"), pen)))
        t, q = golden_inputs(v)
        got = rec(mw.cigar_summary(t, q, o, words))
        assert got[10] == -1, v["id"]
        assert got[:3] == mw.cigar2score(o, words) == (v["expect"]["s"], len(t), len(q)), v["id"]
        assert got == py_summary(pen, words, t, q), v["id"]
        n += 1
    assert n > 100, n


def test_host_twin_on_malformed_words():
    o = mw.opt_init()
    assert (o.x, o.o1, o.e1, o.o2, o.e2) == DEFAULT_PEN
    for name, (words, want) in HAND_CASES.items():
        got = rec(mw.cigar_summary(HAND_T, HAND_Q, o, words))
        assert got == want, (name, got, want)
        assert py_summary(DEFAULT_PEN, words, HAND_T, HAND_Q) == want, name      # the restatement agrees with the hand-stated answers too
    assert rec(mw.cigar_summary(b"", b"", o, [])) == EMPTY_PAIR_RECORD == py_summary(DEFAULT_PEN, [], b"", b"")
    # the score follows the options handed in
    o2 = mw.opt_init(x=4, o1=6, e1=3, o2=26, e2=1)
    assert rec(mw.cigar_summary(HAND_T, HAND_Q, o2, HAND_CASES["clean"][0]))[0] == 4 + min(6 + 9, 26 + 3) + min(6 + 6, 26 + 2) == 31


def test_python_maps_of_the_hand_pair():
    """Pins the test helper py_maps — the numpy expansion the GPU tests compare the map kernel with — on the pair whose answer can be read
    off (10= 1X 3D 8= 2I 12=), and ties it to the host twin: the maps' lengths and their counts of partner / gap entries are the twin's
    t_len, q_len, n_eq + n_x, n_ins and n_del for the same words."""
    words = HAND_CASES["clean"][0]
    q2t, t2q = py_maps(words, len(HAND_T), len(HAND_Q))
    assert q2t.tolist() == list(range(11)) + list(range(14, 22)) + [-1 - 22, -1 - 22] + list(range(22, 34))
    assert t2q.tolist() == list(range(11)) + [-1 - 11] * 3 + list(range(11, 19)) + list(range(21, 33))
    r = {k: int(v) for k, v in zip(mw.SUMMARY_DTYPE.names, mw.cigar_summary(HAND_T, HAND_Q, mw.opt_init(), words))}
    assert (r["t_len"], r["q_len"], r["first_bad"]) == (len(t2q), len(q2t), -1)
    assert (int((q2t >= 0).sum()), int((t2q >= 0).sum())) == (r["n_eq"] + r["n_x"],) * 2
    assert (int((q2t < 0).sum()), int((t2q < 0).sum())) == (r["n_ins"], r["n_del"])


def test_host_twin_under_sanitizers(tmp_path):
    """The malformed cases again in a stand-alone program (tests/host/cigar_summary_sanitize.cpp + csrc/mwf_dbg.cpp) built with
    -fsanitize=address,undefined: host code only, nothing loaded into python.  The sequences are heap blocks of exactly their length."""
    exe = tmp_path / "cigar_summary_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "cigar_summary_sanitize.cpp"),
           os.path.join(ROOT, "miniwfa_amd", "csrc", "mwf_dbg.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "cigar_summary_sanitize OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
