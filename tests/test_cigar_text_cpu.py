"""CPU-side checks of the alignment-text layer (include/miniwfa.h, MWF_TXT_*): the host twin mwf_cigar_text against the hand pair's literals, the
reference's golden CIGAR strings and an independent restatement of the six rules (tests/cigar_text_ref.py); its snprintf contract; unrenderable
words; letter case and digit counts; and the same hand pair and unrenderable words in a stand-alone program under AddressSanitizer / UBSan.  All
comparisons are byte equality.  The device kernels are checked against the same references in tests/test_cigar_text_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import miniwfa_amd as mw
from miniwfa_amd import api
from conftest import load_golden, golden_inputs, ROOT
from cigar_ops_ref import HAND_T, HAND_Q, HAND_WORDS, OP_I, OP_D, OP_EQ, OP_X, malformed_variants, rec
from cigar_text_ref import KINDS, HAND_TEXT, py_text, py_texts, renderable, digit_pair

NEW_SYMBOLS = ("mwf_cigar_text", "mwf_gpu_batch_text", "mwf_gpu_batch_dev_text", "mwf_gpu_batch_text_fetch")


def raw_text(kind, words, t, q, cap, fill=0x23):
    """mwf_cigar_text into a buffer of cap + 8 bytes filled with '#': (return value, the whole buffer)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    buf = (C.c_char * (cap + 8))(*([fill] * (cap + 8)))
    n = mw.lib().mwf_cigar_text(kind, len(w), w.ctypes.data if len(w) else None, len(t), t, len(q), q, buf if cap else None, cap)
    return n, buf.raw


def test_constants_and_symbols():
    assert (mw.MWF_TXT_CIGAR, mw.MWF_TXT_SAM, mw.MWF_TXT_CS, mw.MWF_TXT_MD, mw.MWF_TXT_ROW_T, mw.MWF_TXT_ROW_Q, mw.MWF_TXT_KINDS) == tuple(range(7))
    text = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    for name, value in zip(("CIGAR", "SAM", "CS", "MD", "ROW_T", "ROW_Q", "KINDS"), range(7)):
        assert re.search(r"#define\s+MWF_TXT_%s\s+%d\b" % (name, value), text), name
    L = mw.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in api.ABI_SYMBOLS, name


def test_hand_pair():
    for kind in KINDS:
        assert mw.cigar_text(kind, HAND_T, HAND_Q, HAND_WORDS) == HAND_TEXT[kind], kind
        assert py_text(kind, HAND_WORDS, HAND_T, HAND_Q) == HAND_TEXT[kind], kind      # the restatement agrees with the literals too
    # two empty sequences, no words: a valid (empty) alignment whose MD is "0"
    assert [mw.cigar_text(kind, b"", b"", []) for kind in KINDS] == [b"", b"", b"", b"0", b"", b""] == py_texts([], b"", b"")


def test_snprintf_contract():
    for kind in KINDS:
        want = HAND_TEXT[kind]
        for cap in (0, len(want) - 1, len(want)):
            n, buf = raw_text(kind, HAND_WORDS, HAND_T, HAND_Q, cap)
            assert n == len(want), (kind, cap, n)
            assert buf[:cap] == want[:cap] and buf[cap:] == b"#" * 8, (kind, cap, buf)


def _parse(cig):
    return [int(n) << 4 | api.CIGAR_CHARS.index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=XBid])", cig)]


def test_host_twin_on_golden_cigars():
    n = 0
    for v in load_golden("exact_small.jsonl"):
        if v["kind"] != "literal" or v["expect"].get("cigar") is None:
            continue
        words = _parse(v["expect"]["cigar"])
        t, q = golden_inputs(v)
        got = [mw.cigar_text(kind, t, q, words) for kind in KINDS]
        assert got[0] == v["expect"]["cigar"].encode(), v["id"]           # the reference's own text, byte for byte
        assert got == py_texts(words, t, q), v["id"]
        s = rec(mw.cigar_summary(t, q, mw.opt_init(), words))
        assert len(got[4]) == len(got[5]) == s[3] + s[4] + s[5] + s[6], v["id"]
        # stripping the gaps from a row gives back the sequence: every '-' where the sequence has none of its own (one golden pair is made of all 256
        # byte values, '-' among them), and by position — the columns under I (target row) / D (query row) — for every pair
        for row, seq, gap_op in ((got[4], t, OP_I), (got[5], q, OP_D)):
            if b"-" not in seq:
                assert row.replace(b"-", b"") == seq, v["id"]
            gap = np.repeat(np.array([int(w) & 15 == gap_op for w in words], dtype=bool), np.array([int(w) >> 4 for w in words], dtype=np.int64))
            arr = np.frombuffer(row, dtype=np.uint8)
            assert (arr[gap] == 0x2D).all() and arr[~gap].tobytes() == seq, v["id"]
        n += 1
    assert n > 100, n


def test_unrenderable_words():
    variants = {k: malformed_variants(HAND_WORDS)[k][0] for k in ("op15", "eq_plus7", "dropped", "huge")}
    variants["len0"] = HAND_WORDS[:3] + [0 << 4 | OP_I] + HAND_WORDS[3:]
    for name, words in variants.items():
        assert not renderable(words, len(HAND_T), len(HAND_Q)), name
        for kind in KINDS:
            n, buf = raw_text(kind, words, HAND_T, HAND_Q, 64)
            assert n == -1 and buf == b"#" * 72, (name, kind, n, buf)
            assert mw.cigar_text(kind, HAND_T, HAND_Q, words) is None and py_text(kind, words, HAND_T, HAND_Q) is None
    n, buf = raw_text(6, HAND_WORDS, HAND_T, HAND_Q, 64)
    assert n == -1 and buf == b"#" * 72
    assert mw.cigar_text(6, HAND_T, HAND_Q, HAND_WORDS) is None and mw.cigar_text(-1, HAND_T, HAND_Q, HAND_WORDS) is None


def test_letter_case_and_digits():
    t, q, words = digit_pair()
    assert renderable(words, len(t), len(q))
    got = [mw.cigar_text(kind, t, q, words) for kind in KINDS]
    assert got == py_texts(words, t, q)
    # stated by hand: the digit counts change from run to run; cs lowers only A..Z, MD copies the target byte verbatim
    assert got[0] == b"9=1X10=1X99=1X100=1X999=1X1000="
    assert got[1] == b"%dM" % (9 + 10 + 99 + 100 + 999 + 1000 + 5)
    assert got[2] == b":9*ac:10*ng:99*\x80t:100*ta:999*g\xfe:1000"
    assert got[3] == b"9A10N99\x80100t999G1000"
    assert got[4] == t and got[5] == q                                    # no gaps: the rows are the sequences, verbatim
    # ... and under I and D: lower case stays, upper case is lowered in cs only, N and a byte >= 0x80 are copied
    w2 = [1 << 4 | OP_EQ, 3 << 4 | OP_D, 1 << 4 | OP_EQ, 1 << 4 | OP_X, 1 << 4 | OP_EQ, 2 << 4 | OP_I]
    t2, q2 = b"A" + b"cN\x80" + b"G" + b"t" + b"T", b"A" + b"G" + b"a" + b"T" + b"N\xf0"
    got2 = [mw.cigar_text(kind, t2, q2, w2) for kind in KINDS]
    assert got2 == py_texts(w2, t2, q2)
    assert got2[2] == b":1-cn\x80:1*ta:1+n\xf0"
    assert got2[3] == b"1^cN\x801t1"
    assert got2[4] == b"AcN\x80GtT--" and got2[5] == b"A---GaTN\xf0"


def test_host_twin_under_sanitizers(tmp_path):
    """The hand pair and the unrenderable sets again in a stand-alone program (tests/host/cigar_text_sanitize.cpp + csrc/mwf_dbg.cpp) built with
    -fsanitize=address,undefined: host code only, nothing loaded into python.  The sequences and dst are heap blocks of exactly their size."""
    exe = tmp_path / "cigar_text_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "cigar_text_sanitize.cpp"),
           os.path.join(ROOT, "miniwfa_amd", "csrc", "mwf_dbg.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "cigar_text_sanitize OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
