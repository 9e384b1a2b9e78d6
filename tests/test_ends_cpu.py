"""Ends-free alignment without a GPU: the ABI is there, and the yardsticks of tests/ends_ref.py agree with the oracle and with each other."""
import ctypes as C
import os

import numpy as np

import miniwfa_amd as mw
from miniwfa_amd import api
from miniwfa_amd.synth import synth_pair
from oracle.pyoracle import make_opt

import ends_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mwf_gpu_batch_align_ends", "mwf_gpu_batch_ranges", "mwf_gpu_batch_dev_ranges", "mwf_wfa_ends", "mwf_wfa_ends_batch")
PENS = ((4, 4, 2, 15, 1), (4, 6, 3, 26, 1), (2, 3, 1, 9, 1), (3, 0, 2, 6, 1), (1, 1, 1, 1, 1))  # (each keeps a pair of up to 60 bases below penalty 256)
UNIT = b"ACGTTGCA"
X20 = b"ACGTTGCAACGCATGGATCC"
# the two fixed answers of the feature's specification: (target, query, allowances, s, CIGAR words, range)
FIXED = ((UNIT * 5, UNIT * 2, (1000, 1000, 0, 0), 0, [16 << 4 | 7], (24, 40, 0, 16)),
         (X20, b"T" * 10 + X20, (0, 0, 4, 0), 16, [6 << 4 | 1, 20 << 4 | 7], (0, 20, 4, 30)))


def rand_pair(rng, max_len, two_letter=False):
    alpha = np.frombuffer(b"AC" if two_letter else b"ACGT", dtype=np.uint8)
    t = alpha[rng.integers(0, len(alpha), int(rng.integers(0, max_len + 1)))]
    if rng.random() < 0.3:  # unrelated
        q = alpha[rng.integers(0, len(alpha), int(rng.integers(0, max_len + 1)))]
    else:  # a mutated piece of the target
        a = int(rng.integers(0, len(t) + 1))
        b = int(rng.integers(a, len(t) + 1))
        q = [c if rng.random() > 0.15 else alpha[rng.integers(0, len(alpha))] for c in t[a:b] if rng.random() > 0.05]
        q = np.array(q, dtype=np.uint8)[:max_len]
    return t.tobytes(), q.tobytes()


def test_abi_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "miniwfa.h")).read()
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in api.ABI_SYMBOLS and hasattr(L, name), name
    assert "mwf_ends_t" in header
    assert C.sizeof(mw.MwfEnds) == 16
    assert [f for f, _ in mw.MwfEnds._fields_] == ["t_beg", "t_end", "q_beg", "q_end"]
    for name in ("align_ends", "ranges", "dev_ranges_ptr"):
        assert hasattr(mw.Batch, name), name


def test_dp_with_zero_allowances_is_the_global_optimum(oracle):
    for pen in PENS[:2]:
        x, o1, e1, o2, e2 = pen
        for k in range(50):
            t, q = synth_pair(7100 + k, 20 + 2 * k, 0.12)
            if k % 5 == 0:
                q = q[:len(q) // 2]
            s, _, _ = oracle.align(t, q, make_opt(x=x, o1=o1, e1=e1, o2=o2, e2=e2))
            assert er.dp_score(t, q, pen, (0, 0, 0, 0)) == s, (pen, k)


def test_restated_pass_finds_the_dp_optimum():
    rng = np.random.default_rng(20240611)
    allow = (0, 1, 7, 1000)
    for k in range(200):
        t, q = rand_pair(rng, 60, two_letter=k % 2 == 1)
        pen = PENS[k % len(PENS)]
        ends = tuple(int(allow[v]) for v in rng.integers(0, 4, 4))
        want = er.dp_score(t, q, pen, ends)
        assert want < 256
        s, n_iter, te, qe = er.wfa_ends(t, q, pen, ends)
        assert s == want, (k, pen, ends, t, q)
        assert te == len(t) or qe == len(q)
        assert len(t) - te <= ends[1] and len(q) - qe <= ends[3]
        assert (n_iter == 0) == (s == 0)


def test_fixed_answers():
    opt = mw.opt_init(flag=mw.MWF_F_CIGAR)
    pen = er.pen_of(opt)
    for t, q, ends, s, words, rng in FIXED:
        assert er.dp_score(t, q, pen, ends) == s
        got = er.wfa_ends(t, q, pen, ends)
        assert (got[0], got[2], got[3]) == (s, rng[1], rng[3])
        er.check_cigar(mw, opt, t, q, words, rng, ends, s)


def test_checker_rejects_wrong_alignments():
    opt = mw.opt_init(flag=mw.MWF_F_CIGAR)
    t, q, ends, s, words, rng = FIXED[1]
    for bad in (dict(rng=(0, 20, 5, 30)),            # clips more than q_beg allows
                dict(words=[26 << 4 | 7]),           # = over unequal bases
                dict(words=[6 << 4 | 1, 19 << 4 | 7]),  # does not consume the ranges
                dict(s=15)):                         # another score
        kw = dict(words=words, rng=rng, s=s)
        kw.update(bad)
        try:
            er.check_cigar(mw, opt, t, q, kw["words"], kw["rng"], ends, kw["s"])
        except AssertionError:
            continue
        raise AssertionError(f"the checker accepted {bad}")
