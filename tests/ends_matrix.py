"""The instantiations of the ends-free / extension kernel (miniwfa_amd/csrc/mwf_ends.hip: wfa_ends_kernel<T, EXT>, four kernels, each holding the two bodies
ends_pass<T, TB, EXT>), one entry per body, with what reaches it, its penalty sets, its allowances or (A, Z) and its inputs.  The structure is
tests/generic_matrix.py's.

  tests/test_ends_matrix_cpu.py   the restatements (ends_ref.wfa_ends, ext_ref.wfa_ext, with the shrink) against the oracle and the DP on these inputs; every
                                  condition the GPU tests rely on (penalties beyond 256 and 512, shrinks that narrow the band, the long exact run, the launch rule)
  tests/test_ends_matrix_gpu.py   one test per entry: per penalty set and allowance set (ends form) or (A, Z) (EXT) one align whose only launch is that form on
                                  that many threads (the `ends-free launch:` / `extension launch:` record, MWF_DEBUG), no re-run, every answer the restatement's

Rule: an instantiation is added (or removed, or re-parameterised) together with its entry here.  (tests/test_ext_cpu.py compares the object's kernels with
ENDS_KERNELS; this table's (T, EXT) set must equal it.)

No tunable chooses the workgroup size: run_ends_kernel (mwf_plan.cpp) takes 512 threads when min(max(tl + ql) + 1, 2 max(bound) + 3) >= 8192 over the batch
(window_block) and 256 otherwise, so the inputs select the form:
  narrow batch   pairs of at most 400 bases (one or two longer ones under the cheap sets), tl + ql + 1 < 8192: 256 threads
  wide batch     three pairs with tl + ql + 1 >= 8192 each — and 2 bound + 3 >= 8192 under every set —: 512 threads
"""
from __future__ import annotations

import functools
import json
import os
from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import mutate, random_seq, skewed_pairs, synth_pair
from band_matrix import penalty_bound
from generic_matrix import FAST_SETS, PEN, nH
from test_ext_cpu import ENDS_KERNELS

import ends_ref as er
import ext_ref as xr

FREE = er.FREE
Inst = namedtuple("Inst", "T EXT TB")
MATRIX = tuple(Inst(T, EXT, TB) for T in (256, 512) for EXT in (0, 1) for TB in (0, 1))
assert len(MATRIX) == 8 and {(i.T, "true" if i.EXT else "false") for i in MATRIX} == ENDS_KERNELS

SETS = FAST_SETS                  # all twelve shapes of the generic kernel's table: the pass restates the same ring arithmetic
REFUSED = "ring257"               # nH = 257: refused by the host (kMaxRing)
assert len(SETS) == 12 and max(nH(PEN[n]) for n in SETS) == 256 and nH(PEN[REFUSED]) == 257

# allowances (t_beg, t_end, q_beg, q_end) of the ends form.  Under (0, FREE, FREE, 0) the empty alignment (qb = ql, te = 0) costs nothing: every pair ends at
# penalty 0, on the lowest column of an origin window of ql + 1 columns that holds an end cell.  (20, 20, 20, 20) leaves unrelated pairs dearer than 256.
ALLOW = ((0, 0, 0, 0), (FREE, FREE, 0, 0), (7, 0, 0, 1000), (0, FREE, FREE, 0), (20, 20, 20, 20))
# (A, Z) of the EXT form: no drop rule, and a drop that pairs with unrelated tails meet beyond penalty 256 (tests/test_ends_matrix_cpu.py: which)
EXT_NARROW = ((2, -1), (1, 300))
EXT_WIDE = ((1, -1), (1, 150))
DROP_WIDE_SETS = tuple(n for n in SETS if n not in ("edit", "o1zero"))   # where Z = 150 ends pair (c) of the wide batch beyond penalty 256 (its tails are too cheap under those two)
WIDE_WINDOW = 8192                # mwf_plan.cpp window_block


def inst_id(i: Inst) -> str:
    return f"T{i.T}-{'ext' if i.EXT else 'ends'}-{'cigar' if i.TB else 'score'}"


def pen_tuple(name: str):
    p = PEN[name]
    return p["x"], p["o1"], p["e1"], p["o2"], p["e2"]


def window_block(p: dict, pairs, max_s: int = 0) -> int:
    """mwf_plan.cpp window_block over one batch (penalty_bound honours max_s: the pass stops one penalty after it)."""
    max_len = max(len(t) + len(q) for t, q in pairs)
    max_bound = max(penalty_bound(p, len(t), len(q)) for t, q in pairs)
    if max_s > 0:
        max_bound = min(max_bound, max_s + 1)
    return 512 if min(max_len + 1, 2 * max_bound + 3) >= WIDE_WINDOW else 256


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _window_pair(seed: int, tl: int, at: int, m: int, p: float):
    t = random_seq(seed, tl)
    return t, mutate(t[at:at + m], seed + 500, p)


@functools.lru_cache(maxsize=None)
def _narrow_common():
    t200, t40 = random_seq(11, 200), random_seq(12, 40)
    a, bq = random_seq(13, 90), random_seq(14, 60)
    p = [synth_pair(2101, 300, 0.03), synth_pair(2102, 350, 0.05), synth_pair(2103, 200, 0.02), synth_pair(2104, 400, 0.02)]   # related: below penalty 256
    p += skewed_pairs(21, 9, 100, 400)                                                                                           # a third unrelated, the others one long gap
    p += [(random_seq(31, 400), random_seq(32, 380)), (random_seq(33, 390), random_seq(34, 400)), (random_seq(35, 300), random_seq(36, 400)),
          (random_seq(37, 400), random_seq(38, 250)), (random_seq(39, 333), random_seq(40, 367))]                                # unrelated: beyond 256
    p += [_window_pair(41, 400, 120, 150, 0.05), _window_pair(42, 380, 0, 200, 0.08), (a + bq, bq + random_seq(15, 70))]         # reads in windows, a dovetail
    p += [(b"", t40), (t40, b""), (b"", b""), (b"A", b"C"), (b"A", b"A"), (b"G", b""), (t200, t200)]
    return tuple(p)


# what the cheap sets need to pass 256 four times and 512 once: unrelated pairs long enough for them
_NARROW_EXTRA = {
    "edit": ((51, 560, 52, 600), (53, 620, 54, 580), (59, 600, 60, 640), (55, 1100, 56, 1080)),
    "o1zero": ((57, 640, 58, 600),),
}


@functools.lru_cache(maxsize=None)
def narrow_pairs(pen_name: str):
    return _narrow_common() + tuple((random_seq(s1, n1), random_seq(s2, n2)) for s1, n1, s2, n2 in _NARROW_EXTRA.get(pen_name, ()))


@functools.lru_cache(maxsize=None)
def _wide():
    """(a) 4200 x ~4200 at 1 % around an exact run of 1200 bases from base 701 of the target on, a mismatch on each side of it: the traceback's 512-bases-per-trip
           back-match goes through whole trips (stop == 0) and finds the run's begin in a later one;
       (b) a read of 2000 bases at 5 % from base 2100 of a window of 6200: under free target ends the origin window is 6201 columns, more than 8 x 512;
           for EXT, which starts at the origin, the window is rotated to begin at the read;
       (c) a core of 4100 bases — the first 1400 exact, then a mismatch, the rest at 1 % — with unrelated tails of 280 and 230 bases: the pass goes beyond 256
           on 512 threads, and the back-match reaches the sequences' begin from beyond base 1023 (it leaves the 512-per-trip loop still open)."""
    other = bytes.maketrans(b"ACGT", b"CGTA")
    t = random_seq(61, 4200)
    qa = mutate(t[:700], 62, 0.01) + t[700:701].translate(other) + t[701:1901] + t[1901:1902].translate(other) + mutate(t[1902:], 63, 0.01)
    w = random_seq(64, 6200)
    read = mutate(w[2100:4100], 65, 0.05)
    core = random_seq(66, 4100)
    qc = core[:1400] + core[1400:1401].translate(other) + mutate(core[1401:], 67, 0.01)
    return dict(a=(t, qa), b=(w, read), b_rot=(w[2100:] + w[:2100], read), c=(core + random_seq(68, 280), qc + random_seq(69, 230)))


def wide_pairs(ext: int, allow=None):
    """The wide batch of a cell.  Ends form: (b) is there where both target ends are free — under any other allowances it is a gap of 4200 bases, penalties
    beyond 4200 on a window of 8201 columns, which adds minutes to the restatement and nothing to what the kernel runs through."""
    W = _wide()
    if ext:
        return (W["a"], W["b_rot"], W["c"])
    return (W["a"], W["b"], W["c"]) if allow[0] == FREE and allow[1] == FREE else (W["a"], W["c"])


def batch(inst: Inst, pen_name: str, cfg):
    """The pairs of one run of an entry; cfg: the allowances (ends form) or (A, Z) (EXT)."""
    return narrow_pairs(pen_name) if inst.T == 256 else wide_pairs(inst.EXT, cfg)


def cells(inst: Inst):
    """[(penalty set, cfg)] of an entry."""
    cfgs = (EXT_NARROW if inst.T == 256 else EXT_WIDE) if inst.EXT else ALLOW
    return [(n, c) for n in SETS for c in cfgs]


# the pairs of the persistent-loop test: 26 of at most 120 bases, and six without a common letter, of which a pair of L target bases costs a gap of L - 7 under
# (7, 0, 0, 1000) — a pair of at most 120 bases cannot cost more than 135 there, so these six are longer
@functools.lru_cache(maxsize=None)
def loop_pairs():
    ac, gt = bytes.maketrans(b"GT", b"AC"), bytes.maketrans(b"AC", b"GT")
    p = [synth_pair(3000 + k, 60 + 2 * k, 0.03 + 0.01 * (k % 5)) for k in range(14)]
    p += [(random_seq(3100 + k, 50 + 5 * k), random_seq(3200 + k, 110 - 4 * k)) for k in range(8)]
    p += [_window_pair(3300, 120, 30, 60, 0.05), _window_pair(3301, 100, 0, 50, 0.1), (b"", b"ACGT"), (b"ACGTAC", b"")]
    p += [(random_seq(3400 + k, 280 + 9 * k).translate(ac), random_seq(3500 + k, 300 - 7 * k).translate(gt)) for k in range(6)]
    assert len(p) == 32 and len(set(p)) == 32
    return tuple(p)


LOOP_PEN = (4, 4, 2, 15, 1)
LOOP_ALLOW = (7, 0, 0, 1000)
LOOP_EXT = (1, 40)
LOOP_COPIES = 8192


def loop_order():
    """Which of the 32 pairs each of the 8192 is: every pair 256 times, in a seeded shuffled order."""
    return np.random.default_rng(8192).permutation(np.repeat(np.arange(32), LOOP_COPIES // 32))


# ---- the restated answers ---------------------------------------------------------------------------------------------------------------
_full: dict = {}   # (pair, penalties, EXT, cfg) -> (answer, the band of every penalty, the shrinks), once per process


def _full_job(key):
    (t, q), pen, ext, cfg = key
    trace, shrinks = [], []
    r = xr.wfa_ext(t, q, pen, *cfg, trace=trace, shrinks=shrinks) if ext else er.wfa_ends(t, q, pen, cfg, trace=trace, shrinks=shrinks)
    return r, tuple(trace), tuple(shrinks)


def ends_full(pair, pen, allow):
    """ends_ref.wfa_ends: ((s, n_iter, te, qe), the band of every penalty, the shrinks)."""
    key = (pair, pen, 0, tuple(allow))
    if key not in _full:
        _full[key] = _full_job(key)
    return _full[key]


def ext_full(pair, pen, A: int, Z: int):
    """ext_ref.wfa_ext: (its record, the band of every penalty, the shrinks)."""
    key = (pair, pen, 1, (A, Z))
    if key not in _full:
        _full[key] = _full_job(key)
    return _full[key]


def warm(executor):
    """Every restated answer of fixture_runs() that this process does not hold yet, computed side by side on `executor` (host processes: three quarters of a
    minute of numpy on one)."""
    todo = list(dict.fromkeys((tq, pen, ext, tuple(cfg)) for _, pairs, pen, ext, cfg in fixture_runs() for tq in pairs))
    todo = [k for k in todo if k not in _full]
    todo.sort(key=lambda k: -(len(k[0][0]) + len(k[0][1])))   # the long pairs first
    for k, v in zip(todo, executor.map(_full_job, todo, chunksize=8)):
        _full[k] = v


def want_ends(pair, pen, allow):
    return ends_full(pair, pen, allow)[0]


def want_ext(pair, pen, A: int, Z: int):
    return ext_full(pair, pen, A, Z)[0]


def restated(pairs, pen, ext: int, cfg):
    """One run's answers as the fixture holds them: [s, n_iter, te, qe] per pair, and for EXT V, s_stop, why, F behind them."""
    return [list(want_ext(tq, pen, *cfg)[:8]) if ext else list(want_ends(tq, pen, cfg)) for tq in pairs]


# tests/golden/ends_matrix.jsonl (tests/golden/make_golden_ends_matrix.py) holds restated() of every run below, so that the GPU tests need not compute them (three
# quarters of a minute of numpy); tests/test_ends_matrix_cpu.py recomputes every line and checks the restatement against the oracle and the DP.  Answers of the
# restatement, never of the kernel.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ends_matrix.jsonl")


def run_key(T, ext: int, pen_name: str, cfg) -> str:
    return f"T{T}-{'ext' if ext else 'ends'}-{pen_name}-" + ",".join("FREE" if v == FREE else str(v) for v in cfg)


def fixture_runs():
    """[(key, pairs, penalties, EXT, cfg)] of every run the fixture holds: the cells of the table (the TB twins share theirs) and the two persistent-loop batches."""
    out = []
    for inst in MATRIX:
        if not inst.TB:
            out += [(run_key(inst.T, inst.EXT, n, c), batch(inst, n, c), pen_tuple(n), inst.EXT, c) for n, c in cells(inst)]
    out.append((run_key("loop", 0, "default", LOOP_ALLOW), loop_pairs(), LOOP_PEN, 0, LOOP_ALLOW))
    out.append((run_key("loop", 1, "default", LOOP_EXT), loop_pairs(), LOOP_PEN, 1, LOOP_EXT))
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return {v["run"]: v["want"] for v in map(json.loads, f)}


def expected(inst, pen_name: str, cfg):
    """The fixture's answers of one run of an entry (inst: an Inst, or "loop" with pen_name "default")."""
    T, ext = ("loop", len(cfg) == 2) if inst == "loop" else (inst.T, inst.EXT)
    return [tuple(w) for w in _golden()[run_key(T, ext, pen_name, cfg)]]
