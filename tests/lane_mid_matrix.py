"""The instantiations of the lane kernel (miniwfa_amd/csrc/mwf_lane.hip, wfa_lane_kernel<TB, S2, FOLD>, 6) and of the mid kernel
(miniwfa_amd/csrc/mwf_mid.hip, wfa_mid_kernel<T, TB, S2, FOLD>, 3 x 6), one entry each, with what reaches it — tunables, batch shape, penalty sets —
and the inputs of its two test groups, sized on the CPU from the oracle alone.  The structure is tests/band_matrix.py's.

  tests/test_lane_mid_cpu.py          the set of entries EQUALS the instantiations in the built objects; every cell has its inputs (self_check);
                                      the oracle reproduces tests/golden/lane_mid_pen.jsonl (the compiled reference under the penalty sets used here)
  tests/test_lane_mid_matrix_gpu.py   one test per entry: the launch record names that instantiation, the *fit* group is finished by it (no re-run),
                                      the *overflow* group is handed back, every answer equals the oracle's; and the edge tests

Rule: an instantiation is added (or removed, or re-parameterised) together with its entry here.

fit = the host starts the pair on the kernel (lane_admits / mid_admits restate mwf_plan_classes.h's classify_pair) AND none of the kernel's documented hand-backs
fires, each restated on the oracle's band trace (Oracle.band_trace_far) and the pair's lengths — never on what the device did:
  lane  chunks    k_use >= lane_chunks on center = tl + 1 (mwf_lane.hip, the test in front of the penalty's chunks); exact
        shrink    a final penalty above 255 - nH: the kernel hands back at the first penalty whose good bits a shrink would read; exact
        traceback rows of 64 x chunks bytes, one per penalty, in the slot the host sized (lane_tb_fits); exact
        alphabet  the 2-bit form finishes A/C/G/T only
  mid   span      lo < left || hi > right on the span C = 64 x groups around tl + 1 + (ql - tl) / 2; groups from the host's LDS rule for the LAUNCH
                  (mid_groups: the batch's longest pair decides); exact
        forecast  at penalties 64 / 256 / 1024 against C - 2 nH - 64 (mwf_device.h window_forecast; the furthest offset comes from Oracle.band_trace_far).  As
                  in the band matrix, a pair within 5 % of the threshold counts as not fit — and as not handed back either: it joins neither group
(Under penalty sets with dear extensions a window stays far narrower than the forecast's two columns per penalty: there the forecast, not the span, is what
hands pairs back.)  Candidates that pass every exact rule and are left out because of the forecast's margin are counted (n_dropped) and bounded by MAX_DROPPED_SHARE; the lane
rules are all exact, so the lane share is 0."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import synth_pair
from oracle.pyoracle import make_opt
from band_matrix import MAX_DROPPED_SHARE, ORACLE_THREADS, _rand, _trace_all, is_acgt, penalty_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_OBJ = os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_lane.hip.o")
MID_OBJ = os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_mid.hip.o")

LaneInst = namedtuple("LaneInst", "TB S2 FOLD")
MidInst = namedtuple("MidInst", "T TB S2 FOLD")


def inst_id(i) -> str:
    return f"lane-TB{i.TB}-S2{i.S2}-FOLD{i.FOLD}" if isinstance(i, LaneInst) else f"mid-T{i.T}-TB{i.TB}-S2{i.S2}-FOLD{i.FOLD}"


# ---- penalty sets -----------------------------------------------------------------------------------------------------------------------
# Both kernels read their penalties at run time.  fold: o1 == x (launch_lane / launch_v fold for ANY e1 then, score-only, band_fold 1).
PEN = {
    "default": dict(x=4, o1=4, e1=2, o2=15, e2=1),      # folds
    "a22": dict(x=4, o1=4, e1=2, o2=4, e2=2),           # main.c's -a preset: both pieces equal, every E1/E2 and F1/F2 tie is live; folds
    "edit": dict(x=1, o1=0, e1=1, o2=0, e2=1),          # edit distance: a ring of two slices, E/F rings of ONE row in the lane kernel (read and overwritten)
    "asm5": dict(x=4, o1=6, e1=3, o2=26, e2=1),
    "f_e1": dict(x=3, o1=3, e1=1, o2=9, e2=1),          # folding sets with e1 of 1, 3 and 8
    "f_e1_deep": dict(x=3, o1=3, e1=1, o2=30, e2=1),    # ... e1 of 1 on a ring deep enough that the mid kernel's span cannot hold every window of a 2 kb pair
    "f_e3": dict(x=4, o1=4, e1=3, o2=24, e2=1),
    "f_e8": dict(x=6, o1=6, e1=8, o2=40, e2=2),
    "e88": dict(x=4, o1=6, e1=8, o2=20, e2=8),          # mid_supported's limit on both pieces
    "e2gt": dict(x=4, o1=10, e1=1, o2=4, e2=3),         # e2 > e1
    "lane_deep": dict(x=4, o1=4, e1=2, o2=88, e2=1),    # nH + 2 e1 + 2 e2 == 96: the deepest rings the lane kernel admits; folds
    "mid_deep": dict(x=4, o1=4, e1=2, o2=62, e2=1),     # nH == 64: the deepest ring the mid kernel admits; folds
}
# just beyond each limit: these launch neither kernel (tests/test_lane_mid_matrix_gpu.py::test_limits)
PEN_BEYOND = {
    "lane_97": dict(x=4, o1=4, e1=2, o2=89, e2=1),
    "mid_nH65": dict(x=4, o1=4, e1=2, o2=63, e2=1),
    "mid_e1_9": dict(x=4, o1=4, e1=9, o2=30, e2=1),
    "mid_e2_9": dict(x=4, o1=4, e1=2, o2=15, e2=9),
}

# the lane kernel's gap runs across chunk edges (tests/test_lane_mid_matrix_gpu.py::test_lane_gap_runs_across_chunk_edges): e1 in {1, 2, 3, 8}, e2 in {1, 2, 8}
EDGE_PEN = {   # the piece a long gap runs on:
    "e1_2-e2_1": dict(x=4, o1=4, e1=2, o2=15, e2=1),        # E2 / F2
    "e1_1-e2_2": dict(x=4, o1=4, e1=1, o2=20, e2=2),        # E1 / F1
    "e1_3-e2_2": dict(x=4, o1=2, e1=3, o2=60, e2=2),        # E1 / F1 (up to 57 bases)
    "e1_8-e2_2": dict(x=6, o1=6, e1=8, o2=40, e2=2),        # E2 / F2
    "e1_1-e2_8": dict(x=2, o1=3, e1=1, o2=6, e2=8),         # E1 / F1
}


def nH(p: dict) -> int:
    """mwf_plan.cpp make_penalty: the H ring's depth."""
    return max(p["x"], p["o1"] + p["e1"], p["o2"] + p["e2"]) + 1


def pen_folds(p: dict) -> bool:
    return p["o1"] == p["x"]


def lane_supported(p: dict) -> bool:
    return p["x"] >= 1 and p["e1"] >= 1 and p["e2"] >= 1 and nH(p) + 2 * p["e1"] + 2 * p["e2"] <= 96 and nH(p) < 128


def mid_supported(p: dict) -> bool:
    return p["x"] >= 1 and p["e1"] >= 1 and p["e2"] >= 1 and nH(p) <= 64 and p["e1"] <= 8 and p["e2"] <= 8


assert nH(PEN["lane_deep"]) + 2 * 2 + 2 * 1 == 96 and lane_supported(PEN["lane_deep"]) and not lane_supported(PEN_BEYOND["lane_97"])
assert nH(PEN["mid_deep"]) == 64 and mid_supported(PEN["mid_deep"]) and not any(mid_supported(PEN_BEYOND[k]) for k in ("mid_nH65", "mid_e1_9", "mid_e2_9"))
assert nH(PEN_BEYOND["lane_97"]) + 6 == 97 and nH(PEN_BEYOND["mid_nH65"]) == 65

# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
# Routes, in tunables and batch shape only.
#   lane  mid_max_pairs 0, div_aware 0, coop_min_len out of reach; lane_chunks as the cell says; S2 = 1: seq2bit 1 and a pair with tl + ql >= 450 in
#         the batch (choose_kernel: max_len >= 450), every pair plain A/C/G/T; S2 = 0: seq2bit 0
#   mid   lane_max_len 0, at most mid_max_pairs pairs (the default: one per CU), mid_block T, seq2bit S2
#   FOLD  score-only, o1 == x, band_fold 1; the same set with band_fold 0 must launch the unfolded twin
# Cell: kernel, instantiation, lane_chunks (0: mid), runs ((penalty set, band_fold) — each must launch exactly that instantiation)
Cell = namedtuple("Cell", "kernel inst chunks runs")
LANE_MAX_LEN = 325      # mwf_engine.h lane_max_len
LANE_MAX_SKEW = 24      # classify_pair: skew <= 24
LANE_S2_MIN_LEN = 450   # choose_kernel: 2-bit copies from 450 bases of target + query on
LANE_COMMON = (("mid_max_pairs", 0), ("div_aware", 0), ("coop_min_len", 1 << 40))
MID_COMMON = (("lane_max_len", 0), ("div_aware", 0), ("coop_min_len", 1 << 40))
TB_BUDGET_MB = 512      # a traceback arena that holds every pair's rows at once: a re-run can then only be a hand-back
# The penalty sets are dealt over the cells: every set runs score-only and with CIGAR, on both sequence forms of the lane kernel or on both of one
# workgroup size of the mid kernel; every workgroup size has folding and non-folding sets.
LANE_SETS = {1: ("default", "asm5", "f_e1", "e2gt", "lane_deep", "a22"),       # S2 = 1: four chunks (300 bp pairs)
             0: ("edit", "e88", "f_e3", "f_e8", "asm5", "default")}            # S2 = 0: three chunks (150 bp pairs)
LANE_CHUNKS = {1: 4, 0: 3}
MID_SETS = {256: ("default", "asm5", "f_e1_deep", "edit"), 512: ("a22", "e88", "f_e3", "f_e1"), 1024: ("e2gt", "f_e8", "mid_deep")}


def _runs(sets, tb: int, fold: int):
    if tb:
        return tuple((s, 1) for s in sets)
    if fold:
        return tuple((s, 1) for s in sets if pen_folds(PEN[s]))
    return tuple((s, 1) for s in sets if not pen_folds(PEN[s])) + tuple((s, 0) for s in sets if pen_folds(PEN[s]))


def _matrix():
    cells = []
    for tb, s2, fold in ((1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 1, 1), (0, 0, 1)):
        cells.append(Cell("lane", LaneInst(tb, s2, fold), LANE_CHUNKS[s2], _runs(LANE_SETS[s2], tb, fold)))
    for T in (256, 512, 1024):
        for tb, s2, fold in ((1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 1, 1), (0, 0, 1)):
            cells.append(Cell("mid", MidInst(T, tb, s2, fold), 0, _runs(MID_SETS[T], tb, fold)))
    return cells


MATRIX = _matrix()


def cell_id(c: Cell) -> str:
    return inst_id(c.inst)


def declared_instantiations(kernel: str) -> set:
    return {c.inst for c in MATRIX if c.kernel == kernel}


def tunables(c: Cell, band_fold: int):
    if c.kernel == "lane":
        return LANE_COMMON + (("lane_chunks", c.chunks), ("seq2bit", c.inst.S2), ("band_fold", band_fold))
    return MID_COMMON + (("mid_block", c.inst.T), ("seq2bit", c.inst.S2), ("band_fold", band_fold))


for _c in MATRIX:   # a run's penalties and band_fold force the entry's FOLD; every set of the issue's list runs somewhere
    assert _c.runs, cell_id(_c)
    for _pn, _bf in _c.runs:
        assert bool(_c.inst.FOLD) == bool(_bf and pen_folds(PEN[_pn]) and not _c.inst.TB), (cell_id(_c), _pn, _bf)
        assert lane_supported(PEN[_pn]) if _c.kernel == "lane" else mid_supported(PEN[_pn]), (cell_id(_c), _pn)
assert {pn for c in MATRIX for pn, _ in c.runs} == set(PEN)
assert {PEN[pn]["e1"] for c in MATRIX if c.inst.FOLD for pn, _ in c.runs} >= {1, 2, 3, 8}   # FOLD with e1 other than 2


# ---- the instantiations of the built objects --------------------------------------------------------------------------------------------
def object_instantiations(kernel: str):
    """{LaneInst} / {MidInst} parsed from the object's symbol table (llvm-readelf -sW | c++filt: demangled kernel names only), or a string saying
    why that cannot be done here."""
    import shutil
    import subprocess
    obj, name, n_args, ctor = (LANE_OBJ, "wfa_lane_kernel", 3, LaneInst) if kernel == "lane" else (MID_OBJ, "wfa_mid_kernel", 4, MidInst)
    readelf = next((p for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf") or "") if p and os.path.exists(p)), None)
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not readelf or not cxxfilt:
        return "llvm-readelf or c++filt not found"
    if not os.path.exists(obj):
        return "no " + os.path.relpath(obj, ROOT) + " (the library was not built from this tree)"
    syms = subprocess.run([readelf, "-sW", obj], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run([cxxfilt], input=syms, check=True, capture_output=True, text=True).stdout
    out = set()
    for m in re.finditer(name + r"<([^<>]*)>", dem):
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args, m.group(0)
        vals = []
        for a in args:
            a = re.sub(r"^\(\w+\)", "", a).strip("()")
            vals.append({"true": 1, "false": 0}[a] if a in ("true", "false") else int(a) if re.fullmatch(r"-?\d+", a) else None)
        assert None not in vals, m.group(0)
        out.add(ctor(*vals))
    return out


# ---- the host's rules, restated (mwf_plan_classes.h classify_pair, and mwf_plan.cpp choose_kernel) ------------------------------------------
def _lenw(tl: int, ql: int) -> int:
    """The pair's length as the class limits see it (div_aware 0): a forced gap counts six-fold beyond a sixteenth of the length."""
    ln, skew = tl + ql, abs(tl - ql)
    return ln + 6 * max(0, skew - ln // 16)


def lane_lds_bytes(p: dict, chunks: int, seq_bytes: int) -> int:
    rings = ((nH(p) + 2 * p["e1"] + 2 * p["e2"]) * (32 * chunks + 2) * 4 + 15) // 16 * 16
    return (rings + seq_bytes + 64 + 15) // 16 * 16


def _group_seq_lds(pairs) -> int:
    """GroupInfo::max_seq_lds of a launch."""
    return max(((len(t) + 3) & ~3) + 8 + ((len(q) + 3) & ~3) + 16 for t, q in pairs)


def lane_admits(p: dict, tl: int, ql: int) -> bool:
    """to_lane: the penalties, the length limit, skew <= 24, and a band class of 1 ... 4 by the lengths (always 4 at these lengths: lenw + 1 <= 1400)."""
    return (lane_supported(p) and max(tl, ql) <= LANE_MAX_LEN and abs(tl - ql) <= LANE_MAX_SKEW and _lenw(tl, ql) + 1 <= 1400
            and tl + penalty_bound(p, tl, ql) < 32767)


def lane_group_admits(p: dict, chunks: int, s2: int, pairs) -> bool:
    """The launch: rings and sequence copies within 60 KB; the 2-bit form needs a pair of 450 bases of target + query."""
    if lane_lds_bytes(p, chunks, _group_seq_lds(pairs)) > 60 * 1024:
        return False
    return max(len(t) + len(q) for t, q in pairs) >= LANE_S2_MIN_LEN if s2 else True


def mid_seq_off(p: dict, C: int) -> int:
    """mwf_mid.hip mid_layout: rows | good bits | window table | bookkeeping, each on 16 bytes."""
    n, RL = nH(p), (C + 2 + 7) & ~7
    at = (n + 2 * (p["e1"] + 1) + 2 * (p["e2"] + 1)) * RL * 2
    at = (at + 15) & ~15
    at += n * (C // 64) * 8
    at += n * 8
    at = (at + 15) & ~15
    at += 48   # sizeof(MidVars)
    return (at + 15) & ~15


def mid_lds_bytes(p: dict, groups: int, seq_bytes: int) -> int:
    return (mid_seq_off(p, 64 * groups) + seq_bytes + 64 + 15) // 16 * 16


MID_LDS_LIMIT = 158 * 1024


def _mid_groups(p: dict, window: int, seq_bytes: int) -> int:
    groups = min((window + 2 * nH(p) + 63) // 64, 128)
    while groups > 1 and mid_lds_bytes(p, groups, seq_bytes) > MID_LDS_LIMIT:
        groups -= 1
    return groups


def mid_groups(p: dict, pairs) -> int:
    """choose_kernel (GEOM_MID): the span of a LAUNCH, from the longest pair, the largest penalty bound and the largest sequence copy of its pairs."""
    max_len = max(len(t) + len(q) for t, q in pairs)
    max_bound = max(penalty_bound(p, len(t), len(q)) for t, q in pairs)
    g = _mid_groups(p, min(max_len + 1, 2 * max_bound + 3), _group_seq_lds(pairs))
    assert mid_lds_bytes(p, g, _group_seq_lds(pairs)) <= MID_LDS_LIMIT
    return g


def _half(d: int) -> int:
    """(ql - tl) / 2 as C++ divides: towards zero."""
    return d // 2 if d >= 0 else -((-d) // 2)


def mid_span(groups: int, tl: int, ql: int):
    C = 64 * groups
    left = tl + 1 + _half(ql - tl) - C // 2
    return left, left + C - 1


def mid_admits(p: dict, tl: int, ql: int):
    """classify_pair, CLS_MID: False, or "holds_all" / "want" — which of the two conditions admitted the pair.  (The band class the lengths give must be
    at most 4: true of every pair whose weighed length stays within 8200.)"""
    bound, ln = penalty_bound(p, tl, ql), tl + ql
    if not mid_supported(p) or tl + bound >= 32760 or _lenw(tl, ql) + 1 > 8200:
        return False
    seq_lds = ((tl + 7) & ~7) + 16 + ((ql + 7) & ~7) + 32
    window = min(ln + 1, 2 * bound + 3)
    want = min(window, _lenw(tl, ql) * 34 // 100 + 128) + 2 * nH(p)
    groups = _mid_groups(p, window, seq_lds)
    if mid_lds_bytes(p, groups, seq_lds) > MID_LDS_LIMIT:
        return False
    left, right = mid_span(groups, tl, ql)
    if max(1, tl + 1 - (bound + 1)) - nH(p) >= left and min(ln + 1, tl + 1 + bound + 1) + nH(p) <= right:
        return "holds_all"
    return "want" if 64 * groups >= want and abs(tl - ql) < groups * 32 else False


# ---- the kernels' hand-backs, restated on the oracle's band trace (lohi: diagonals of every new slice, far: furthest offset of slice s - x) ------
def lane_k_use(lohi: np.ndarray) -> int:
    """The outermost chunk a penalty's window reaches: column c < center lies in chunk (center - 1 - c) / 32, c >= center in (c - center) / 32."""
    if not len(lohi):
        return 0
    lo, hi = int(lohi[:, 0].min()), int(lohi[:, 1].max())
    return max((-1 - lo) >> 5 if lo < 0 else 0, hi >> 5 if hi > 0 else 0)


def lane_s_max(p: dict) -> int:
    """The last penalty the lane kernel finishes a pair at: it hands back before computing penalty 256 - nH."""
    return 255 - nH(p)


def lane_tb_fits(p: dict, chunks: int, lohi: np.ndarray, tl: int, ql: int, n_slots: int) -> bool:
    """run_batch_kernel: the slot holds (min(bound, 256) + 2) rows of the span unless the budget cuts it; the kernel needs one row per penalty."""
    slot = max(4096, min((min(penalty_bound(p, tl, ql), 256) + 2) * 64 * chunks, (TB_BUDGET_MB << 20) // max(1, n_slots))) // 4 * 4
    return len(lohi) * 64 * chunks <= slot


def lane_fits(p: dict, chunks: int, lohi: np.ndarray) -> bool:
    return lane_k_use(lohi) < chunks and len(lohi) <= lane_s_max(p)


def mid_span_margin(groups: int, lohi: np.ndarray, tl: int, ql: int) -> int:
    """Columns between the pair's windows and the span's nearer edge, the smallest over the penalties; negative: handed back."""
    left, right = mid_span(groups, tl, ql)
    if not len(lohi):
        return min(tl + 1 - left, right - (tl + 1))
    return min(int(lohi[:, 0].min()) + tl + 1 - left, right - (int(lohi[:, 1].max()) + tl + 1), tl + 1 - left, right - (tl + 1))


def mid_forecast_margin(p: dict, groups: int, far: np.ndarray, tl: int, ql: int, off: float = 10.5) -> float:
    """Columns between the window the forecast expects (window_forecast) and the one it hands the pair back at, the smallest over penalties 64 / 256 / 1024,
    with 5 % taken off the threshold (off = 9.5: added to it); negative: counted as handed back.  The device looks at the furthest offset of slice s: entry
    s + x - 1 of the trace (the slice the mismatch term of penalty s + x read), or, where the pair ends before that, entry s - 1, which is never further."""
    cap, kmax, s_final, margin, x = 64 * groups - 2 * nH(p) - 64, -1, len(far), float("inf"), p["x"]
    for s in (64, 256, 1024):
        if s >= s_final:       # the pair is done at that penalty or before
            break
        kmax = max(kmax, int(far[s + x - 1] if s + x - 1 < s_final else far[s - 1]))
        if kmax < 8 or tl < 64:
            continue
        need = min(2 * s * tl // min(kmax + 1, tl) + 16, tl + ql + 1)
        slack = 25 if s < 128 else 17 if s < 512 else 13
        margin = min(margin, cap * slack / off - need)
    return margin


def mid_fits(p: dict, groups: int, lohi: np.ndarray, far: np.ndarray, tl: int, ql: int):
    """(the exact rules, the exact rules and the forecast)."""
    exact = mid_span_margin(groups, lohi, tl, ql) >= 0 and len(lohi) + tl < 32760
    return exact, exact and mid_forecast_margin(p, groups, far, tl, ql) >= 0


def mid_handed_back(p: dict, groups: int, lohi: np.ndarray, far: np.ndarray, tl: int, ql: int) -> bool:
    """The kernel hands the pair back for certain: its window leaves the span, or a forecast passes its threshold by 5 % and more."""
    return not mid_fits(p, groups, lohi, far, tl, ql)[0] or mid_forecast_margin(p, groups, far, tl, ql, off=9.5) < 0


def mid_holds_everything(p: dict, groups: int, tl: int, ql: int) -> bool:
    """The span holds every column of the pair's matrix: nothing such a pair does can leave it, and no forecast can reach the threshold."""
    left, right = mid_span(groups, tl, ql)
    return left <= 1 and right >= tl + ql + 1 and (64 * groups - 2 * nH(p) - 64) * 13 >= (tl + ql + 1) * 10


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _seed(kernel: str, pen_name: str) -> int:
    return (7 if kernel == "lane" else 9) * 100000 + 1000 * sorted(PEN).index(pen_name)


def _cut(t: bytes, q: bytes, L: int):
    return t[:L], q[:L]


def _mutate_non_acgt(t: bytes, q: bytes):
    k = len(t) // 3
    return t[:k] + b"N" + t[k + 1:], q[:k // 2] + b"n" + q[k // 2 + 1:2 * k] + b"R" + q[2 * k + 1:]


def _disjoint(tl: int, ql: int):
    """Sequences with no base in common (A/C against G/T): no match anywhere, the alignment is all mismatches and gaps — its penalty moves with the lengths."""
    r = np.random.default_rng(tl * 1000 + ql)
    return (np.frombuffer(b"AC", dtype=np.uint8)[r.integers(0, 2, tl)].tobytes(), np.frombuffer(b"GT", dtype=np.uint8)[r.integers(0, 2, ql)].tobytes())


_limit_cache: dict = {}


def lane_limit_pairs(orc, pen_name: str, chunks: int):
    """(a pair whose final penalty is exactly 255 - nH, that penalty, a pair that needs 256 - nH, that penalty) — where the costs' parity rules one of the two
    out (LANE_LIMIT_PARITY), the penalty next to it — or None where no pair inside the chunks costs that much.  A window grows by a column either side per penalty whatever the bases (a gap
    can always be opened), so only the matrix keeps a window of such a penalty inside the chunks: tl <= 32 chunks, ql < 32 chunks.  Searched over pairs
    without a common base, whose penalty follows from the lengths."""
    key = (pen_name, chunks)
    if key not in _limit_cache:
        p, smax = PEN[pen_name], lane_s_max(PEN[pen_name])
        cand = [_disjoint(tl, ql) for tl in range(32 * chunks, 20, -1) for ql in range(min(32 * chunks - 1, tl + LANE_MAX_SKEW), max(0, tl - LANE_MAX_SKEW) - 1, -1)]
        o = make_opt(**p)
        sc = [r[0] for r in orc.align_many(cand, o, threads=ORACLE_THREADS)[0]]
        below = sorted((-s, i) for i, s in enumerate(sc) if smax - 1 <= s <= smax)
        above = sorted((s, i) for i, s in enumerate(sc) if s > smax)
        _limit_cache[key] = (cand[below[0][1]] if below else None, -below[0][0] if below else None, cand[above[0][1]] if above else None, above[0][0] if above else None)
    return _limit_cache[key]


# what is known about the limit pairs from the penalties alone (checked by check_groups): no pair inside three chunks costs 238 under the default set
# (two gaps of 95 bases: 220), none inside any chunks has an edit distance of 253
LANE_NO_LIMIT_PAIR = {("edit", 3), ("default", 3)}
# ... and where every cost a pair this short can pay is even, an odd penalty is never a final one: (fit side, overflow side) instead of (255 - nH, 256 - nH).
# -a: 4, 4 + 2k; the deepest set: 4, 4 + 2k, and its second piece only pays from gaps of 85 bases on (88 + k < 4 + 2k), which cost more than the limit.
# (4, 6 + 8k, 20 + 8k) and (6, 6 + 8k, 40 + 2k): even as well.
LANE_LIMIT_PARITY = {("a22", 4): (248, 250), ("lane_deep", 4): (164, 166), ("e88", 3): (226, 228), ("f_e8", 3): (212, 214)}


def lane_candidates(orc, pen_name: str, chunks: int, s2: int):
    """[(kind, target, query)]: 60 - 320 bases.  Four chunks: 300 bp reads as well (the 2-bit form's 450 bases of target + query)."""
    seed = _seed("lane", pen_name)
    rng = np.random.default_rng(seed)
    out = []
    lens = (150, 149, 151, 160, 144, 128, 129, 200) + ((300, 301, 299, 320) if chunks == 4 else ())
    for i in range(36):      # reads at 0.5 ... 14 %: most fit, the diverged ones reach the last chunk or leave it
        L = lens[i % len(lens)]
        t, q = synth_pair(seed * 10 + i, L, 0.005 + 0.004 * i)
        if max(len(t), len(q)) > LANE_MAX_LEN:
            t, q = _cut(t, q, LANE_MAX_LEN)
        out.append(("related", t, q))
    t = _rand(rng, 257)
    out.append(("identical", t, t))
    out.append(("empty-target", b"", _rand(rng, 20)))
    out.append(("empty-query", _rand(rng, 17), b""))
    out.append(("homopolymer", b"A" * 150, b"A" * 139))
    unit = _rand(rng, 7)
    rep = (unit * 40)[:180]
    out.append(("tandem-indel", rep, rep[:90] + rep[90 + 7 + 3:]))
    out.append(("tandem-indel", rep, rep[:90] + unit[:4] + rep[90:]))
    for a, b in ((60, 64), (75, 70), (90, 95), (64, 60), (40, 44), (30, 27), (32 * chunks, 32 * chunks - 1)):   # unrelated: the matrix keeps their windows inside the chunks
        out.append(("unrelated", _rand(rng, a), _rand(rng, b)))
    for i in range(8):       # beyond the chunks: reads at 18 ... 40 %, unrelated reads
        t, q = _cut(*synth_pair(seed * 10 + 50 + i, (150, 300)[(i + (chunks == 4)) % 2], 0.18 + 0.03 * i), LANE_MAX_LEN)
        out.append(("over-related", t, q))
    out.append(("over-unrelated", _rand(rng, 230), _rand(rng, 240)))
    out.append(("over-unrelated", _rand(rng, 320), _rand(rng, 300)))
    if not s2:
        out.append(("non-acgt", *_mutate_non_acgt(*synth_pair(seed * 10 + 91, 150, 0.03))))
        out.append(("non-acgt", *_mutate_non_acgt(*synth_pair(seed * 10 + 92, 140, 0.06))))
    at, _, above, _ = lane_limit_pairs(orc, pen_name, chunks)
    if at is not None:
        out.append(("penalty-limit", *at))
    if above is not None:
        out.append(("over-penalty-limit", *above))
    return out


MID_MAX = 2000


def mid_anchor_len(pen_name: str) -> int:
    """Every mid batch of a run holds a pair of A x A bases and none longer on either side, so both groups' launches get the same span.  A: the longest pair
    of equal lengths, up to 2000 bases, that the host starts on the mid kernel under the set (a deep ring leaves a span that its rule about 0.34 of
    the length admits shorter pairs to)."""
    return next(L for L in range(MID_MAX, 399, -25) if mid_admits(PEN[pen_name], L, L))


def _mid_anchor(seed: int, p: float, A: int):
    return _cut(*synth_pair(seed, A + 60, p), A)


def mid_run_groups(pen_name: str) -> int:
    A = mid_anchor_len(pen_name)
    return mid_groups(PEN[pen_name], [(b"A" * A, b"A" * A)])


def mid_candidates(pen_name: str, s2: int):
    """[(kind, target, query)]: 400 - 2000 bases (and the short, empty and skewed shapes)."""
    seed = _seed("mid", pen_name)
    rng = np.random.default_rng(seed)
    A = mid_anchor_len(pen_name)
    out = [("related", *_mid_anchor(seed * 10, 0.004, A))]
    lens = (A * 3 // 5, A * 3 // 4 + 1, A - 1, A, max(401, A // 2 + 1), A * 4 // 5 + 1, max(400, A * 2 // 5), 447)
    for i in range(28):      # 0.5 ... 17 %: which of them fit depends on the set's span
        out.append(("related", *_cut(*synth_pair(seed * 10 + 1 + i, lens[i % len(lens)], 0.005 + 0.006 * i), A)))
    t = _rand(rng, 1024)
    out.append(("identical", t, t))
    for e in (500, 400, 300, 200):
        out.append(("empty-target", b"", _rand(rng, e)))
        out.append(("empty-query", _rand(rng, e + 1), b""))
    out.append(("homopolymer", b"A" * (A * 3 // 4), b"A" * (A * 3 // 5)))
    out.append(("homopolymer", b"A" * (A // 2), b"A" * (A // 2 - 40)))
    unit = _rand(rng, 7)
    rep = (unit * 200)[:min(1201, A)]
    out.append(("tandem-indel", rep, rep[:600] + rep[600 + 7 + 3:]))
    out.append(("tandem-indel", rep, rep[:600] + unit[:4] + rep[600:]))
    for a, b in ((450, 430), (400, 420), (300, 310), (200, 180), (700, 640)):
        out.append(("unrelated", _rand(rng, a), _rand(rng, b)))
    # length-skewed, related: the query is a mutated piece of the target (the gap fills of DESIGN 4.3); final penalties past 512: two shrinks
    for a, b in ((900, 100), (100, 900), (800, 100), (700, 100), (100, 700), (650, 60)):
        big = _rand(rng, max(a, b))
        small = synth_pair(seed * 10 + a + b, min(a, b), 0.03)
        piece = big[len(big) // 2:len(big) // 2 + min(a, b)]
        small_q = bytes(x if y == z else z for x, y, z in zip(piece, small[0][:len(piece)], small[1][:len(piece)]))   # the piece with synth_pair's substitutions
        out.append(("skewed", big, small_q) if a > b else ("skewed", small_q, big))
    for i in range(4):       # a long gap plus substitutions: the window drifts to one side
        t = _rand(rng, A * 9 // 10)
        g = 150 + 100 * i
        out.append(("long-gap", t, t[:600] + t[600 + g:]) if i % 2 else ("long-gap", t[:700] + t[700 + g:], t))
    for i in range(6):       # beyond the span of every set the LDS limits: 20 ... 45 %, and unrelated pairs of the longest admitted size
        out.append(("over-related", *_mid_anchor(seed * 10 + 70 + i, 0.20 + 0.05 * i, A)))
    for i in range(4):
        out.append(("over-unrelated", _rand(rng, A), _rand(rng, A - 7 * i)))
    if not s2:
        out.append(("non-acgt", *_mutate_non_acgt(*_cut(*synth_pair(seed * 10 + 91, A * 3 // 4, 0.03), A))))
        out.append(("non-acgt", *_mutate_non_acgt(*synth_pair(seed * 10 + 92, 600, 0.02))))
    return out


def _mid_near_limit(orc, p: dict, groups: int, t: bytes, q: bytes):
    """Cut a pair whose window leaves the span down to the longest prefix that stays inside it (a prefix's alignment is the pair's own up to the penalty at which
    it ends): its windows then end within one group of the span's edge.  Every step is judged by the oracle's trace of the cut pair."""
    lo_k, hi_k = 400, len(t)
    best = None
    for _ in range(12):
        k = (lo_k + hi_k) // 2
        cand = (t[:k], q[:max(1, k * len(q) // len(t))])
        (lohi, far), = _trace_all(orc, p, [cand])
        if mid_span_margin(groups, lohi, len(cand[0]), len(cand[1])) >= 0:
            lo_k, best = k, (cand, lohi, far)
        else:
            hi_k = k
        if hi_k - lo_k <= 1:
            break
    if best is None:
        return None
    cand, lohi, far = best
    ok = mid_admits(p, len(cand[0]), len(cand[1])) and mid_fits(p, groups, lohi, far, len(cand[0]), len(cand[1]))[1] and mid_span_margin(groups, lohi, len(cand[0]), len(cand[1])) < 64
    return (cand, lohi, far) if ok else None


def _mid_near_forecast(orc, p: dict, groups: int, t: bytes, q: bytes, far: np.ndarray):
    """Where the forecast, not the span, is what bounds the pairs the kernel keeps: cut a pair the forecast hands back down to the target length at which it
    passes by less than a group (the window it expects is proportional to the target length).  Judged by the oracle's trace of the cut pair."""
    cap, x = 64 * groups - 2 * nH(p) - 64, p["x"]
    for aim in (30, 45, 15, 55):
        tl_new, kmax = len(t), -1
        for s in (64, 256, 1024):
            if s + x - 1 >= len(far):
                break
            kmax = max(kmax, int(far[s + x - 1]))
            if kmax < 8:
                continue
            if kmax + 64 >= tl_new:   # (the cut pair ends before this penalty)
                break
            slack = 25 if s < 128 else 17 if s < 512 else 13
            tl_new = min(tl_new, max(kmax + 65, int((cap * slack / 10.5 - 16 - aim) * (kmax + 1) / (2 * s))))
        if tl_new >= len(t):
            return None
        cand = (t[:tl_new], q[:max(1, tl_new * len(q) // len(t))])
        if not mid_admits(p, len(cand[0]), len(cand[1])):
            continue
        (l2, f2), = _trace_all(orc, p, [cand])
        if mid_fits(p, groups, l2, f2, len(cand[0]), len(cand[1]))[1] and mid_forecast_margin(p, groups, f2, len(cand[0]), len(cand[1])) < 64:
            return cand, l2, f2
    return None


LANE_FIT_KINDS = ("related", "identical", "empty-target", "empty-query", "homopolymer", "tandem-indel", "unrelated", "near-limit")
MID_FIT_KINDS = LANE_FIT_KINDS + ("two-shrinks", "skewed-holds-all")
Groups = namedtuple("Groups", "fit over fit_kinds over_kinds n_exact_ok n_dropped near_limit span can_overflow")
_groups_cache: dict = {}


def build_groups(orc, kernel: str, pen_name: str, chunks: int, s2: int) -> Groups:
    """The fit and the overflow group of one (kernel, penalty set, chunks, sequence form) — the same for score-only and CIGAR, folded or not —
    from the oracle's band traces and the lengths alone.  span: lane_chunks, or the mid launch's groups."""
    key = (kernel, pen_name, chunks, s2)
    if key in _groups_cache:
        return _groups_cache[key]
    p = PEN[pen_name]
    fit, over, fk, ok, n_ok, n_drop, near = [], [], [], [], 0, 0, 0
    if kernel == "lane":
        cand = [c for c in lane_candidates(orc, pen_name, chunks, s2) if lane_admits(p, len(c[1]), len(c[2]))]
        tr = _trace_all(orc, p, [(t, q) for _, t, q in cand])
        for (kind, t, q), (lohi, far) in zip(cand, tr):
            good = lane_fits(p, chunks, lohi) and (is_acgt(t) and is_acgt(q) or not s2)
            n_ok += good
            if good:   # (a candidate meant for the overflow group that these penalties keep inside the chunks is a fit pair like any other)
                assert lane_tb_fits(p, chunks, lohi, len(t), len(q), 64)
                fit.append((t, q)), fk.append(kind[5:] if kind.startswith("over-") else kind)
                if lane_k_use(lohi) == chunks - 1 or len(lohi) > lane_s_max(p) - 32:   # within a chunk of the chunks' limit, or within 32 penalties of the shrink's
                    near += 1
                    fk.append("near-limit")
            elif is_acgt(t) and is_acgt(q) or not s2:
                over.append((t, q)), ok.append(kind)   # (a read diverged enough to leave the chunks)
        span, can_over = chunks, True
    else:
        span = mid_run_groups(pen_name)
        A = mid_anchor_len(pen_name)
        can_over = not mid_holds_everything(p, span, A, A)
        cand = [c for c in mid_candidates(pen_name, s2) if mid_admits(p, len(c[1]), len(c[2])) and max(len(c[1]), len(c[2])) <= A]
        tr = _trace_all(orc, p, [(t, q) for _, t, q in cand])
        nl = None
        for (kind, t, q), (lohi, far) in zip(cand, tr):   # the pair within a group of the limit: from the first related pair beyond it
            if nl is None and kind in ("related", "over-related", "long-gap") and mid_span_margin(span, lohi, len(t), len(q)) < 0:
                nl = _mid_near_limit(orc, p, span, t, q)
        if nl is None:   # ... or the first the forecast hands back inside the span
            for (kind, t, q), (lohi, far) in zip(list(cand), list(tr)):
                if nl is None and kind in ("related", "over-related") and mid_fits(p, span, lohi, far, len(t), len(q))[0] and mid_handed_back(p, span, lohi, far, len(t), len(q)):
                    nl = _mid_near_forecast(orc, p, span, t, q, far)
        if nl is not None:
            cand.append(("near-limit", *nl[0])), tr.append((nl[1], nl[2]))
        for (kind, t, q), (lohi, far) in zip(cand, tr):
            exact, good = mid_fits(p, span, lohi, far, len(t), len(q))
            if mid_handed_back(p, span, lohi, far, len(t), len(q)):
                over.append((t, q)), ok.append(kind)
                continue
            n_ok += 1
            n_drop += not good
            if good:
                fit.append((t, q)), fk.append(kind[5:] if kind.startswith("over-") else kind)
                if mid_span_margin(span, lohi, len(t), len(q)) < 64 or mid_forecast_margin(p, span, far, len(t), len(q)) < 64:
                    near += 1
                    fk.append("near-limit")
                if len(lohi) > 512:
                    fk.append("two-shrinks")
                if kind == "skewed" and mid_admits(p, len(t), len(q)) == "holds_all":
                    fk.append("skewed-holds-all")
        # (both batches hold a pair of the anchor's size, so both launches get the span the groups were sized for)
        assert mid_groups(p, fit) == span and (not over or not can_over or mid_groups(p, over) == span), (pen_name, span)
    G = Groups(fit, over, fk, ok, n_ok, n_drop, near, span, can_over)
    _groups_cache[key] = G
    return G


MIN_FIT, MIN_OVER = 16, 4


def check_groups(kernel: str, pen_name: str, chunks: int, s2: int, G: Groups, label: str) -> str:
    """Assert what tests/test_lane_mid_matrix_gpu.py relies on; returns the line it reports."""
    p = PEN[pen_name]
    unit = "chunk" if kernel == "lane" else "group"
    line = (f"{label}: span {G.span} {unit}s, fit {len(G.fit)} (within one {unit} of the limit: {G.near_limit}), overflow {len(G.over)}, "
            f"forecast margin dropped {G.n_dropped} of {G.n_exact_ok}")
    assert len(G.fit) >= MIN_FIT, line
    assert G.n_dropped <= MAX_DROPPED_SHARE * G.n_exact_ok and (kernel == "mid" or G.n_dropped == 0), line
    kinds = (LANE_FIT_KINDS if kernel == "lane" else MID_FIT_KINDS) + (("non-acgt",) if not s2 else ())
    if G.can_overflow:
        assert len(G.over) >= MIN_OVER and G.near_limit >= 1, line
    else:   # the LDS holds a span over every column a 2 kb pair's window can reach under this set: nothing can be handed back, and there is no limit to be near
        assert not G.over, line
        kinds = tuple(k for k in kinds if k != "near-limit")
        line += " (the span holds every window: no overflow group)"
    for k in kinds:
        assert k in G.fit_kinds, (line, "no fit pair of kind", k)
    if kernel == "lane":
        assert lane_group_admits(p, chunks, s2, G.fit) and lane_group_admits(p, chunks, s2, G.over), line
        assert all(lane_admits(p, len(t), len(q)) for t, q in G.fit + G.over), line
        if (pen_name, chunks) in LANE_NO_LIMIT_PAIR:
            assert "penalty-limit" not in G.fit_kinds, line
        else:
            assert "penalty-limit" in G.fit_kinds and "over-penalty-limit" in G.over_kinds, (line, "no pair at the penalty limit")
            _, s_at, _, s_above = _limit_cache[(pen_name, chunks)]
            assert (s_at, s_above) == LANE_LIMIT_PARITY.get((pen_name, chunks), (lane_s_max(p), lane_s_max(p) + 1)), (line, s_at, s_above)
    else:
        assert all(mid_admits(p, len(t), len(q)) for t, q in G.fit + G.over), line
    return line


def run_key(c: Cell, pen_name: str):
    return (c.kernel, pen_name, c.chunks, c.inst.S2)


def self_check(orc, log=print):
    """Every cell's inputs, built and checked on the CPU."""
    for c in MATRIX:
        for pen_name, bf in c.runs:
            k = run_key(c, pen_name)
            log(check_groups(*k, build_groups(orc, *k), f"{c.kernel} {pen_name} {'chunks %d ' % c.chunks if c.chunks else ''}S2 {c.inst.S2}"))


# ---- what a batch under DEFAULT routing may hand back (the existing fuzz tests) ----------------------------------------------------------
def may_hand_back(orc, pairs, opt_kw: dict, lane_chunks: int = 0) -> int:
    """An upper bound for n_retries of a batch of at most as many pairs as the device has CUs, known to the host byte for byte, under the default routing and
    default tunables but lane_chunks, mid_block, seq2bit and div_aware 0: a pair the host starts on the lane kernel (up to 320 bases in such a batch) or on the mid kernel counts when
    the rules above say that kernel hands it back — once: what the lane kernel hands back in such a batch is re-run on the mid kernel, whose span then holds every column
    of a pair that short.  What the mid kernel hands back, and every pair neither kernel starts, goes to the band classes, whose hand-backs are tests/band_matrix.py's
    matter: a pair can be re-run on a wider geometry and then on the generic kernel, so these count three times.
    Score and CIGAR alike (the traceback arena is the default's: the device's memory).  Not for stop rules (max_s, max_iter)."""
    p = dict(PEN["default"])
    p.update({k: v for k, v in opt_kw.items() if k in p})
    lane_idx = [i for i, (t, q) in enumerate(pairs) if lane_admits(p, len(t), len(q)) and max(len(t), len(q)) <= 320]
    lane_i = set(lane_idx)
    mid_idx = [i for i, (t, q) in enumerate(pairs) if i not in lane_i and mid_admits(p, len(t), len(q))]
    tr = _trace_all(orc, p, pairs)
    n = 3 * (len(pairs) - len(lane_idx) - len(mid_idx))
    if lane_idx:
        lp = [pairs[i] for i in lane_idx]
        chunks = lane_chunks if lane_chunks > 0 else 3   # (lane_chunks 0: three or four by the launch's longest pair — and the pairs the host knows not to be A/C/G/T get a launch of their own: the bound takes three)
        if lane_lds_bytes(p, chunks, _group_seq_lds(lp)) > 60 * 1024:
            n += len(lane_idx)
        else:
            n += sum(not lane_fits(p, chunks, tr[i][0]) for i in lane_idx)
    if mid_idx:
        mp = [pairs[i] for i in mid_idx]
        g = mid_groups(p, mp)
        n += 3 * sum(not mid_fits(p, g, tr[i][0], tr[i][1], len(pairs[i][0]), len(pairs[i][1]))[1] for i in mid_idx)   # (within 5 % of a forecast's threshold: may)
    return n
