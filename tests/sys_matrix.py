"""The instantiations of the whole-device kernel (miniwfa_amd/csrc/mwf_sys_pass.h: wfa_sys_kernel<E1, E2, P, DEFER, TB, C> and the provenance pass
wfa_sys_seg_kernel<E1, E2, P, DEFER, C>, instantiated by mwf_sys.hip and mwf_sys_deep.hip; 48 in all), one entry each, with what reaches it — tunables, mode,
penalty sets — the launch records every run must print, and the inputs of its test groups, sized on the CPU from the oracle alone.  The structure is
tests/lane_mid_matrix.py's.

  tests/test_sys_matrix_cpu.py   the set of entries EQUALS the instantiations in the two built objects; every cell has its inputs (self_check); the oracle
                                 reproduces tests/golden/sys_pen.jsonl (the compiled reference under the penalty sets used here)
  tests/test_sys_matrix_gpu.py   one test per entry and penalty set: the launch records (MWF_DEBUG, `sys launch:`) are exactly the sequence this table states, the *fit*
                                 group is finished without a re-run, the *overflow* group is launched again on four columns per lane, every answer equals
                                 the oracle's; and the edge tests

Rule: an instantiation is added or removed together with its entry here.

Which instantiation a launch takes (launch_pass_d ... launch_pass_pc, restated by `records`):
  E1, E2  the penalties' gap extensions; P = 8 (the one block length the product build has)
  C       columns per lane: the tunable sys_c, or with sys_c 0 the host's choice per pass (run_coop_group's c_first / c_second, restated by auto_c)
  DEFER   x >= 3 && o1 + e1 >= 3 && o2 + e2 >= 3, for e1 == 2 only — but never with traceback on four columns per lane, and never in the provenance pass
  TB      the pass stores traceback: flag 1, every pass but the provenance pass
  SEG     the provenance pass of the two-pass low-memory mode (coop_pass 3)
Modes (what a run sets besides its route) and the passes they launch, in order:
  score    flag 0                                              pass 0
  cigar    flag 1                                              pass 0
  walk     flag 1, step STEP, a budget the walk's arena fits   pass 1, pass 2
  twopass  flag 1, step STEP, lowmem_budget_mb 1               pass 3 (SEG), pass 2
(Which form of the low-memory mode a launch takes is the host's rule on the arena the walk would need against lowmem_budget_mb — two_pass_rule below.  Under the
default budget of 8 GB sixteen pairs side by side already take the two-pass form, whatever their lengths: the walk runs set a budget of WALK_BUDGET_MB so that
both routes launch passes 1 and 2.)
Routes, in tunables only: force_kind 1, sys_c as the cell says, div_aware 0, and
  alone         coop_grid 16: every pair is launched by itself on 16 workgroups (256 chunk slots)
  side by side  the default grid: up to n_cu / 16 pairs of these lengths per launch, each on 16 workgroups (side_by_side restates route_whole_device)

fit = none of the kernel's hand-backs fires, each restated on the oracle's band trace (Oracle.band_trace_far) and the pair's lengths, never on what the device did:
  chunks     at the start of every epoch of 256 penalties, the chunks whose owned columns (64 C - 2 P) meet the window widened by 257 + P either side number at
             most TC - 1 (mwf_sys_pass.h, `n_ep > TC - 1`).  The trace gives every new slice's lo = max(wf_lo - 1, 1) and hi: the window a column wider than the
             kernel's, so the count is never below the kernel's.  A pair within one chunk of the limit joins neither group.
  snapshots  (two-pass runs) the provenance pass's snapshots — nH + 2 e1 + 2 e2 array-slices of the epoch's chunks, one every STEP penalties — fit the arena the
             host sizes from the pair's lengths (run_coop_group's snap_slot_ints): a pair that outgrows it is run again with twice the arena, which is a re-run.
             Unrelated pairs and pairs under the 256-row sets outgrow it; they are left out of the two-pass runs' group, and counted.
Pairs left out of a group by a margin are counted and bounded by band_matrix.MAX_DROPPED_SHARE; for the C = 4 cells the chunks rule drops none (asserted).
overflow (C = 1 cells only; sys_c 0, div_aware 0, coop_grid 16): pairs for which the host's estimate picks 64-column slots (auto_c) and whose window, by the
chunks rule on a window a column NARROWER than the trace's, outgrows 255 of them but not 255 of the 256-column ones: the first record is the cell's instantiation,
n_retries equals the group's size, each pair is launched again on the C = 4 twin, nothing is re-run on one workgroup.
C = 4 cells have no overflow group: the smallest pair that outgrows 16 workgroups of 256-column slots has a window near 60 k columns (255 x 240), which is no
few-second test."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import fuzz_pairs, random_seq, skewed_pairs, synth_pair
from band_matrix import MAX_DROPPED_SHARE, _trace_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYS_OBJS = (os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_sys.hip.o"), os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_sys_deep.hip.o"))

SysInst = namedtuple("SysInst", "E1 E2 P DEFER TB C SEG")
P_BLOCK = 8          # sys_p_supported: the product build instantiates one block length
K_EPOCH = 256
MAX_RING = 256       # mwf_internal.h kMaxRing: coop_supported admits nH <= 256
TC = 256             # chunk slots of 16 workgroups: 8 waves x 2 slots each (sys_chunk_slots)
GROUP_WG = 16
STEP = 97            # the low-memory runs' step: a snapshot in almost every pair
WALK_BUDGET_MB = 1 << 16


def inst_id(i: SysInst) -> str:
    return f"sys-E{i.E1}{i.E2}-{'seg' if i.SEG else 'TB%d' % i.TB}-{'defer' if i.DEFER else 'plain'}-C{i.C}"


# ---- penalty sets -----------------------------------------------------------------------------------------------------------------------
PEN = {
    # (2,1)
    "default": dict(x=4, o1=4, e1=2, o2=15, e2=1),        # deferred
    "x2": dict(x=2, o1=4, e1=2, o2=15, e2=1),             # plain via x
    "oe2_2": dict(x=4, o1=4, e1=2, o2=1, e2=1),           # plain via o2 + e2
    "o1zero": dict(x=3, o1=0, e1=2, o2=12, e2=1),         # plain; the first piece's open lag equals its extension lag
    "xdeep": dict(x=30, o1=2, e1=2, o2=10, e2=1),         # deferred, the ring's depth set by x
    "ring256_21": dict(x=4, o1=4, e1=2, o2=254, e2=1),    # deferred, nH 256
    # (2,2)
    "a22": dict(x=4, o1=4, e1=2, o2=4, e2=2),             # main.c's -a preset; deferred
    "d22": dict(x=4, o1=4, e1=2, o2=24, e2=2),            # deferred
    "x2_22": dict(x=2, o1=4, e1=2, o2=24, e2=2),          # plain
    "open0_22": dict(x=4, o1=0, e1=2, o2=0, e2=2),        # plain, both opens 0
    "ring256_22": dict(x=4, o1=4, e1=2, o2=253, e2=2),    # deferred, nH 256
    # (1,1): never deferred
    "edit": dict(x=1, o1=0, e1=1, o2=0, e2=1),            # every lag 1, a ring of two
    "e11": dict(x=3, o1=3, e1=1, o2=9, e2=1),
    "xring_11": dict(x=6, o1=2, e1=1, o2=4, e2=1),        # the ring's depth set by x
    "ring256_11": dict(x=4, o1=4, e1=1, o2=254, e2=1),    # nH 256
    # the deep sets (mwf_sys_deep.hip): never deferred
    "e31": dict(x=4, o1=6, e1=3, o2=26, e2=1),
    "o1zero_31": dict(x=4, o1=0, e1=3, o2=10, e2=1),
    "ring256_31": dict(x=4, o1=6, e1=3, o2=254, e2=1),
    "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2),
    "xdeep_32": dict(x=40, o1=2, e1=3, o2=10, e2=2),
    "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1),
    "oe2_3_41": dict(x=4, o1=10, e1=4, o2=2, e2=1),
    "e42": dict(x=2, o1=4, e1=4, o2=24, e2=2),
    "ring256_42": dict(x=4, o1=4, e1=4, o2=253, e2=2),
}
RING256 = tuple(k for k in PEN if k.startswith("ring256"))
# just beyond the limit: o2 one higher than each 256-row set (nH 257) — refused under force_kind 1, the generic kernel's under default routing
PEN_BEYOND = {k.replace("ring256", "ring257"): dict(PEN[k], o2=PEN[k]["o2"] + 1) for k in RING256}
EXTS = ((2, 1), (2, 2), (1, 1), (3, 1), (3, 2), (4, 1), (4, 2))


def nH(p: dict) -> int:
    """mwf_plan.cpp make_penalty: the H ring's depth."""
    return max(p["x"], p["o1"] + p["e1"], p["o2"] + p["e2"]) + 1


def ext(p: dict):
    return p["e1"], p["e2"]


def coop_supported(p: dict) -> bool:
    return ext(p) in EXTS and nH(p) <= MAX_RING


def defers(p: dict) -> bool:
    """launch_pass_d: DEFER needs every H lag >= 3, and is built for e1 == 2 only."""
    return p["e1"] == 2 and p["x"] >= 3 and p["o1"] + p["e1"] >= 3 and p["o2"] + p["e2"] >= 3


def sets_of(e) -> tuple:
    return tuple(k for k, p in PEN.items() if ext(p) == e)


assert {ext(p) for p in PEN.values()} == set(EXTS) and all(coop_supported(p) for p in PEN.values())
assert [k for k in PEN if defers(PEN[k])] == ["default", "xdeep", "ring256_21", "a22", "d22", "ring256_22"]
assert all(nH(PEN[k]) == 256 for k in RING256) and {ext(PEN[k]) for k in RING256} == {(2, 1), (2, 2), (1, 1), (3, 1), (4, 2)}
assert all(nH(p) == 257 and not coop_supported(p) for p in PEN_BEYOND.values()) and len(PEN_BEYOND) == 5
assert max(nH(p) for k, p in PEN.items() if k not in RING256) == 41 and nH(PEN["edit"]) == 2 and nH(PEN["xdeep"]) == 31 and nH(PEN["xring_11"]) == 7
assert nH(PEN["xdeep"]) == PEN["xdeep"]["x"] + 1 and nH(PEN["xdeep_32"]) == PEN["xdeep_32"]["x"] + 1   # rings whose depth comes from x
assert [k for k, p in PEN.items() if p["o1"] == 0] == ["o1zero", "open0_22", "edit", "o1zero_31"]


# ---- which instantiation a pass launches, restated --------------------------------------------------------------------------------------
MODES = ("score", "cigar", "walk", "twopass")


def _inst(p: dict, tb: int, c: int, seg: int = 0) -> SysInst:
    d = defers(p) and not seg and not (tb and c == 4)
    return SysInst(p["e1"], p["e2"], P_BLOCK, int(d), tb, c, seg)


def records(p: dict, mode: str, c_first: int, c_second: int):
    """[(instantiation, pass)] of one launch group in `mode`: the exact sequence of `sys launch:` records."""
    if mode == "score":
        return [(_inst(p, 0, c_first), 0)]
    if mode == "cigar":
        return [(_inst(p, 1, c_first), 0)]
    if mode == "walk":
        return [(_inst(p, 1, c_first), 1), (_inst(p, 1, c_second), 2)]
    assert mode == "twopass"
    return [(_inst(p, 0, c_first, 1), 3), (_inst(p, 1, c_second), 2)]


def mode_opt(mode: str) -> dict:
    return dict(flag=0 if mode == "score" else 1, step=STEP if mode in ("walk", "twopass") else 0)


def mode_tunables(mode: str):
    return (("lowmem_budget_mb", 1),) if mode == "twopass" else (("lowmem_budget_mb", WALK_BUDGET_MB),) if mode == "walk" else ()


def route_tunables(route: str, c: int):
    return (("force_kind", 1), ("sys_c", c), ("div_aware", 0)) + ((("coop_grid", GROUP_WG),) if route == "alone" else ())


ROUTES = ("alone", "side")


# ---- the host's rules, restated (mwf_plan.cpp run_coop_group, route_whole_device) -----------------------------------------------------------
def owned_cols(c: int) -> int:
    return 64 * c - 2 * P_BLOCK


def window_cap(c: int, tc: int = TC) -> int:
    return (tc - 4) * owned_cols(c) - 2 * (257 + P_BLOCK)


def est1(ln: int) -> int:
    """The first pass's expected window with div_aware 0: a fifth of tl + ql, at least 8192, at most every column."""
    return min(ln + 1, max(8192, ln // 5))


def est2(p: dict, ln: int, step: int) -> int:
    """The second pass's: the band collapses at every checkpoint."""
    return min(ln + 1, 2 * (step + 2 * nH(p)) + 8)


def auto_c(p: dict, ln: int, step: int):
    """(c_first, c_second) with sys_c 0 on 16 workgroups."""
    return (1 if est1(ln) <= window_cap(1) else 4), (1 if est2(p, ln, step) <= window_cap(1) else 4)


def two_pass_rule(ln: int, n_groups: int, c_first: int, budget_mb: int) -> bool:
    budget = (budget_mb << 20) if budget_mb > 0 else 8 << 30
    return max(1 << 30, 6000 * ln) * n_groups * (12 if c_first == 1 else 9) // 8 > budget


def coop_group_size(n_cu: int, ln: int, alone: bool, ow: int = 240) -> int:
    G = n_cu
    chunks = ln // ow + (3 if ow == 256 else 8) if alone else ln // ow // 3 + (8 if ow == 256 else 12)
    while G > (64 if alone else 16) and chunks <= (G // 2) * 16:
        G //= 2
    return G


def side_by_side(lens, n_cu: int):
    """[(pairs in the launch, workgroups per pair)] of route_whole_device: longest first, as many side by side as the device holds groups of the longest one's size."""
    lens = sorted(lens, reverse=True)
    out, at = [], 0
    while at < len(lens):
        if n_cu <= GROUP_WG:   # coop_grid 16: one pair at a time
            out.append((1, coop_group_size(n_cu, lens[at], True)))
            at += 1
            continue
        gs = coop_group_size(n_cu, lens[at], False)
        n = min(len(lens) - at, max(1, n_cu // gs))
        out.append((1, coop_group_size(n_cu, lens[at], True)) if n <= 1 else (n, gs))
        at += n
    return out


def snap_slot_ints(p: dict, ln: int, step: int) -> int:
    """The snapshot arena of one pair in a launch whose longest pair has `ln` bases of target + query (coop_tb_mult 1: a fresh engine)."""
    NS = nH(p) + 2 * p["e1"] + 2 * p["e2"]
    n_guess = (ln * 3 // 100 + 1024) // step + 2
    cols = sum(min(ln + 1, 2 * j * step) + 1100 for j in range(1, n_guess + 1))
    return min(max(4 << 20, NS * cols), (48 << 30) // 4) // 4 * 4


# ---- the kernel's hand-backs, restated on the oracle's band trace (lohi: diagonals lo, hi of every new slice; column = diagonal + tl + 1) ----------
def epoch_chunks(lohi: np.ndarray, tl: int, ql: int, c: int, narrow: int = 0):
    """Chunks that take part in every epoch the pass starts (sys_pass: gA, gB, n_ep).  The window at the start of the epoch behind penalty s is the trace's
    slice of penalty s + 1 taken a column narrower either side (wf_lo - 1 = lo unless lo sits on the matrix' edge): narrow 0 counts with the trace's
    own lo, hi (never fewer chunks than the kernel), narrow 1 with lo + 1, hi - 1 (never more)."""
    ow, cmax, s_final = owned_cols(c), tl + ql + 1, len(lohi)
    gmax, out = cmax // ow, []
    for s in range(0, s_final + 1, K_EPOCH):
        if s == 0:
            wl = wh = tl + 1
        elif s < s_final:
            wl, wh = int(lohi[s][0]) + tl + 1 + narrow, int(lohi[s][1]) + tl + 1 - narrow
        elif narrow:
            break          # (whether an epoch starts behind the final penalty is the kernel's matter: not counted for "certainly overflows")
        else:
            wl, wh = int(lohi[s - 1][0]) + tl + 1 - 1, int(lohi[s - 1][1]) + tl + 1 + 1
        gA = max(0, (wl - (K_EPOCH + 1 + P_BLOCK)) // ow)     # (Python's // is the kernel's floordiv)
        gB = min(gmax, (wh + K_EPOCH + 1 + P_BLOCK) // ow)
        out.append(gB - gA + 1)
    return out


def chunks_fit(lohi, tl, ql, c, margin=1) -> bool:
    return max(epoch_chunks(lohi, tl, ql, c)) <= TC - 1 - margin


def chunks_overflow(lohi, tl, ql, c) -> bool:
    """For certain."""
    return max(epoch_chunks(lohi, tl, ql, c, narrow=1)) > TC - 1


def snap_need(p: dict, lohi, tl, ql, c, step: int) -> int:
    """ints of snapshots the provenance pass writes: per epoch, (snapshots due in it) x (nH + 2 e1 + 2 e2) x (chunks x owned columns).  The pass acts on the end
    cell at the epoch's end, so the final epoch counts in full."""
    NS, ow, need, nxt = nH(p) + 2 * p["e1"] + 2 * p["e2"], owned_cols(c), 0, step - 1
    for k, n_ep in enumerate(epoch_chunks(lohi, tl, ql, c)):
        s = k * K_EPOCH
        n_snap = (s + K_EPOCH - 1 - nxt) // step + 1 if nxt <= s + K_EPOCH - 1 else 0
        need += n_snap * NS * n_ep * ow
        nxt += n_snap * step
    return need


def snap_fit(p, lohi, tl, ql, c, step=STEP) -> bool:
    return snap_need(p, lohi, tl, ql, c, step) <= snap_slot_ints(p, tl + ql, step)   # (no margin: epoch_chunks never counts fewer chunks than the kernel, and only the provenance pass takes snapshots)


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
# Cell: instantiation, runs ((penalty set, mode) — each run's launches must be exactly records(set, mode, C, C), on both routes).
# The sets are dealt so that every cell runs at least two sets, every set runs score-only on both C and in cigar, walk and twopass at least once:
#   TB0 cells       every set of the cell's DEFER, score
#   TB1 C1 cells    every set of the cell's DEFER: twopass (its second pass), and cigar / walk by the set's turn — a deferred set both: its traceback passes on
#                   four columns per lane are the plain form's, launched by the TB0 defer C4 cell's CIGAR twin and by the seg C4 cell's second passes
#   TB1 C4 cells    every set that is not deferred: twopass, and walk / cigar the other way round
#   seg cells       twopass (its first pass) under the first half of the extensions' sets on one column per lane, the second half on four; two sets at least
# (A cell run by itself pays the oracle's traces and answers of its sets: no cell has more than four.)
# over: the (set, mode) of the cell's overflow group (C = 1 cells) — its first run that is not under the edit set (whose windows stay too narrow for pairs of a few
# kb to outgrow 255 slots) and, for a traceback cell, not the two-pass form (whose first launch is the seg cell's).
Cell = namedtuple("Cell", "inst runs over")


def _cell(inst: SysInst, runs) -> Cell:
    over = None
    if inst.C == 1:
        over = next(r for r in runs if r[0] != "edit" and (r[1] != "twopass" or inst.SEG))
    return Cell(inst, tuple(runs), over)


def _matrix():
    cells = []
    for e in EXTS:
        names = sets_of(e)
        turn = {n: i % 2 for i, n in enumerate(names)}
        for d in ((0, 1) if e[0] == 2 else (0,)):
            mine = tuple(n for n in names if defers(PEN[n]) == bool(d))
            for c in (1, 4):
                cells.append(_cell(SysInst(*e, P_BLOCK, d, 0, c, 0), tuple((n, "score") for n in mine)))
            cells.append(_cell(SysInst(*e, P_BLOCK, d, 1, 1, 0), tuple((n, m) for n in mine for m in (("twopass", "cigar", "walk") if d else ("twopass", "walk" if turn[n] else "cigar")))))
            if not d:
                cells.append(_cell(SysInst(*e, P_BLOCK, 0, 1, 4, 0), tuple((n, m) for n in names if not defers(PEN[n]) for m in ("twopass", "cigar" if turn[n] else "walk"))))
        half = max(2, (len(names) + 1) // 2)
        for c, part in ((1, names[:half]), (4, names[-half:])):
            cells.append(_cell(SysInst(*e, P_BLOCK, 0, 0, c, 1), tuple((n, "twopass") for n in part)))
    return cells


MATRIX = _matrix()


def cell_id(c: Cell) -> str:
    return inst_id(c.inst)


def declared_instantiations() -> set:
    return {c.inst for c in MATRIX}


assert len(MATRIX) == len(declared_instantiations()) == 48
assert [sum(ext(PEN[c.runs[0][0]]) == e for c in MATRIX) for e in EXTS] == [9, 9, 6, 6, 6, 6, 6]
for _c in MATRIX:   # a run's penalties and mode force the entry; every cell runs two sets and more
    assert len({n for n, _ in _c.runs}) >= 2, cell_id(_c)
    for _n, _m in _c.runs:
        assert _c.inst in [i for i, _ in records(PEN[_n], _m, _c.inst.C, _c.inst.C)], (cell_id(_c), _n, _m)
assert not any(c.inst.DEFER and c.inst.TB and c.inst.C == 4 for c in MATRIX)   # the deferred traceback form is reached with C = 1 only
for _n in PEN:      # every set: score-only on both C, and every other mode at least once
    _seen = {(m, c.inst.C) for c in MATRIX for n, m in c.runs if n == _n}
    assert {("score", 1), ("score", 4)} <= _seen and {m for m, _ in _seen} == set(MODES), (_n, _seen)
assert max(len({n for n, _ in c.runs}) for c in MATRIX) <= 4


# ---- the instantiations of the built objects --------------------------------------------------------------------------------------------
def object_instantiations():
    """{SysInst} parsed from the two objects' symbol tables (llvm-readelf -sW | c++filt: demangled kernel names only), or a string saying why that cannot
    be done here."""
    import shutil
    import subprocess
    readelf = next((p for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf") or "") if p and os.path.exists(p)), None)
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not readelf or not cxxfilt:
        return "llvm-readelf or c++filt not found"
    out = set()
    for obj in SYS_OBJS:
        if not os.path.exists(obj):
            return "no " + os.path.relpath(obj, ROOT) + " (the library was not built from this tree)"
        syms = subprocess.run([readelf, "-sW", obj], check=True, capture_output=True, text=True).stdout
        dem = subprocess.run([cxxfilt], input=syms, check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"wfa_sys(_seg)?_kernel<([^<>]*)>", dem):
            vals = []
            for a in m.group(2).split(","):
                a = re.sub(r"^\(\w+\)", "", a.strip()).strip("()")
                vals.append({"true": 1, "false": 0}[a] if a in ("true", "false") else int(a) if re.fullmatch(r"-?\d+", a) else None)
            assert None not in vals and len(vals) == (5 if m.group(1) else 6), m.group(0)
            out.add(SysInst(vals[0], vals[1], vals[2], vals[3], 0, vals[4], 1) if m.group(1) else SysInst(*vals, 0))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _seed(pen_name: str) -> int:
    return 810000 + 1000 * sorted(PEN).index(pen_name)


def _disjoint(tl: int, ql: int):
    """Sequences with no base in common (A/C against G/T): no match anywhere — the penalty follows from the lengths."""
    r = np.random.default_rng(tl * 1000 + ql)
    return (np.frombuffer(b"AC", dtype=np.uint8)[r.integers(0, 2, tl)].tobytes(), np.frombuffer(b"GT", dtype=np.uint8)[r.integers(0, 2, ql)].tobytes())


def spaced_subs(L: int, k: int, seed: int = 5):
    """A pair of L bases with k substitutions spaced evenly (further apart than any gap could pay for): the penalty is k x."""
    t = bytearray(random_seq(seed + L, L))
    q = bytearray(t)
    for i in range(k):
        at = (2 * i + 1) * L // (2 * k)
        q[at] = b"ACGT"[(b"ACGT".index(t[at]) + 1) % 4]
    return bytes(t), bytes(q)


def candidates(pen_name: str):
    """[(kind, target, query)]: 0 - 6 kb, one 9 kb pair, one unrelated 5200 x 3900 pair."""
    seed = _seed(pen_name)
    out = [("fuzz", t, q) for t, q in fuzz_pairs(seed, 8, 3000)]
    out += [("skewed", t, q) for t, q in skewed_pairs(seed + 3, 3, 200, 3000)]
    a = random_seq(seed + 10, 2500)
    out += [("identical", a, a), ("empty", b"", b""), ("empty", b"", a[:700]), ("empty", a[:900], b""), ("one-base", b"A", b"C"), ("one-base", b"G", b"G"),
            ("piece", a, a[:300]), ("piece", a[2000:], a),
            ("homopolymer", b"A" * 1500, b"A" * 1390), ("homopolymer", b"C" * 700, b"G" * 640)]
    unit = random_seq(seed + 14, 7)
    rep = (unit * 200)[:1201]
    out += [("tandem-indel", rep, rep[:600] + rep[600 + 7 + 3:]), ("tandem-indel", rep, rep[:600] + unit[:4] + rep[600:])]
    out.append(("unrelated-corners", random_seq(seed + 11, 5200), random_seq(seed + 12, 3900)))
    out.append(("long-indels", *synth_pair(seed + 21, 9000, 0.1, 2, 500)))
    out.append(("related", *synth_pair(seed + 20, 6000, 0.04)))
    for i, n in enumerate((47, 48, 49, 239, 240, 241, 255, 256)):    # target length + 1 on slot ownership and chunk edges
        out.append(("edge-length", *synth_pair(seed + 30 + i, n - 1, 0.08)))
    if pen_name in RING256:   # ends below penalty 256 (the ring never wraps) / beyond 600 (it wraps twice)
        out.append(("ring-no-wrap", *synth_pair(seed + 40, 400, 0.03)))
        out.append(("ring-wraps-twice", *synth_pair(seed + 41, 2500, 0.12)))
    return out


def overflow_candidates(pen_name: str):
    """Unrelated pairs of 7.5 - 8 kb (9 - 9.6 kb where x < 3): about the smallest whose windows outgrow 255 slots of 48 owned columns (the oracle's time grows with the square of the penalty:
    unrelated 9 kb pairs cost half as much again, diverged 20 kb pairs six times as much)."""
    seed = _seed(pen_name)
    base = 7500 if PEN[pen_name]["x"] >= 3 else 9000   # (a mismatch cost of 2 keeps an unrelated pair's window narrower)
    return [(random_seq(seed + 61 + 2 * i, base + 120 * i), random_seq(seed + 62 + 2 * i, base + 100 + 70 * i)) for i in range(6)]


FIT_KINDS = ("fuzz", "skewed", "identical", "empty", "one-base", "piece", "homopolymer", "tandem-indel", "unrelated-corners", "long-indels", "related", "edge-length")
MIN_FIT, MIN_FIT_TWOPASS, MIN_OVER = 24, 16, 4
WIDE_TWOPASS_EXTS = ((2, 1), (2, 2), (1, 1), (3, 1))
LONG_INDELS_NEAR_LIMIT = ("e31", "e41")   # (4,6,3,26,1) and (4,6,4,26,1): dear first pieces keep more diagonals alive
# The overflow group's two-pass runs: a step at which the snapshots of an unrelated pair fit the arena the host sizes from the lengths (snap_fit: a few snapshots of
# every column), and a traceback budget that holds the second pass's rows between checkpoints that far apart — so that the only re-run is the one on four columns.
OVER_STEP, OVER_TB_BUDGET_MB = 4000, 4096
Groups = namedtuple("Groups", "fit fit_kinds idx twopass n_cand n_dropped n_dropped_twopass s_final width")
_groups_cache: dict = {}
_trace_cache: dict = {}


def build_groups(orc, pen_name: str, c: int) -> Groups:
    """The fit group of one (penalty set, columns per lane) — every mode's but twopass's — and the indices of the fit pairs the two-pass runs keep, from the
    oracle's band traces and the lengths alone.  idx: the fit pairs' places among candidates(pen_name), whose oracle answers both C share; width: every fit pair's widest window."""
    key = (pen_name, c)
    if key in _groups_cache:
        return _groups_cache[key]
    p = PEN[pen_name]
    if pen_name not in _trace_cache:   # (one trace per candidate, for both C)
        cand = candidates(pen_name)
        _trace_cache[pen_name] = (cand, _trace_all(orc, p, [(t, q) for _, t, q in cand]))
    cand, tr = _trace_cache[pen_name]
    fit, kinds, idx, two, s_final, width, n_drop = [], [], [], [], [], [], 0
    for j, ((kind, t, q), (lohi, _)) in enumerate(zip(cand, tr)):
        if not chunks_fit(lohi, len(t), len(q), c):
            assert not chunks_overflow(lohi, len(t), len(q), 4), (pen_name, kind)   # (nothing here outgrows the 256-column slots)
            n_drop += 1
            continue
        if snap_fit(p, lohi, len(t), len(q), c):
            two.append(len(fit))
        fit.append((t, q)), kinds.append(kind), idx.append(j), s_final.append(len(lohi)), width.append(int((lohi[:, 1] - lohi[:, 0]).max()) + 1 if len(lohi) else 1)
    G = Groups(fit, kinds, idx, two, len(cand), n_drop, len(fit) - len(two), s_final, width)
    _groups_cache[key] = G
    return G


def check_groups(pen_name: str, c: int, G: Groups) -> str:
    """Assert what tests/test_sys_matrix_gpu.py relies on; returns the line it reports."""
    line = (f"{pen_name} C {c}: {G.n_cand} candidates, fit {len(G.fit)} (two-pass runs keep {len(G.twopass)}), within a chunk of the limit or beyond {G.n_dropped}, "
            f"left out of the two-pass runs by the snapshot arena {G.n_dropped_twopass}, penalties up to {max(G.s_final)}")
    assert MIN_FIT <= len(G.fit) <= 40 and len(G.twopass) >= MIN_FIT_TWOPASS, line
    assert G.n_dropped <= MAX_DROPPED_SHARE * G.n_cand and (c == 1 or G.n_dropped == 0), line
    assert G.n_dropped_twopass <= MAX_DROPPED_SHARE * len(G.fit), line
    # (the 9 kb pair's window comes within a chunk of 255 slots of 48 columns under the sets of LONG_INDELS_NEAR_LIMIT: there, on one column per lane, it joins
    # neither group and is counted above; everywhere else it must be a fit pair)
    for k in FIT_KINDS:
        assert (k in G.fit_kinds) == (not (k == "long-indels" and c == 1 and pen_name in LONG_INDELS_NEAR_LIMIT)), (line, "fit pair of kind", k)
    two_kinds = {G.fit_kinds[i] for i in G.twopass}
    # (under the 256-row sets a snapshot is 262 - 270 array-slices: pairs whose penalty passes a thousand or so — one sequence a piece of the other, the 6 kb pair —
    # outgrow the arena the host sizes from the lengths; what the two-pass runs keep is asserted by count, by these kinds and by the pairs past the first shrink)
    assert {"fuzz", "identical", "empty", "edge-length", "homopolymer"} <= two_kinds, (line, sorted(two_kinds))
    assert sum(s > K_EPOCH for s in G.s_final) >= 4 and sum(G.s_final[i] > K_EPOCH for i in G.twopass) >= 2, (line, "pairs past the first shrink")
    if pen_name in RING256:
        assert "ring-no-wrap" in G.fit_kinds and "ring-wraps-twice" in G.fit_kinds, line
        assert G.s_final[G.fit_kinds.index("ring-no-wrap")] < 256 and G.s_final[G.fit_kinds.index("ring-wraps-twice")] > 600, line
    return line


_over_cache: dict = {}


def build_overflow(orc, pen_name: str):
    """The overflow group of a penalty set: pairs the host starts on 64-column slots (auto_c) whose windows outgrow 255 of them for certain and stay a chunk
    and more below 255 of the 256-column ones, and whose snapshots every OVER_STEP penalties fit the host's arena on both — by the oracle's band trace."""
    if pen_name not in _over_cache:
        p, oc = PEN[pen_name], overflow_candidates(pen_name)
        _over_cache[pen_name] = [(t, q) for (t, q), (lohi, _) in zip(oc, _trace_all(orc, p, oc))
                                 if auto_c(p, len(t) + len(q), OVER_STEP) == (1, 1) and chunks_overflow(lohi, len(t), len(q), 1) and chunks_fit(lohi, len(t), len(q), 4)
                                 and snap_fit(p, lohi, len(t), len(q), 1, OVER_STEP) and snap_fit(p, lohi, len(t), len(q), 4, OVER_STEP)][:MIN_OVER]
    return _over_cache[pen_name]


def check_overflow(pen_name: str, over) -> str:
    line = f"{pen_name} overflow group: {len(over)} pairs of {min(len(t) + len(q) for t, q in over)} - {max(len(t) + len(q) for t, q in over)} bases"
    assert len(over) >= MIN_OVER and all(max(len(t), len(q)) <= 30000 for t, q in over), line
    return line


def overflow_opt(mode: str) -> dict:
    return dict(mode_opt(mode), step=OVER_STEP) if mode == "twopass" else mode_opt(mode)


def overflow_tunables(mode: str):
    return route_tunables("alone", 0) + mode_tunables(mode) + ((("tb_budget_mb", OVER_TB_BUDGET_MB),) if mode == "twopass" else ())


def run_pairs(G: Groups, mode: str):
    return [G.fit[i] for i in G.twopass] if mode == "twopass" else G.fit


def self_check(orc, log=print):
    """Every cell's inputs, built and checked on the CPU."""
    seen = set()
    for cell in MATRIX:
        for pen_name, _ in cell.runs:
            if (pen_name, cell.inst.C) not in seen:
                seen.add((pen_name, cell.inst.C))
                log(check_groups(pen_name, cell.inst.C, build_groups(orc, pen_name, cell.inst.C)))
    assert seen == {(n, c) for n in PEN for c in (1, 4)}
    # The provenance pass across workgroups: under these extensions a set's two-pass runs on four columns per lane keep a pair whose window passes one workgroup's
    # 16 x 240 columns (the 9 kb pair or the unrelated one); under (3,2), (4,1) and (4,2) those pairs' snapshots outgrow the host's arena under every set, and the
    # wide windows of the provenance pass are the overflow group's (15 k columns and more, re-run on four columns per lane).
    for e in WIDE_TWOPASS_EXTS:
        wide = {n: max(G.width[i] for i in G.twopass) for n in sets_of(e) for G in [build_groups(orc, n, 4)]}
        log(f"extensions {e}: widest window of a two-pass pair on four columns per lane {wide}")
        assert max(wide.values()) > 16 * owned_cols(4), (e, wide)
    for pen_name in sorted({c.over[0] for c in MATRIX if c.over}):
        log(check_overflow(pen_name, build_overflow(orc, pen_name)))
