"""The instantiations of the packed band kernel (miniwfa_amd/csrc/mwf_band2_kernel.h, wfa_band2_kernel<T, K, E1, E2, TB, S2, BI4, FOLD>), one
entry each, with what reaches it — tunables, penalty sets, inputs — and the inputs of its two test groups, sized on the CPU from the oracle alone.

  tests/test_band_matrix_cpu.py   the set of entries EQUALS the set of instantiations in the built object; the inputs of every cell hold what
                                  tests/test_band_matrix_gpu.py needs (self_check)
  tests/test_band_matrix_gpu.py   one test per entry: the launch record names that instantiation, the *fit* group is finished by it (no re-run),
                                  the *overflow* group is handed back, and every answer equals the oracle's

Rule: an instantiation is added (or removed, or re-parameterised) together with its entry here.

fit = the pair's widest window (Oracle.band_trace) is at most the geometry's admission window AND the rules below, each of which restates
a documented hand-back of the kernel in terms of the oracle's band trace and the pair's lengths — never of what the device did:
  chunks    the kernel holds whole 256-column chunks, NWK - 1 of them counted from the chunk its slot mapping starts at, and the mapping follows
            a window whose start moves up only kAgeOut penalties late (mwf_band2_kernel.h: the test in front of `gl_next`, and the remap after a penalty)
  forecast  the 64-, 128- and 256-thread geometries (at penalties 64, 256, 1024) and the span geometry (1024, 4096) hand a pair back EARLY when its
            progress so far says its window will outgrow them (mwf_device.h window_forecast; the furthest offset comes from Oracle.band_trace_far).
            A pair within 5 % of that threshold counts as not fit: the device's furthest offset is taken over the chunks it computes
  range     biased offsets (span geometry, 512 x 5 / 512 x 6): checked every 256 penalties (mwf_band2_kernel.h wide_bias, kBiasMargin), and the
            window's start must stay within 65 535 columns of the last column
Of the candidates that pass the plain width test, the share the rules drop is reported per cell and bounded (MAX_DROPPED_SHARE)."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

from miniwfa_amd.synth import synth_pair
from oracle.pyoracle import make_opt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND2_SRC = os.path.join(ROOT, "miniwfa_amd", "csrc", "mwf_band2.hip")   # (its checked statement of the template's constants: namespace band2_text)
BAND2_OBJ = os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_band2.hip.o")
ORACLE_THREADS = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
MAX_DROPPED_SHARE = 0.25
CHUNK = 256

Inst = namedtuple("Inst", "T K E1 E2 TB S2 BI4 FOLD")


def inst_id(i: Inst) -> str:
    return f"T{i.T}-K{i.K}-E{i.E1}{i.E2}-TB{i.TB}-S2{i.S2}-BI4{i.BI4}-FOLD{i.FOLD}"


def _src_const(name: str) -> int:
    m = re.search(r"constexpr\s+int(?:32_t)?\s+[^;]*\b" + name + r"\s*=\s*(\d+)", open(BAND2_SRC).read())
    assert m, name
    return int(m.group(1))


FOLD_MAX_LAG = _src_const("kFoldMaxLag")   # o1 + e1 below it folds (launch_variant), from it on it must not
BIAS_OVER, BIAS_MARGIN = _src_const("kBiasOver"), _src_const("kBiasMargin")
SPAN_MAX_SEQ = 62000                       # mwf_plan_classes.h kBandSpanMaxSeq

# ---- penalty sets -----------------------------------------------------------------------------------------------------------------------
# (2,1): the defaults fold (o1 == x); the second set cannot.  (2,2): main.c's -a preset — on the default x, o1, e1 it is the same set as "o2=4, e2=2" —
# both pieces equal, every E1/E2 and F1/F2 tie is live; it folds.  (1,1): the -e preset (edit distance: a ring of two slices) and a set with distinct pieces.
PEN = {
    "default": dict(x=4, o1=4, e1=2, o2=15, e2=1),
    "nofold21": dict(x=6, o1=2, e1=2, o2=20, e2=1),
    "a22": dict(x=4, o1=4, e1=2, o2=4, e2=2),
    "edit": dict(x=1, o1=0, e1=1, o2=0, e2=1),
    "e11": dict(x=2, o1=3, e1=1, o2=6, e2=1),
    # o1 + e1 = kFoldMaxLag - 1: the last set that folds; = kFoldMaxLag: the first that must not (o1 == x in both)
    "lag_last_fold": dict(x=FOLD_MAX_LAG - 3, o1=FOLD_MAX_LAG - 3, e1=2, o2=15, e2=1),
    "lag_first_nofold": dict(x=FOLD_MAX_LAG - 2, o1=FOLD_MAX_LAG - 2, e1=2, o2=15, e2=1),
}


def pen_folds(p: dict) -> bool:
    return p["o1"] == p["x"] and p["e1"] == 2 and p["o1"] + p["e1"] < FOLD_MAX_LAG


# ---- geometries -------------------------------------------------------------------------------------------------------------------------
# route: how the host is brought to launch this geometry first, for every pair of the batch
#   block    forced: force_kind 2, block T, band_pack 1 (block 768: the byte-wise copy, whatever the bases)
#   wide4    default routing, wide_slots 4: the pairs of the 512-thread class on four chunk slots
#   biased   default routing: pairs the worst-case rule keeps off plain 16-bit offsets (or whose lengths pass the 512-thread class's limit) — five slots while
#            target + query stay below 3.5 of that span, else six
#   span     default routing, band_span 2: every pair the span geometry can take
# L: length of one sequence of the related pairs (the class rules of the default routing, host_class, bound it for wide4 / biased)
Geom = namedtuple("Geom", "T K S2 BI4 route L min_fit min_over")
GEOMS = {
    (64, 3, 0): Geom(64, 3, 1, 0, "block", 420, 24, 4),
    (128, 3, 0): Geom(128, 3, 1, 0, "block", 1100, 24, 4),
    (256, 3, 0): Geom(256, 3, 1, 0, "block", 2500, 24, 4),
    (512, 3, 0): Geom(512, 3, 1, 0, "block", 5000, 24, 4),
    (768, 2, 0): Geom(768, 2, 0, 0, "block", 5000, 24, 4),
    (512, 4, 0): Geom(512, 4, 1, 0, "wide4", 6000, 24, 4),
    (512, 5, 1): Geom(512, 5, 1, 1, "biased", 17800, 8, 2),
    (512, 6, 1): Geom(512, 6, 1, 1, "biased", 19000, 8, 2),
    (1024, 5, 0): Geom(1024, 5, 1, 0, "span", 30000, 8, 2),
}
COMMON_DEFAULT_ROUTING = (("div_aware", 0), ("lane_max_len", 0), ("mid_max_pairs", 0), ("coop_min_len", 1 << 40))


def nwk(g: Geom) -> int:
    return g.T // 64 * g.K


def admission_window(g: Geom) -> int:
    """The widest window the planner chooses the geometry for: (waves x K chunks - 1) x 256 - 64 columns (mwf_plan_classes.h: kBand*Window / band_window)."""
    return (nwk(g) - 1) * CHUNK - 64


def span_columns(g: Geom) -> int:
    return nwk(g) * CHUNK


def is_biased(g: Geom) -> bool:
    return bool(g.BI4) or g.route == "span"


def tunables(g: Geom, band_fold: int):
    if g.route == "block":
        return (("force_kind", 2), ("block", g.T), ("band_pack", 1), ("band_fold", band_fold))
    extra = {"wide4": (("wide_slots", 4),), "biased": (), "span": (("band_span", 2),)}[g.route]
    return COMMON_DEFAULT_ROUTING + extra + (("band_fold", band_fold),)


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
# Cell: the instantiation, its geometry, and its runs — (penalty set, band_fold) — each of which must launch exactly that instantiation
Cell = namedtuple("Cell", "inst geom runs tag")


def _runs(g: Geom, e1: int, e2: int, fold: int):
    foldable_geom = g.T >= 512 and g.S2 and e1 == 2
    if (e1, e2) == (2, 1):
        if fold:
            return (("default", 1),)
        return (("default", 0), ("nofold21", 1)) if foldable_geom else (("default", 1), ("nofold21", 1))
    if (e1, e2) == (2, 2):
        return (("a22", 1),) if fold or not foldable_geom else (("a22", 0),)
    return (("edit", 1), ("e11", 1))


def _matrix():
    cells = []
    for key, g in GEOMS.items():
        pens = ((2, 1),) if g.BI4 else ((2, 1), (2, 2), (1, 1))
        for e1, e2 in pens:
            folds = (0, 1) if (g.T >= 512 and g.S2 and e1 == 2) else (0,)
            for fold in folds:
                for tb in (0, 1):
                    cells.append(Cell(Inst(g.T, g.K, e1, e2, tb, g.S2, g.BI4, fold), g, _runs(g, e1, e2, fold), ""))
    return cells


MATRIX = _matrix()
# the two edges of the fold's condition, on 512 x 3 with traceback (extra cells of instantiations the matrix already holds)
EDGE_CELLS = [
    Cell(Inst(512, 3, 2, 1, 1, 1, 0, 1), GEOMS[(512, 3, 0)], (("lag_last_fold", 1),), "lag%d-folds" % (FOLD_MAX_LAG - 1)),
    Cell(Inst(512, 3, 2, 1, 1, 1, 0, 0), GEOMS[(512, 3, 0)], (("lag_first_nofold", 1),), "lag%d-must-not-fold" % FOLD_MAX_LAG),
]
ALL_CELLS = MATRIX + EDGE_CELLS


def cell_id(c: Cell) -> str:
    return inst_id(c.inst) + ("-" + c.tag if c.tag else "")


def declared_instantiations() -> set:
    return {c.inst for c in MATRIX}


for _c in ALL_CELLS:   # a run's penalties and band_fold force the entry's E1, E2 and FOLD
    for _pn, _bf in _c.runs:
        _p = PEN[_pn]
        assert (_p["e1"], _p["e2"]) == (_c.inst.E1, _c.inst.E2), (cell_id(_c), _pn)
        assert bool(_c.inst.FOLD) == bool(_bf and pen_folds(_p) and _c.geom.T >= 512 and _c.geom.S2), (cell_id(_c), _pn, _bf)


# ---- the instantiations of the built object ---------------------------------------------------------------------------------------------
def _inst_of(template_args: str) -> Inst:
    """Inst of a demangled argument list: "512, 3, 2, 1, false, true, false, true" (or with casts: "(bool)1")."""
    vals = []
    for a in template_args.split(","):
        a = re.sub(r"^\(\w+\)", "", a.strip()).strip("()")
        vals.append({"true": 1, "false": 0}[a] if a in ("true", "false") else int(a))
    assert len(vals) == 8, template_args
    return Inst(*vals)


def _tools(*names):
    """{tool: path} of LLVM tools (ROCm's, else the PATH's) and c++filt; a missing one maps to None."""
    import shutil
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    tools = {t: (os.path.join(llvm, t) if os.path.exists(os.path.join(llvm, t)) else shutil.which(t)) for t in names}
    tools["c++filt"] = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    return tools


def object_instantiations(obj: str = BAND2_OBJ):
    """{Inst} parsed from the object's symbol table (llvm-readelf -sW | c++filt), or a string saying why that cannot be done here."""
    import subprocess
    tools = _tools("llvm-readelf")
    if not all(tools.values()):
        return "llvm-readelf or c++filt not found"
    if not os.path.exists(obj):
        return "no " + os.path.relpath(obj, ROOT) + " (the library was not built from this tree)"
    syms = subprocess.run([tools["llvm-readelf"], "-sW", obj], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run([tools["c++filt"]], input=syms, check=True, capture_output=True, text=True).stdout
    return {_inst_of(m.group(1)) for m in re.finditer(r"wfa_band2_kernel<([^<>]*)>", dem)}


NOTE_FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def device_kernels(obj: str, kernel: str = "wfa_band2_kernel"):
    """The KERNELS in the object's gfx950 code object — what is compiled for the GPU, launchable or not: ({Inst: notes} of `kernel`'s instantiations, {demangled
    name: notes} of every other kernel), or a string saying why the object cannot be read here.  notes: the NOTE_FIELDS of the kernel's metadata note as ints, and
    "name", its demangled name.  object_instantiations reads the host symbol table, i.e. the kernel stubs: a dispatch arm that can never run leaves no stub
    behind but still instantiates its kernels on the device side.  The code object is the gfx950 entry of the object's .hip_fatbin section (llvm-objcopy,
    clang-offload-bundler); its kernels are the entries of its metadata notes (llvm-readelf --notes)."""
    import subprocess
    import tempfile
    tools = _tools("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
    if not all(tools.values()):
        return "llvm-objcopy, clang-offload-bundler, llvm-readelf or c++filt not found"
    if not os.path.exists(obj):
        return "no " + os.path.relpath(obj, ROOT) + " (the library was not built from this tree)"
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(d, "copy.o")], check=True, capture_output=True)
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co],
                       check=True, capture_output=True)
        notes = subprocess.run([tools["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = [], None
    for ln in notes.splitlines():   # (an entry of a list starts with "- "; a kernel's is the one that holds .symbol — its .args entries in front of it hold none of the fields)
        m = re.match(r"\s*(- )?\.(\w+):\s*(\S+)?\s*$", ln)
        if not m:
            continue
        if m.group(1):
            cur = {}
        if cur is None:
            continue
        if m.group(2) in NOTE_FIELDS:
            cur[m.group(2)] = int(m.group(3))
        elif m.group(2) == "symbol":
            cur["symbol"] = m.group(3)[:-3] if m.group(3).endswith(".kd") else m.group(3)
            kernels.append(cur)
    names = subprocess.run([tools["c++filt"]], input="\n".join(k.pop("symbol") for k in kernels), check=True, capture_output=True, text=True).stdout.split("\n")
    insts, others = {}, {}
    for k, name in zip(kernels, names):
        assert set(k) == set(NOTE_FIELDS), (name, k)
        k["name"] = name.strip()
        m = re.search(r"\b" + kernel + r"<([^<>]*)>", name)
        if m:
            insts[_inst_of(m.group(1))] = k
        else:
            others[k["name"]] = k
    assert len(insts) + len(others) == len(kernels), "a kernel is listed twice"
    return insts, others


# ---- the host's rules, restated ---------------------------------------------------------------------------------------------------------
def penalty_bound(p: dict, tl: int, ql: int) -> int:
    """mwf_plan_classes.h penalty_bound: delete the whole target, insert the whole query."""
    gap = lambda L: 0 if L == 0 else min(p["o1"] + L * p["e1"], p["o2"] + L * p["e2"])
    return gap(tl) + gap(ql)


def host_class(p: dict, tl: int, ql: int, wide_slots: int = 0, band_span: int = 1) -> int:
    """The size class classify_pair (mwf_plan_classes.h) gives an A/C/G/T pair when the lane, mid and whole-device kernels are off and the divergence estimate is not
    used (COMMON_DEFAULT_ROUTING), as its PairClass number: 4, 3, 2: CLS_MICRO, CLS_TINY, CLS_SMALL (the 64-, 128-, 256-thread geometries), 1: CLS_WIDE (512 threads),
    14: CLS_BIASED (its copies on biased offsets), 13: CLS_SPAN, 0: CLS_GENERIC.  tests/test_plan_classes_cpu.py compares the two at every limit."""
    ln, bound = tl + ql, penalty_bound(p, tl, ql)
    window = min(ln + 1, 2 * bound + 3)
    skew = abs(tl - ql)
    lenw = ln + 6 * max(0, skew - ln // 16)
    packable = tl + bound < 32767
    span_ok = tl <= SPAN_MAX_SEQ and ql <= SPAN_MAX_SEQ
    if span_ok and band_span == 2:
        return 13
    if packable and (window <= 448 or lenw + 1 <= 1400):
        return 4
    if packable and (window <= 1216 or lenw + 1 <= 3600):
        return 3
    if packable and (window <= 2752 or lenw + 1 <= 8200):
        return 2
    if packable and (lenw + 1 <= 4 * 8 * 3 * 256 or window <= 5824):
        return 1
    if span_ok and (p["e1"], p["e2"]) == (2, 1) and wide_slots != 3 and ln + 1 <= 7 * (48 * 256) // 2:
        return 14
    if span_ok and (ln + 1 <= 7 * 80 * 256 or window <= 20160):
        return 13
    return 0


BIASED5_MAX_LEN = 7 * (40 * 256) // 2 - 1     # choose_kernel: six slots from target + query + 1 > 3.5 x the five-slot span


def host_admits(g: Geom, p: dict, tl: int, ql: int) -> bool:
    """The lengths alone let the pair start on this geometry (the group's longest pair decides five or six slots: group_admits)."""
    if g.route == "block":
        return tl + penalty_bound(p, tl, ql) < 32767 and ((tl + ql) >> 4) * 4 + 16 <= (140 if g.T == 768 else 70 if g.T == 512 else 36 if g.T == 256 else 18 if g.T == 128 else 9) * 1024
    if g.route == "wide4":
        return host_class(p, tl, ql, wide_slots=4) == 1
    if g.route == "biased":
        return host_class(p, tl, ql) == 14 and (tl + ql <= BIASED5_MAX_LEN if g.K == 5 else True)
    return host_class(p, tl, ql, band_span=2) == 13


def group_admits(g: Geom, pairs) -> bool:
    if g.route == "biased" and g.K == 6:   # six slots: the longest pair of the launch is beyond the five-slot limit
        return max(len(t) + len(q) for t, q in pairs) > BIASED5_MAX_LEN
    return True


# ---- the kernel's hand-backs, restated on the oracle's band trace -----------------------------------------------------------------------
def widest(lohi: np.ndarray) -> int:
    return int((lohi[:, 1] - lohi[:, 0] + 1).max()) if len(lohi) else 1


def rule_chunks(g: Geom, age_out: int, lohi: np.ndarray, tl: int, ql: int) -> bool:
    """True when the window stays inside the NWK - 1 chunks counted from the slot mapping's first chunk at every penalty (columns: diagonal + tl + 1)."""
    n, cmax = nwk(g), tl + ql + 1
    gl, up_wait, up_min = max(tl, 1) >> 8, 0, 0
    for lo_d, hi_d in lohi.tolist():
        lo, hi = lo_d + tl + 1, hi_d + tl + 1
        gl_next = max(lo - 1, 1) >> 8
        if (min(hi + 1, cmax) >> 8) - min(gl_next, gl) + 1 > n - 1:
            return False
        if gl_next < gl:
            gl, up_wait = gl_next, 0
        elif gl_next > gl:
            up_min = gl_next if up_wait == 0 else min(up_min, gl_next)
            up_wait += 1
            if up_wait > age_out:
                gl, up_wait = up_min, 0
        else:
            up_wait = 0
    return True


def forecast_margin(g: Geom, far: np.ndarray, tl: int, ql: int) -> float:
    """Columns between the window the early forecast expects of the pair (mwf_device.h window_forecast) and the one it hands the pair back at, the smallest over
    the penalties the geometry forecasts at, with 5 % taken off the threshold; negative: handed back.  inf: no forecast is made for the pair."""
    n = nwk(g)
    at = (64, 256, 1024) if n < 24 else (1024, 4096) if n >= 64 else ()
    cap, kmax, s_final, margin = admission_window(g), -1, len(far), float("inf")
    bias = max(tl + BIAS_OVER - 32767, 0) if is_biased(g) else 0
    for s in at:
        if s >= s_final:       # the pair is done at that penalty or before
            break
        m = int(far[s - 1])    # the slice the mismatch term of penalty s read
        if m + bias >= 0 and m > -(1 << 29):
            kmax = max(kmax, m)
        if kmax < 8 or tl < 64:
            continue
        need = min(2 * s * tl // min(kmax + 1, tl) + 16, tl + ql + 1)
        slack = 25 if s < 128 else 17 if s < 512 else 13
        margin = min(margin, cap * slack / 10.5 - need)
    return margin


def rule_forecast(g: Geom, far: np.ndarray, tl: int, ql: int) -> bool:
    """True when no early forecast hands the pair back, with 5 % of margin.  (The forecast takes a window to grow two columns per penalty; under penalty sets whose
    costs are all even it grows one, so such pairs are handed back from about half the admission window on — the -a preset on the span geometry.)"""
    return forecast_margin(g, far, tl, ql) >= 0


def rule_range(g: Geom, lohi: np.ndarray, tl: int, ql: int) -> bool:
    """Biased offsets: dead values gain one per penalty from -32768 and must stay kBiasMargin below -1 - B (checked every 256 penalties: one period
    of margin here); the window's first column within 65 535 of the last."""
    if not is_biased(g):
        return True
    bias = max(tl + BIAS_OVER - 32767, 0)
    if len(lohi) + CHUNK > 32768 - 1 - bias - BIAS_MARGIN:
        return False
    return bool(len(lohi) == 0 or (tl + ql + 1) - (max(int(lohi[:, 0].min()) - 1, -tl) + tl + 1) <= 65535)


def age_out(inst_or_fold, e1: int = 0, e2: int = 0) -> int:
    if isinstance(inst_or_fold, Inst):
        return FOLD_MAX_LAG if inst_or_fold.FOLD else max(inst_or_fold.E1, inst_or_fold.E2) + 1
    return FOLD_MAX_LAG if inst_or_fold else max(e1, e2) + 1


def fits(g: Geom, fold: int, p: dict, lohi: np.ndarray, far: np.ndarray, tl: int, ql: int):
    """(the plain width test, the width test and every rule)."""
    wide_ok = widest(lohi) <= admission_window(g)
    if not wide_ok:
        return False, False
    return True, rule_chunks(g, age_out(fold, p["e1"], p["e2"]), lohi, tl, ql) and rule_forecast(g, far, tl, ql) and rule_range(g, lohi, tl, ql)


def is_acgt(s: bytes) -> bool:
    return not s.translate(None, b"ACGT")


_trace_cache: dict = {}


def not_fit_count(orc, pairs, opt_kw: dict, T: int, K: int, fold: int, biased: bool = False, span: bool = False) -> int:
    """How many pairs of a batch forced onto one geometry that geometry may hand back: those that are not *fit* (width or a rule above), and on the 2-bit
    geometries those with a base outside A/C/G/T.  An upper bound for n_retries of such a batch."""
    from concurrent.futures import ThreadPoolExecutor
    g = Geom(T, K, 0 if T == 768 else 1, 1 if biased else 0, "span" if span else "block", 0, 0, 0)
    p = dict(PEN["default"])
    p.update({k: v for k, v in opt_kw.items() if k in p})
    o = make_opt(**p)
    key = (id(pairs), len(pairs), tuple(sorted(p.items())))   # (the fuzzers ask once per geometry for the same batch and penalties)
    if key not in _trace_cache:
        _trace_cache.clear()
        with ThreadPoolExecutor(ORACLE_THREADS) as ex:
            _trace_cache[key] = list(ex.map(lambda tq: orc.band_trace_far(tq[0], tq[1], o, cap=penalty_bound(p, len(tq[0]), len(tq[1])) + 2), pairs))
    n = 0
    for (t, q), (lohi, far) in zip(pairs, _trace_cache[key]):
        if g.S2 and not (is_acgt(t) and is_acgt(q)):
            n += 1
        elif not fits(g, fold and pen_folds(p) and T >= 512 and g.S2, p, lohi, far, len(t), len(q))[1]:
            n += 1
    return n


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rand(rng, n: int) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _edge_lengths(L: int):
    """Lengths at k*256 - 1, k*256, k*256 + 1 and 16*k +- 1 near L (chunk and 2-bit word edges)."""
    k = max(1, L // 256)
    return [k * 256 - 1, k * 256, k * 256 + 1, L // 16 * 16 - 1, L // 16 * 16 + 1]


def _p_full(g: Geom, pen_name: str) -> float:
    """A first guess of the divergence at which a pair of 2 x L bases reaches the admission window (~0.27 (tl + ql) at 5 % under the default penalties);
    the ladders below are scaled by it and searched, so it only has to be the right order of magnitude."""
    unit = {"edit": 2.2, "e11": 1.1}.get(pen_name, 1.0)
    return min(0.30, unit * 0.05 * admission_window(g) / (0.27 * 2 * g.L))


def candidates(g: Geom, pen_name: str):
    """[(kind, target, query)]: the candidates whose shape is fixed in advance; build_groups adds the ones it has to search for with the oracle
    (the pair within a chunk of the admission limit, the overflow pairs)."""
    seed = g.T * 10 + g.K + 1000 * sorted(PEN).index(pen_name)
    rng = np.random.default_rng(seed)
    W, L = admission_window(g), g.L
    out = []
    n_rel = 16 if g.min_fit >= 24 else 3
    lens = _edge_lengths(L)
    for i in range(n_rel):   # related pairs below the limit, lengths on chunk and 2-bit word edges
        t, q = synth_pair(seed * 100 + i, lens[i % len(lens)], _p_full(g, pen_name) * (0.08 + 0.8 * i / n_rel))
        out.append(("related", t, q))
    t = _rand(rng, lens[1])
    out.append(("identical", t, t))
    # (an empty sequence: one gap; the lengths are what the route's class rule admits)
    e = {"wide4": 5000, "biased": 9000}.get(g.route, min(W - 100, 5000))
    out.append(("empty-target", b"", _rand(rng, e)))
    out.append(("empty-query", _rand(rng, e), b""))
    out.append(("homopolymer", b"A" * lens[0], b"A" * (lens[0] - 3)))
    unit_s = _rand(rng, 7)
    rep = (unit_s * (L // 7 + 2))[:lens[2]]
    cut = len(rep) // 2
    out.append(("tandem-indel", rep, rep[:cut] + rep[cut + 7 + 3:]))          # one unit and three bases out of the repeat
    out.append(("tandem-indel", rep, rep[:cut] + unit_s[:4] + rep[cut:]))
    # unrelated pairs of different lengths: the window's start climbs across chunk edges as diagonals run out of the matrix
    for a_share in (0.3, 0.62):
        tot = max(2 * L * 2 // 5, 64)
        out.append(("unrelated", _rand(rng, max(1, int(tot * a_share))), _rand(rng, max(1, tot - int(tot * a_share)))))
    # related through one long deletion (the window drifts to one side)
    t = _rand(rng, L)
    gap = max(8, W // 6)
    out.append(("long-gap", t, t[:L // 3] + t[L // 3 + gap:]))
    if g.route in ("biased", "span"):   # the longest target the host admits, at low divergence
        tot = 2 * SPAN_MAX_SEQ if g.route == "span" else BIASED5_MAX_LEN if g.K == 5 else 7 * (48 * 256) // 2 - 1
        t, q = synth_pair(seed * 100 + 90, tot // 2 + (tot & 1), 0.0015)
        out.append(("longest-target", t, q[:tot - len(t)]))
    if not g.S2:   # the byte-wise geometry: bases outside A/C/G/T
        t, q = synth_pair(seed * 100 + 91, lens[3], _p_full(g, pen_name) * 0.4)
        out.append(("non-acgt", t[:100] + b"N" + t[101:], q[:50] + b"n" + q[51:300] + b"R" + q[301:]))
    return out


def _ladder_pair(g: Geom, pen_name: str, j: int):
    """Related pairs of growing divergence, x 1.25 per step from the first guess: the first whose window passes the admission limit is cut down to the pair
    within a chunk of it, those more than a chunk beyond the span are the overflow group."""
    seed = g.T * 10 + g.K + 1000 * sorted(PEN).index(pen_name)
    # (long enough for a window more than a chunk beyond the span — where the route's class rule lets the pair be that long)
    L = g.L
    if g.route in ("block", "wide4"):
        L = max(L, (span_columns(g) + CHUNK) * (5 if pen_name == "edit" else 4) // 4)
        if g.route == "wide4":   # (plain 16-bit offsets: target length + worst-case penalty below 32767, mwf_plan_classes.h classify_pair `packable`)
            p = PEN[pen_name]
            while L + penalty_bound(p, L, L + L // 50) >= 32767 - 64:
                L -= 128
    lens = _edge_lengths(L)
    return synth_pair(seed * 100 + 50 + j, lens[j % len(lens)], min(0.9, _p_full(g, pen_name) * g.L / L * 0.6 * 1.25 ** j))


REQUIRED_FIT_KINDS = ("related", "identical", "empty-target", "empty-query", "homopolymer", "tandem-indel", "unrelated", "near-limit")
Groups = namedtuple("Groups", "fit over fit_kinds over_kinds n_width_ok n_dropped near_limit")
_groups_cache: dict = {}


def _trace_all(orc, p: dict, pairs):
    from concurrent.futures import ThreadPoolExecutor
    o = make_opt(**p)
    with ThreadPoolExecutor(ORACLE_THREADS) as ex:
        return list(ex.map(lambda tq: orc.band_trace_far(tq[0], tq[1], o, cap=min(1 << 17, penalty_bound(p, len(tq[0]), len(tq[1])) + 2)), pairs))


def _near_limit(orc, g: Geom, p: dict, fold: int, t: bytes, q: bytes, lohi, far):
    """Cut a pair whose window passes the admission limit down to a prefix whose widest window lies within a chunk below it: the prefixes' alignments are the
    pair's own up to the penalty at which they end.  A common prefix of matching bases then moves the window's columns (column = diagonal + target length + 1)
    to where whole chunks hold it.  Returns (target, query) or None; every step is judged by the oracle's trace of the cut pair."""
    W = admission_window(g)
    want = W - 150
    width = np.maximum.accumulate(lohi[:, 1] - lohi[:, 0] + 1)
    for _ in range(5):
        s = int(np.searchsorted(width, want, side="right"))     # first penalty whose window is wider than wanted
        if s >= len(far):
            return None
        k = int(far[max(0, s - 3):s + 1].max()) + 1    # (penalty sets with even costs only: every other slice is empty)
        if k < 16:
            return None
        tt, qq = t[:k], q[:max(1, k * len(q) // max(1, len(t)))]
        (l2, f2), = _trace_all(orc, p, [(tt, qq)])
        w = widest(l2)
        if w > W:
            want -= (w - W) + 60
        elif w <= W - CHUNK + 20:
            want += (W - CHUNK // 2) - w
        else:
            shifted = [(b"ACGT" * (pre // 4) + tt, b"ACGT" * (pre // 4) + qq) for pre in (0, 64, 128, 192)]
            shifted = [c for c in shifted if host_admits(g, p, len(c[0]), len(c[1]))]
            for cand, (l3, f3) in zip(shifted, _trace_all(orc, p, shifted)):
                if W - CHUNK < widest(l3) <= W and fits(g, fold, p, l3, f3, len(cand[0]), len(cand[1]))[1]:
                    return cand
                if forecast_margin(g, f3, len(cand[0]), len(cand[1])) < 0:
                    return "forecast"   # handed back early whatever the columns: the forecast is what bounds this geometry under these penalties
            want -= 40
    return None


def _near_forecast_limit(orc, g: Geom, p: dict, fold: int, t: bytes, q: bytes, far):
    """Where the early forecast, not the width, is what bounds the pairs a geometry keeps: cut a pair the forecast hands back down to the target length at which the
    forecast passes by less than a chunk (its expected window is proportional to the target length).  Judged by the oracle's trace of the cut pair."""
    n = nwk(g)
    cap, tl_new, kmax = admission_window(g), len(t), -1
    for s in ((64, 256, 1024) if n < 24 else (1024, 4096) if n >= 64 else ()):
        if s >= len(far):
            break
        kmax = max(kmax, int(far[s - 1]))
        if kmax < 8:
            continue
        slack = 25 if s < 128 else 17 if s < 512 else 13
        tl_new = min(tl_new, int((cap * slack / 10.5 - 16 - 60) * (kmax + 1) / (2 * s)))
    if tl_new >= len(t) or tl_new <= kmax + 64:
        return None
    cand = (t[:tl_new], q[:tl_new * len(q) // len(t)])
    if not host_admits(g, p, len(cand[0]), len(cand[1])):
        return None
    (l2, f2), = _trace_all(orc, p, [cand])
    ok = fits(g, fold, p, l2, f2, len(cand[0]), len(cand[1]))[1] and forecast_margin(g, f2, len(cand[0]), len(cand[1])) < CHUNK
    return cand if ok else None


def build_groups(orc, g: Geom, pen_name: str, fold: int) -> Groups:
    """The fit and the overflow group of one (geometry, penalty set, folded or not), from the oracle's band traces and the lengths alone."""
    p = PEN[pen_name]
    fold = 1 if fold and pen_folds(p) and g.T >= 512 and g.S2 else 0
    key = (g, pen_name, fold)
    if key in _groups_cache:
        return _groups_cache[key]
    W, S = admission_window(g), span_columns(g)
    tkey = (g, pen_name, "traces")
    if tkey not in _groups_cache:
        cand = [c for c in candidates(g, pen_name) if host_admits(g, p, len(c[1]), len(c[2]))]
        tr = _trace_all(orc, p, [(t, q) for _, t, q in cand])
        # the ladder, four steps at a time, until the overflow group is full (the pairs get dearer with every step)
        n_over, j, nb = 0, 0, min(4, max(2, g.min_over))
        while n_over < g.min_over and j < 24:
            step = [_ladder_pair(g, pen_name, j + i) for i in range(nb)]
            step = [tq for tq in step if host_admits(g, p, len(tq[0]), len(tq[1]))]
            for tq, (lohi, far) in zip(step, _trace_all(orc, p, step)):
                over = widest(lohi) > S + CHUNK
                n_over += over
                cand.append(("over-related" if over else "ladder", tq[0], tq[1])), tr.append((lohi, far))
            j += nb
        _groups_cache[tkey] = (cand, tr)
    cand, tr = _groups_cache[tkey]
    cand, tr = list(cand), list(tr)
    # the pair within a chunk of the limit: from the first ladder pair beyond it
    beyond = [(widest(lohi), i) for i, ((kind, _, _), (lohi, _)) in enumerate(zip(cand, tr)) if kind in ("ladder", "over-related") and widest(lohi) > W]
    for _, i in sorted(beyond)[:5]:
        nl = _near_limit(orc, g, p, fold, cand[i][1], cand[i][2], *tr[i])
        if nl == "forecast":
            nl = None
            for (kind, t, q), (lohi, far) in zip(list(cand), list(tr)):
                if nl is None and kind == "ladder" and widest(lohi) <= W and forecast_margin(g, far, len(t), len(q)) < 0:
                    nl = _near_forecast_limit(orc, g, p, fold, t, q, far)
        if nl is not None:
            cand.append(("near-limit", nl[0], nl[1])), tr.extend(_trace_all(orc, p, [nl]))
            break
    fit, over, fk, ok, n_w, n_drop, near = [], [], [], [], 0, 0, 0
    for (kind, t, q), (lohi, far) in zip(cand, tr):
        w = widest(lohi)
        if kind == "over-related":
            over.append((t, q)), ok.append(kind)
            continue
        w_ok, all_ok = fits(g, fold, p, lohi, far, len(t), len(q))
        n_w += w_ok
        n_drop += w_ok and not all_ok
        if all_ok:
            fit.append((t, q)), fk.append("related" if kind == "ladder" else kind)
            near += w > W - CHUNK or forecast_margin(g, far, len(t), len(q)) < CHUNK
    G = Groups(fit, over, fk, ok, n_w, n_drop, near)
    _groups_cache[key] = G
    return G


def check_groups(g: Geom, G: Groups, label: str) -> str:
    """Assert what tests/test_band_matrix_gpu.py relies on; returns the line it reports."""
    line = f"{label}: fit {len(G.fit)} (within one chunk of the limit: {G.near_limit}), overflow {len(G.over)}, rules dropped {G.n_dropped} of {G.n_width_ok}"
    assert len(G.fit) >= g.min_fit, line
    assert len(G.over) >= g.min_over, line
    assert G.near_limit >= 1, line
    assert G.n_dropped <= MAX_DROPPED_SHARE * G.n_width_ok, line
    for k in REQUIRED_FIT_KINDS + (("longest-target",) if g.route in ("biased", "span") else ()) + (("non-acgt",) if not g.S2 else ()):
        assert k in G.fit_kinds, (line, "no fit pair of kind", k)
    assert group_admits(g, G.fit) and group_admits(g, G.over), line
    return line


def self_check(orc, log=print):
    """Every cell's inputs, built and checked on the CPU."""
    for c in ALL_CELLS:
        for pen_name, bf in c.runs:
            log(check_groups(c.geom, build_groups(orc, c.geom, pen_name, bf), f"{cell_id(c)} {pen_name} band_fold {bf}"))
