"""The instantiations of the generic kernel (miniwfa_amd/csrc/mwf_kernels.hip: wfa_batch_kernel<T, STREAM, LDS2, H16, MODE>, 14, and wfa_bigring_kernel<256>),
one entry each, with what reaches it — tunables and batch shape —, its penalty sets, its modes and its inputs.  The structure is tests/lane_mid_matrix.py's.

  tests/test_generic_matrix_cpu.py   the set of entries EQUALS the instantiations in the built object; every cell's inputs hold what its GPU test relies on
                                     (the plan's rules restated); the oracle reproduces tests/golden/generic_pen.jsonl (the compiled reference under every
                                     set and mode of this table)
  tests/test_generic_matrix_gpu.py   one test per entry: per set and mode one align whose only launch is that instantiation (the `generic launch:` record,
                                     MWF_DEBUG), no re-run, every answer equal to the oracle's; and the edge tests

Rule: an instantiation is added (or removed, or re-parameterised) together with its entry here.

The generic kernel takes ANY penalties (reference: one loop, miniwfa.c:243-259, :390-393) and every hand-back of the other kernels ends on it, so a cell is
not sized to "fit": the kernel finishes whatever it is given, and the only hand-backs it has are the 16-bit rows' (the edge tests).  What a cell's batch must
satisfy is what makes the host launch exactly that form ONCE:
  block cells   force_kind 0 and block N (scalar cells: scalar_generic 1) keep the whole batch in one group — except that in low-memory mode a pair whose
                penalty bound lies below `step` can never take a snapshot and runs in a high-memory launch of its own (mwf_plan_classes.h classify_pair, step0): the
                low-memory batches hold the pairs with bound >= step only
  LDS2 cells    block 0, e2 == 1, no step, div_aware 0, and min(max(tl + ql) + 1, 2 max(bound) + 3) >= 8192 over the batch (run_batch_kernel): then 768 threads
                on 32-bit rows (ring16 0), and on 16-bit rows (ring16 2) 512 threads score-only, 768 with traceback; every pair plain A/C/G/T
  big ring      nH > 256 (kMaxRing): wfa_bigring_kernel<256> whatever the tunables
"""
from __future__ import annotations

import os
import re
from collections import namedtuple

from miniwfa_amd.synth import fuzz_pairs, random_seq, skewed_pairs, synth_pair
from oracle.pyoracle import make_opt
from band_matrix import ORACLE_THREADS, _trace_all, is_acgt, penalty_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "miniwfa_amd", "csrc", "build", "mwf_kernels.hip.o")

Inst = namedtuple("Inst", "T STREAM LDS2 H16 MODE BIG")
K_MAX_RING = 256      # mwf_internal.h kMaxRing
LDS_COLS = 16384      # run_batch_kernel lds_e2_cols
WIDE_WINDOW = 8192    # run_batch_kernel: the 512-thread choice, and with it E2/F2 in LDS


def inst_id(i: Inst) -> str:
    if i.BIG:
        return f"bigring-T{i.T}"
    if i.LDS2:
        return f"lds2-T{i.T}-H16{i.H16}-MODE{i.MODE}"
    return f"{'stream' if i.STREAM else 'scalar'}-T{i.T}"


# ---- penalty sets -----------------------------------------------------------------------------------------------------------------------
PEN = {
    "default": dict(x=4, o1=4, e1=2, o2=15, e2=1),
    "edit": dict(x=1, o1=0, e1=1, o2=0, e2=1),        # nH = 2, the shallowest ring; o == 0 on both pieces (j1 == jg1, j2 == jg2, x == o1 + e1)
    "asm5": dict(x=4, o1=6, e1=3, o2=26, e2=1),       # minimap2's asm5-like set
    "e81": dict(x=6, o1=5, e1=8, o2=40, e2=1),        # a long E1 history (n1 = 9)
    "xdeep": dict(x=30, o1=2, e1=2, o2=10, e2=1),     # ring depth set by x
    "o1zero": dict(x=3, o1=0, e1=2, o2=12, e2=1),     # j1 == jg1
    "ring256": dict(x=4, o1=4, e1=2, o2=254, e2=1),   # nH == kMaxRing, the deepest ring of the fast forms: every penalty tracks the good bits
    "e51": dict(x=4, o1=6, e1=5, o2=30, e2=1),        # e1 = 5 on e2 == 1
    "a22": dict(x=4, o1=4, e1=2, o2=24, e2=2),        # e2 = 2
    "e33": dict(x=3, o1=5, e1=3, o2=20, e2=3),        # e1 == e2
    "e2gt": dict(x=5, o1=3, e1=1, o2=2, e2=3),        # e2 > e1
    "e88": dict(x=9, o1=4, e1=8, o2=20, e2=8),        # both histories long
    "ring257": dict(x=4, o1=4, e1=2, o2=255, e2=1),   # nH = 257: the big-ring form only
    "big_a22": dict(x=4, o1=4, e1=2, o2=298, e2=2),   # ... with e2 = 2 (nH 301)
    "big_e3": dict(x=4, o1=6, e1=3, o2=280, e2=1),    # ... with e1 = 3 (nH 282)
}
FAST_SETS = ("default", "edit", "asm5", "e81", "xdeep", "o1zero", "ring256", "e51", "a22", "e33", "e2gt", "e88")
LDS2_SETS = tuple(n for n in FAST_SETS if PEN[n]["e2"] == 1)
BIG_SETS = ("ring257", "big_a22", "big_e3")
CAP_SETS = ("default", "asm5", "ring256")   # the 8400 x 8400 pair's window passes the LDS cap and comes back under these
CAP_PAIR_SETS = CAP_SETS + ("edit",)        # ... and under the edit set the same pair never leaves the LDS copy


def nH(p: dict) -> int:
    """mwf_plan.cpp make_penalty: the H ring's depth."""
    return max(p["x"], p["o1"] + p["e1"], p["o2"] + p["e2"]) + 1


def n_slices(p: dict) -> int:
    """NS: the slices of a snapshot, nH + 2 n1 + 2 n2."""
    return nH(p) + 2 * (p["e1"] + 1) + 2 * (p["e2"] + 1)


assert len(FAST_SETS) == 12 and len(LDS2_SETS) == 8 and nH(PEN["edit"]) == 2 and nH(PEN["ring256"]) == K_MAX_RING
assert [nH(PEN[n]) for n in BIG_SETS] == [257, 301, 282] and all(nH(PEN[n]) <= K_MAX_RING for n in FAST_SETS)

# ---- modes ------------------------------------------------------------------------------------------------------------------------------
# (name, options, batch): "base" — the whole batch; "low" — its pairs with a penalty bound >= step (see above); "small" — its pairs with tl, ql <= 300
# (a snapshot every penalty or two costs NS slices each)
SMALL_MAX = 300
WIDE_MAX_S = 4200     # stops the unrelated wide pairs inside the wide form (under the edit set only the 8400 x 8400 one, penalty 4359)


def modes(pen_name: str, lds2: bool = False, mode: int = -1):
    """The modes of one penalty set: every one for the block and big-ring cells; for an LDS2 cell the two without a step that its MODE serves."""
    n = nH(PEN[pen_name])
    out = [("score", dict(flag=0), "base"), ("score-max_s60", dict(flag=0, max_s=60), "base"),
           ("cigar", dict(flag=1), "base"), ("cigar-max_iter5000", dict(flag=1, max_iter=5000), "base")]
    if lds2:
        # max_s caps the penalty bound the plan sizes the window by: under max_s = 60 no window can pass 2 x 61 + 3 columns, the wide form is never taken and
        # the run lands on the stream form of 256 threads (launched_inst) — the stop rule INSIDE the wide forms needs 2 (max_s + 1) + 3 >= 8192
        out.insert(2, ("score-max_s4200", dict(flag=0, max_s=WIDE_MAX_S), "base"))
        return [m for m in out if m[1]["flag"] == mode]
    steps = [97, n] + ([n - 1] if n - 1 > 2 else [])      # (under the edit set nH - 1 == 1: the small step below)
    out += [(f"lowmem-step{s}", dict(flag=1, step=s), "low") for s in dict.fromkeys(steps)]
    out += [(f"lowmem-step{s}-small", dict(flag=1, step=s), "small") for s in (1, 2)]
    return out


def all_modes(pen_name: str):
    """Every mode some cell runs the set under (what tests/golden/generic_pen.jsonl pins the oracle for)."""
    out = modes(pen_name)
    if pen_name in LDS2_SETS:
        out += [m for m in modes(pen_name, True, 0) if m[0] not in {x[0] for x in out}]
    return out


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "inst tun sets wide")
COMMON = (("force_kind", 0), ("div_aware", 0))


def _matrix():
    cells = []
    for T in (64, 128, 256, 512, 1024):
        cells.append(Cell(Inst(T, 1, 0, 0, -1, 0), COMMON + (("block", T),), FAST_SETS, 0))
    for T in (64, 128, 256, 512, 1024):
        cells.append(Cell(Inst(T, 0, 0, 0, -1, 0), COMMON + (("block", T), ("scalar_generic", 1)), FAST_SETS, 0))
    for T, h16, mode in ((768, 0, 0), (768, 0, 1), (512, 1, 0), (768, 1, 1)):
        cells.append(Cell(Inst(T, 1, 1, h16, mode, 0), COMMON + (("block", 0), ("ring16", 2 if h16 else 0)), LDS2_SETS, 1))
    cells.append(Cell(Inst(256, 0, 0, 0, -1, 1), COMMON, BIG_SETS, 0))
    return cells


MATRIX = _matrix()
assert len(MATRIX) == 15 and len({c.inst for c in MATRIX}) == 15


def cell_id(c: Cell) -> str:
    return inst_id(c.inst)


def declared_instantiations() -> set:
    return {c.inst for c in MATRIX}


def cell_modes(c: Cell, pen_name: str):
    return modes(pen_name, bool(c.inst.LDS2), c.inst.MODE)


# ---- the instantiations of the built object ---------------------------------------------------------------------------------------------
def object_instantiations():
    """{Inst} parsed from the object's symbol table (llvm-readelf -sW | c++filt: demangled kernel names only), or a string saying why that cannot be done here."""
    import shutil
    import subprocess
    readelf = next((p for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), shutil.which("llvm-readelf") or "") if p and os.path.exists(p)), None)
    cxxfilt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not readelf or not cxxfilt:
        return "llvm-readelf or c++filt not found"
    if not os.path.exists(OBJ):
        return "no " + os.path.relpath(OBJ, ROOT) + " (the library was not built from this tree)"
    syms = subprocess.run([readelf, "-sW", OBJ], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run([cxxfilt], input=syms, check=True, capture_output=True, text=True).stdout
    out = set()
    for m in re.finditer(r"wfa_(batch|bigring)_kernel<([^<>]*)>", dem):
        vals = []
        for a in (x.strip() for x in m.group(2).split(",")):
            a = re.sub(r"^\(\w+\)", "", a).strip("()")
            vals.append({"true": 1, "false": 0}[a] if a in ("true", "false") else int(a) if re.fullmatch(r"-?\d+", a) else None)
        assert None not in vals and len(vals) == (5 if m.group(1) == "batch" else 1), m.group(0)
        out.add(Inst(*vals, 0) if m.group(1) == "batch" else Inst(vals[0], 0, 0, 0, -1, 1))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
_base_cache: list = []


def base_pairs():
    """The batch of every block and big-ring cell (41 pairs): fuzz and length-skewed pairs, the degenerate ones, and targets of 255 / 256 / 1023 / 1024 bases
    — the origin column tl + 1 and the window's edges on both sides of a 256-column chunk edge."""
    if not _base_cache:
        t = random_seq(11, 400)
        p = [pq for pq in fuzz_pairs(7, 24, 1200) if pq != (b"", b"")] + skewed_pairs(8, 6, 100, 1200)
        p += [(random_seq(1, 700), random_seq(2, 500)), (t, t), (b"", t), (t, b""), (b"A", b"C"), (random_seq(12, 900), random_seq(12, 900)[:333]), synth_pair(77, 1500, 0.10)]
        for i, tl in enumerate((255, 256, 1023, 1024)):
            t2, q2 = synth_pair(900 + i, tl + 40, 0.06)
            p.append((t2[:tl], q2[:tl - 9 + 6 * i]))
        _base_cache.extend(p)
    return list(_base_cache)


WIDE_PAIR = (4200, 4100)
CAP_PAIR = (8400, 8400)


def wide_pairs(pen_name: str | None = None, cap: bool | None = None):
    """What an LDS2 batch adds: an unrelated 4200 x 4100 pair (the form is taken), and — `cap`; by default under CAP_PAIR_SETS — an unrelated 8400 x 8400 pair whose
    chunk-rounded window passes the 16384 columns of the LDS copy and comes back under CAP_SETS."""
    out = [(random_seq(3, WIDE_PAIR[0]), random_seq(4, WIDE_PAIR[1]))]
    if (pen_name in CAP_PAIR_SETS) if cap is None else cap:
        out.append((random_seq(5, CAP_PAIR[0]), random_seq(6, CAP_PAIR[1])))
    return out


def batch(c: Cell, pen_name: str, which: str, step: int = 0):
    """(key, pairs) of one run; the key names the batch for the oracle cache."""
    p = PEN[pen_name]
    pairs = base_pairs()
    if which == "low":
        pairs = [tq for tq in pairs if penalty_bound(p, len(tq[0]), len(tq[1])) >= step]
    elif which == "small":
        pairs = [tq for tq in pairs if max(len(tq[0]), len(tq[1])) <= SMALL_MAX and penalty_bound(p, len(tq[0]), len(tq[1])) >= step]
    if c.wide:
        assert which == "base"
        return ("wide", pen_name in CAP_PAIR_SETS), pairs + wide_pairs(pen_name)
    return (which, step if which != "base" else 0), pairs


def takes_wide_form(p: dict, pairs, max_s: int = 0) -> bool:
    """run_batch_kernel: the 512-thread choice, which the LDS copy of E2/F2 is tied to.  (penalty_bound honours max_s: the pass stops one penalty after it.)"""
    max_len = max(len(t) + len(q) for t, q in pairs)
    max_bound = max(penalty_bound(p, len(t), len(q)) for t, q in pairs)
    if max_s > 0:
        max_bound = min(max_bound, max_s + 1)
    return min(max_len + 1, 2 * max_bound + 3) >= WIDE_WINDOW and p["e2"] == 1 and nH(p) <= K_MAX_RING


def launched_inst(c: Cell, pen_name: str, okw: dict, pairs) -> Inst:
    """The instantiation a run of the cell launches: the cell's own, except an LDS2 cell's run whose max_s keeps every window below the wide form's."""
    if c.inst.LDS2 and not takes_wide_form(PEN[pen_name], pairs, okw.get("max_s", 0)):
        return Inst(256, 1, 0, 0, -1, 0)
    return c.inst


def ring16_admitted(pairs) -> bool:
    """run_batch_kernel, div_aware 0: max(tl) + max(tl + ql) / 8 < 65500."""
    return max(len(t) for t, _ in pairs) + max(len(t) + len(q) for t, q in pairs) // 8 < 65500


def in_lds(lo: int, hi: int, tl: int) -> bool:
    """stream_pass cur_in_lds on a penalty's window (diagonals lo ... hi of the oracle's band trace; column = diagonal + tl + 1): whole 256-column chunks within the cap."""
    clo, chi = lo + tl + 1, hi + tl + 1
    return ((chi | 255) - (clo & ~255) + 1) <= LDS_COLS


_cap_cache: dict = {}


def cap_crossings(orc, pen_name: str, pair=None):
    """(penalties, widest window, penalty at which the window first leaves the LDS copy | None, LDS -> HBM hand-overs, HBM -> LDS hand-overs) of the 8400 x 8400 pair."""
    key = (pen_name, None if pair is None else (len(pair[0]), len(pair[1]), hash(pair)))
    if key not in _cap_cache:
        t, q = pair or (random_seq(5, CAP_PAIR[0]), random_seq(6, CAP_PAIR[1]))
        (lohi, _), = _trace_all(orc, PEN[pen_name], [(t, q)])
        state = [in_lds(int(lo), int(hi), len(t)) for lo, hi in lohi]
        out_ = sum(1 for a, b in zip(state, state[1:]) if a and not b)
        in_ = sum(1 for a, b in zip(state, state[1:]) if not a and b)
        first = next((i + 1 for i, s in enumerate(state) if not s), None)
        _cap_cache[key] = (len(lohi), int((lohi[:, 1] - lohi[:, 0] + 1).max()), first, out_, in_)
    return _cap_cache[key]


def check_cell_inputs(orc, c: Cell, log=print):
    """Assert what tests/test_generic_matrix_gpu.py relies on for every run of the cell."""
    for pen_name in c.sets:
        p = PEN[pen_name]
        assert (nH(p) > K_MAX_RING) == bool(c.inst.BIG), (cell_id(c), pen_name)
        for mname, okw, which in cell_modes(c, pen_name):
            key, pairs = batch(c, pen_name, which, okw.get("step", 0))
            label = f"{cell_id(c)} {pen_name} {mname}"
            assert len(pairs) >= (4 if which == "small" else 20), (label, len(pairs))
            assert (b"", b"") not in pairs, label
            if okw.get("step", 0) > 0:      # one launch: every pair can reach the first snapshot by its bound
                assert all(penalty_bound(p, len(t), len(q)) >= okw["step"] for t, q in pairs), label
                if which == "small":
                    assert all(max(len(t), len(q)) <= SMALL_MAX for t, q in pairs), label
            if c.inst.LDS2:
                assert p["e2"] == 1 and "step" not in okw and takes_wide_form(p, pairs), label
                assert (launched_inst(c, pen_name, okw, pairs) == c.inst) == (okw.get("max_s", 0) != 60), label
                assert 2 * (WIDE_MAX_S + 1) + 3 >= WIDE_WINDOW, label
                assert any(len(t) + len(q) >= WIDE_WINDOW for t, q in pairs), label
                if c.inst.H16:
                    assert all(is_acgt(t) and is_acgt(q) for t, q in pairs) and ring16_admitted(pairs), label
                    assert all(len(t) + penalty_bound(p, len(t), len(q)) + 3 <= 65532 for t, q in pairs), label   # no pair can outgrow the 16-bit rows
            else:                           # nothing in a block cell's batch may look like a wide one to a reader: the forced block decides, and says so
                assert dict(c.tun).get("block", 0) != 0 or c.inst.BIG, label
        tls = {len(t) for t, _ in batch(c, pen_name, "base")[1]}
        assert {255, 256, 1023, 1024} <= tls, (cell_id(c), pen_name)
    if c.inst.LDS2:
        for pen_name in CAP_SETS:
            n_s, width, first, n_out, n_in = cap_crossings(orc, pen_name)
            log(f"{pen_name}: the {CAP_PAIR[0]} x {CAP_PAIR[1]} pair, {n_s} penalties, widest window {width}, leaves the LDS copy at penalty {first}, "
                f"{n_out} hand-overs to HBM, {n_in} back")
            assert width > LDS_COLS and n_out >= 1 and n_in >= 1, (pen_name, width, n_out, n_in)
        n_s, width, first, n_out, n_in = cap_crossings(orc, "edit")
        log(f"edit: the same pair, {n_s} penalties, widest window {width}: never leaves the LDS copy")
        assert first is None and n_out == 0, (width, first)


def expected(orc, pen_name: str, okw: dict, pairs):
    """[(s, n_iter, cigar | None)] of a run, under the run's own options."""
    return orc.align_many(pairs, make_opt(**okw, **PEN[pen_name]), threads=ORACLE_THREADS)[0]
