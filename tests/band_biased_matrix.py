"""The packed band kernel's five- and six-slot copies of the 512-thread geometry on biased offsets — wfa_band2_kernel<512, 5 | 6, E1, E2, TB, 1, 1, FOLD>, class 14 (CLS_BIASED)
of the host's routing — for every set but (2,1): (2,2) folded and not, (1,1), (3,1), (3,2), (4,1), built by miniwfa_amd/csrc/mwf_band2_bi.hip and
mwf_band2_bi_deep.hip.  One entry each, with what reaches it and the inputs of its two test groups.

  tests/test_band_biased_cpu.py          the entries EQUAL the instantiations in the two objects; the fixture; the inputs of every cell (self_check)
  tests/test_band_biased_matrix_gpu.py   one test per entry, by the method of tests/test_band_matrix_gpu.py
  tests/test_band_biased_gpu.py          the short end, default routing, the range check, gap runs, forced-routing fuzz, guard rails

Built the way tests/band_deep_matrix.py is: a SECOND, private instance of band_matrix.py under another module name.  Its PEN gains the deep module's three sets,
and its host_class — the restatement of the class rule (mwf_plan_classes.h classify_pair) — admits class 14 for the sets whose copies are built (band2_biased512_supported) where the
public one admits it for (2,1) alone.  `band_matrix` as every other test imports it and the deep module's instance are only read from."""
from __future__ import annotations

import importlib.util
import os
import sys

import band_matrix as _bm_public   # (only to read from: never assigned to)
import band_deep_matrix as _dm     # (likewise)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_BUILD = os.path.join(os.path.dirname(HERE), "miniwfa_amd", "csrc", "build")
BIASED_OBJS = {"bi": os.path.join(CSRC_BUILD, "mwf_band2_bi.hip.o"), "bi_deep": os.path.join(CSRC_BUILD, "mwf_band2_bi_deep.hip.o")}
DEEP_PEN = _dm.DEEP_PEN
# set name -> (unit, runs with band_fold 0 as well): the sets whose copies are built.  (2,1)'s copies are the default unit's, tests/band_matrix.py.
BUILT = {"a22": "bi", "edit": "bi", "e31": "bi_deep", "e32": "bi_deep", "e41": "bi_deep"}
BUILT_EXT = {(2, 1), (2, 2), (1, 1), (3, 1), (3, 2), (4, 1)}   # band2_biased512_supported


def _private_band_matrix():
    name = "band_matrix__biased_instance"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "band_matrix.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.PEN = dict(mod.PEN, **DEEP_PEN)

    def host_class(p: dict, tl: int, ql: int, wide_slots: int = 0, band_span: int = 1) -> int:
        """band_matrix.host_class with class 14 open to every set whose copies are built; the rule's form and order are classify_pair's (mwf_plan_classes.h)."""
        ln, bound = tl + ql, mod.penalty_bound(p, tl, ql)
        window = min(ln + 1, 2 * bound + 3)
        skew = abs(tl - ql)
        lenw = ln + 6 * max(0, skew - ln // 16)
        packable = tl + bound < 32767
        span_ok = tl <= mod.SPAN_MAX_SEQ and ql <= mod.SPAN_MAX_SEQ
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
        if span_ok and (p["e1"], p["e2"]) in BUILT_EXT and wide_slots != 3 and ln + 1 <= 7 * (48 * 256) // 2:
            return 14
        if span_ok and (ln + 1 <= 7 * 80 * 256 or window <= 20160):
            return 13
        return 0

    mod.host_class = host_class   # (host_admits looks it up in the instance's globals)
    return mod


base = _private_band_matrix()
assert base is not _bm_public and base is not _dm.base
assert not (set(DEEP_PEN) & set(_bm_public.PEN)) and _bm_public.host_class.__module__ == "band_matrix", "the public band_matrix must stay as it is"

Inst, Geom, Cell = base.Inst, base.Geom, base.Cell
inst_id, cell_id = base.inst_id, base.cell_id
ORACLE_THREADS, MAX_DROPPED_SHARE = base.ORACLE_THREADS, base.MAX_DROPPED_SHARE
PEN = {k: base.PEN[k] for k in BUILT}
# the two geometries, with the existing biased cells' values
GEOMS = {k: g for k, g in base.GEOMS.items() if g.BI4}
assert sorted(GEOMS.values()) == sorted([Geom(512, 5, 1, 1, "biased", 17800, 8, 2), Geom(512, 6, 1, 1, "biased", 19000, 8, 2)])


def _matrix():
    cells = []
    for g in GEOMS.values():
        for pen_name in BUILT:
            p = base.PEN[pen_name]
            for fold in ((0, 1) if p["e1"] == 2 else (0,)):
                for tb in (0, 1):
                    # (a set that folds runs folded with band_fold 1 and unfolded with band_fold 0; the others are launched the same either way)
                    cells.append(Cell(Inst(g.T, g.K, p["e1"], p["e2"], tb, g.S2, 1, fold), g, ((pen_name, fold if p["e1"] == 2 else 1),), ""))
    return cells


MATRIX = _matrix()
ALL_CELLS = MATRIX

for _c in ALL_CELLS:   # a run's penalties and band_fold force the entry's E1, E2 and FOLD
    for _pn, _bf in _c.runs:
        _p = base.PEN[_pn]
        assert (_p["e1"], _p["e2"]) == (_c.inst.E1, _c.inst.E2), (cell_id(_c), _pn)
        assert bool(_c.inst.FOLD) == bool(_bf and base.pen_folds(_p)), (cell_id(_c), _pn, _bf)


def declared_instantiations(unit: str | None = None) -> set:
    return {c.inst for c in MATRIX if unit is None or BUILT[c.runs[0][0]] == unit}


def object_instantiations(unit: str):
    """{Inst} of the unit's host stubs, or a string saying why the object cannot be read here."""
    return base.object_instantiations(BIASED_OBJS[unit])


def device_instantiations(unit: str):
    """{Inst} of the KERNELS in the unit's gfx950 code object — what is compiled for the GPU, launchable or not (band_matrix.device_kernels) — or a string
    saying why it cannot be read here."""
    got = base.device_kernels(BIASED_OBJS[unit], "wfa_band2_kernel")
    return got if isinstance(got, str) else set(got[0])


def tunables(g: Geom, band_fold: int):
    return base.tunables(g, band_fold)


_groups: dict = {}


def _near_limit_by_bisection(orc, g: Geom, p: dict, fold: int, over_pairs):
    """band_deep_matrix._near_limit_by_bisection on this module's instance (whose host_admits knows class 14 for the set): a prefix of an overflow pair whose
    widest window lies within a chunk below the admission limit, moved by a common prefix of matching bases to where whole chunks hold it."""
    W = base.admission_window(g)
    for t, q in over_pairs:
        lo_k, hi_k = 16, len(t)
        for _ in range(24):
            k = (lo_k + hi_k) // 2
            cand = (t[:k], q[:max(1, k * len(q) // len(t))])
            (lohi, far), = base._trace_all(orc, p, [cand])
            w = base.widest(lohi)
            if w > W:
                hi_k = k
            elif w <= W - base.CHUNK + 20:
                lo_k = k
            else:
                shifted = [(b"ACGT" * (pre // 4) + cand[0], b"ACGT" * (pre // 4) + cand[1]) for pre in (0, 64, 128, 192)]
                shifted = [c for c in shifted if base.host_admits(g, p, len(c[0]), len(c[1]))]
                for c, (l3, f3) in zip(shifted, base._trace_all(orc, p, shifted)):
                    if W - base.CHUNK < base.widest(l3) <= W and base.fits(g, fold, p, l3, f3, len(c[0]), len(c[1]))[1]:
                        return c
                break
            if hi_k - lo_k < 2:
                break
    return None


def build_groups(orc, g: Geom, pen_name: str, band_fold: int):
    """band_matrix.build_groups on the private instance; where its search found no pair within a chunk of the limit, one found by bisection joins the fit group."""
    p = base.PEN[pen_name]
    fold = 1 if band_fold and base.pen_folds(p) else 0
    key = (g, pen_name, fold)
    if key not in _groups:
        G = base.build_groups(orc, g, pen_name, fold)
        if "near-limit" not in G.fit_kinds:
            nl = _near_limit_by_bisection(orc, g, p, fold, G.over)
            if nl is not None and group_ok(g, G.fit + [nl]):
                G = G._replace(fit=G.fit + [nl], fit_kinds=G.fit_kinds + ["near-limit"], n_width_ok=G.n_width_ok + 1, near_limit=G.near_limit + 1)
        _groups[key] = G
    return _groups[key]


def group_ok(g: Geom, pairs) -> bool:
    return base.group_admits(g, pairs)


def check_groups(g: Geom, G, label: str) -> str:
    return base.check_groups(g, G, label)


def self_check(orc, log=print):
    """Every cell's inputs, built and checked on the CPU (a score-only cell and its CIGAR twin share theirs)."""
    seen = set()
    for c in ALL_CELLS:
        for pen_name, bf in c.runs:
            fold = 1 if bf and base.pen_folds(base.PEN[pen_name]) else 0
            if (c.geom, pen_name, fold) in seen:
                continue
            seen.add((c.geom, pen_name, fold))
            log(check_groups(c.geom, build_groups(orc, c.geom, pen_name, bf), f"T{c.geom.T}-K{c.geom.K} {pen_name} fold {fold}"))


def not_fit_count(orc, pairs, opt_kw: dict, K: int, band_fold: int = 1) -> int:
    """How many pairs of a batch that starts on the 512 x K copies on biased offsets those may hand back: band_matrix.not_fit_count on the private instance."""
    return base.not_fit_count(orc, pairs, opt_kw, 512, K, band_fold, biased=True)


def crossover(p: dict) -> int:
    return _dm.crossover(p)
