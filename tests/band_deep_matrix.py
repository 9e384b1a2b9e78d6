"""The packed band kernel's instantiations for gap extensions of 3 and 4 — wfa_band2_kernel<T, K, E1, E2, TB, S2, 0, 0> with (E1, E2) = (3,1), (3,2), (4,1),
built by miniwfa_amd/csrc/mwf_band2_e3.hip and mwf_band2_e4.hip — one entry each, with what reaches it and the inputs of its two test groups.

  tests/test_band_deep_cpu.py          the entries EQUAL the instantiations in the two objects; the fixture; the inputs of every cell (self_check)
  tests/test_band_deep_matrix_gpu.py   one test per entry, by the method of tests/test_band_matrix_gpu.py
  tests/test_band_deep_gpu.py          gap-depth hazards, forced-geometry fuzz, default routing, chain mode, guard rails

Everything that depends on the geometry alone — Geom, Inst, the admission windows, the kernel's hand-back rules restated on the oracle's band trace, the host's
class rules, the search for the fit / overflow groups — is tests/band_matrix.py's.  Its input builders look a penalty set up by NAME in its PEN table (and seed
their generators from the name's rank in it), and that table must stay as it is: the existing cells derive their seeds from it.  So this module loads a SECOND,
private instance of band_matrix.py under another module name and gives THAT instance the new sets; `band_matrix` as every other test imports it is not touched.

The new sets never fold (launch_variant folds for e1 == 2 only) and have no copies on biased offsets (512 x 5 / 512 x 6: band2_biased512_supported), so a cell
is (geometry, set, TB), its one run is (set, band_fold 1), and kAgeOut = max(e1, e2) + 1 = 4 or 5 (band_matrix.age_out)."""
from __future__ import annotations

import importlib.util
import os
import sys

import band_matrix as _bm_public   # (only to read from: never assigned to)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_BUILD = os.path.join(os.path.dirname(HERE), "miniwfa_amd", "csrc", "build")
DEEP_OBJS = {3: os.path.join(CSRC_BUILD, "mwf_band2_e3.hip.o"), 4: os.path.join(CSRC_BUILD, "mwf_band2_e4.hip.o")}

# the sets of tests/test_sys_penalties_gpu.py: minimap2's asm5-like 4,6,3,26,1 and one per other pair of extensions the band kernel is built for
DEEP_PEN = {
    "e31": dict(x=4, o1=6, e1=3, o2=26, e2=1),
    "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2),
    "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1),
}
# (4,2) missed its speed gate on 1024 x 10 kb and is NOT built for the band kernel: it keeps the routing of every other pair of extensions
NOT_BUILT_PEN = {"e42": dict(x=2, o1=4, e1=4, o2=24, e2=2)}


def _private_band_matrix():
    name = "band_matrix__deep_instance"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "band_matrix.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.PEN = dict(mod.PEN, **DEEP_PEN)   # the private instance's table: the old sets keep their names, the new ones sort in among them
    return mod


base = _private_band_matrix()
assert base is not _bm_public and not (set(DEEP_PEN) & set(_bm_public.PEN)), "the public band_matrix must keep its own penalty table"

Inst, Geom, Cell = base.Inst, base.Geom, base.Cell
inst_id, cell_id = base.inst_id, base.cell_id
ORACLE_THREADS, MAX_DROPPED_SHARE = base.ORACLE_THREADS, base.MAX_DROPPED_SHARE
# every geometry the new sets are built on: all of band_matrix.GEOMS but the copies on biased offsets
GEOMS = {k: g for k, g in base.GEOMS.items() if not g.BI4}
assert sorted((g.T, g.K) for g in GEOMS.values()) == [(64, 3), (128, 3), (256, 3), (512, 3), (512, 4), (768, 2), (1024, 5)]


def _matrix():
    cells = []
    for g in GEOMS.values():
        for pen_name, p in DEEP_PEN.items():
            for tb in (0, 1):
                cells.append(Cell(Inst(g.T, g.K, p["e1"], p["e2"], tb, g.S2, 0, 0), g, ((pen_name, 1),), ""))
    return cells


MATRIX = _matrix()
ALL_CELLS = MATRIX


def declared_instantiations(e1: int | None = None) -> set:
    return {c.inst for c in MATRIX if e1 is None or c.inst.E1 == e1}


def object_instantiations(e1: int):
    """{Inst} of the unit for gap extension e1, or a string saying why the object cannot be read here."""
    return base.object_instantiations(DEEP_OBJS[e1])


def device_instantiations(e1: int):
    """{Inst} of the KERNELS in the unit's gfx950 code object — what is compiled for the GPU, launchable or not (band_matrix.device_kernels) — or a string
    saying why it cannot be read here."""
    got = base.device_kernels(DEEP_OBJS[e1], "wfa_band2_kernel")
    return got if isinstance(got, str) else set(got[0])


def tunables(g: Geom):
    return base.tunables(g, 1)


_groups: dict = {}


def _near_limit_by_bisection(orc, g: Geom, p: dict, over_pairs):
    """A pair whose widest window lies within a chunk below the admission limit and that passes every rule: a prefix of an overflow pair, its length found by
    bisection on the oracle's band trace (the prefixes' alignments are the pair's own up to the penalty at which they end), then moved by a common prefix of
    matching bases to where whole chunks hold it.  band_matrix's own search steps by the furthest offset at the penalty the window passes the limit; under
    a set whose costs are all even every other slice is empty and it can step past the one chunk it aims for."""
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
                    if W - base.CHUNK < base.widest(l3) <= W and base.fits(g, 0, p, l3, f3, len(c[0]), len(c[1]))[1]:
                        return c
                break
            if hi_k - lo_k < 2:
                break
    return None


def build_groups(orc, g: Geom, pen_name: str):
    """band_matrix.build_groups on the private instance; where its search found no pair within a chunk of the limit, one found by bisection joins the fit group."""
    key = (g, pen_name)
    if key not in _groups:
        G = base.build_groups(orc, g, pen_name, 0)
        if "near-limit" not in G.fit_kinds:
            nl = _near_limit_by_bisection(orc, g, DEEP_PEN[pen_name], G.over)
            if nl is not None:
                G = G._replace(fit=G.fit + [nl], fit_kinds=G.fit_kinds + ["near-limit"], n_width_ok=G.n_width_ok + 1, near_limit=G.near_limit + 1)
        _groups[key] = G
    return _groups[key]


def check_groups(g: Geom, G, label: str) -> str:
    return base.check_groups(g, G, label)


def self_check(orc, log=print):
    """Every cell's inputs, built and checked on the CPU (a score-only cell and its CIGAR twin share theirs)."""
    seen = set()
    for c in ALL_CELLS:
        for pen_name, _ in c.runs:
            if (c.geom, pen_name) in seen:
                continue
            seen.add((c.geom, pen_name))
            log(check_groups(c.geom, build_groups(orc, c.geom, pen_name), f"T{c.geom.T}-K{c.geom.K} {pen_name}"))


def not_fit_count(orc, pairs, opt_kw: dict, block: int) -> int:
    """How many pairs of a batch forced onto ONE geometry (block 64 ... 768, or 1024: band_span 2) under ANY penalties that geometry may hand back: those
    whose oracle band trace is wider than its admission window or meets a hand-back rule with kAgeOut = max(e1, e2) + 1 (no fold), and pairs outside A/C/G/T
    on a 2-bit geometry.  band_matrix.not_fit_count takes the penalties from opt_kw; this fixes the rest for the unfolded sets."""
    return base.not_fit_count(orc, pairs, opt_kw, block, 5 if block == 1024 else 2 if block == 768 else 3, 0, span=block == 1024)


def crossover(p: dict) -> int:
    """The gap length from which the second piece is the cheaper one: smallest L with o2 + L e2 <= o1 + L e1 (10 for 4,6,3,26,1)."""
    L = 1
    while p["o1"] + L * p["e1"] < p["o2"] + L * p["e2"]:
        L += 1
    return L
