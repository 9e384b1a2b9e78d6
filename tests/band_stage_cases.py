"""Inputs of the tests of the table form's every-penalty tail (miniwfa_amd/csrc/mwf_band2_kernel.h, kChain / kLeanTail: the iteration budget is counted DOWN and the
stop test is its sign; a slot's bit in `est` says that its chunk holds column ql + 1, the only column the end cell can lie in, and only such a chunk compares the
column with the window; the flag word gets a window edge's bits and the end cell's where they arise).  Built on the CPU from the oracle's band trace:

  budget   max_iter one below, exactly at and one above the cells counted through a penalty s* at which a wave runs two chunks, and a budget beyond 2^32
  endslot  pairs whose end column lies in the chunk of slot 0, 1, 2 (three and four slots) and 3 (four slots) of its wave at the pair's last penalty, at the first
           and the last column of a chunk, and far from the origin's column (an insertion of 4 - 6 kb: the bit is set long before the window reaches the column)

tests/test_band_stage_cpu.py asserts what every case is chosen for; tests/test_band_stage_gpu.py runs them on 512 threads x 3 and x 4 chunk slots."""
from __future__ import annotations

import numpy as np

from oracle.pyoracle import make_opt
import band_matrix as bm
import band_epoch_cases as ec
import band_chain_cases as cc

DEFAULT = cc.DEFAULT
G3, G4 = cc.G3, cc.G4
NW = cc.NW
BIG_BUDGET = (1 << 33) + 5     # does not fit 32 bits: the budget is a 64-bit count


# ---- budget -----------------------------------------------------------------------------------------------------------------------------
def budget_pair():
    return cc.multi_pairs()[0]


def budget_cases(orc):
    """(pair, s*, cum, [(label, max_iter)]): cum[s - 1] = cells counted through penalty s (the kernel's hi - lo + 1 per penalty)."""
    t, q = budget_pair()
    (lohi, _), = bm._trace_all(orc, DEFAULT, [(t, q)])
    wide = cc.penalties_with_running_chunks(lohi, len(t), len(q), NW + 1)
    s_star = wide[len(wide) // 2]
    c = ec.columns(lohi, len(t))
    cum = np.cumsum(c[:, 1] - c[:, 0] + 1)
    at = int(cum[s_star - 1])
    return (t, q), s_star, cum, [("below", at - 1), ("exact", at), ("above", at + 1), ("big", BIG_BUDGET)]


BUDGET_LABELS = ("below", "exact", "above", "big")


# ---- endslot ----------------------------------------------------------------------------------------------------------------------------
def _insertion_pair(seed: int, tl: int, ql: int):
    """A target of `tl` bases whose copy (3 % substitutions, the last forty exact) ends a query of `ql`: the alignment pays an insertion of ql - tl and the window
    climbs to the end column, ql + 1, from the origin's, tl + 1 (tests/band_chain_cases.py stale_up_clamped_pairs, shorter)."""
    rng = np.random.default_rng(seed)
    a = bm._rand(rng, tl)
    return a, bm._rand(rng, ql - tl) + cc._mutated(rng, a[:-40], 0.03) + a[-40:]


def _related_pair(seed: int, tl: int, ql: int):
    """Two copies of one sequence at 4 % substitutions, the longer one with a tail of |tl - ql| bases."""
    rng = np.random.default_rng(seed)
    a = bm._rand(rng, min(tl, ql))
    b = cc._mutated(rng, a, 0.04)
    tail = bm._rand(rng, abs(tl - ql))
    return (a + tail, b) if tl > ql else (a, b + tail)


def endslot_pairs():
    """[(t, q, note)]; ql + 1 = 768 and 767: the first and the last column of a chunk; the unrelated pair's end column lies in chunk 9, the insertion pairs' in
    chunks 17 and 25."""
    rng = np.random.default_rng(909)
    return [_related_pair(901, 760, 767) + ("first column of chunk 3",),
            _related_pair(902, 770, 766) + ("last column of chunk 2",),
            (bm._rand(rng, 2400), bm._rand(rng, 2450), "unrelated, chunk 9"),
            _insertion_pair(903, 400, 4500) + ("insertion, chunk 17",),
            _insertion_pair(904, 420, 6500) + ("insertion, chunk 25",)]


def end_slot(lohi, tl: int, ql: int, nwk: int):
    """(slot index k, wave) of the slot that holds the chunk of column ql + 1 at the pair's last penalty, by the kernel's mapping rules (cc.mapping_events)."""
    chunks = cc.slot_chunks(max(tl, 1) >> 8, nwk)
    for e in cc.mapping_events(lohi, tl, nwk):
        if e.s < len(lohi):
            chunks = e.new
    r = chunks.index((ql + 1) >> 8)
    return r // NW, r % NW


def bit_lead(lohi, tl: int, ql: int):
    """Penalties from the first at which the window's chunks [ga, gb] include the end column's chunk to the first at which the window includes the column."""
    c, g = ec.columns(lohi, tl), (ql + 1) >> 8
    in_chunks = [i for i, (lo, hi) in enumerate(c) if int(lo) >> 8 <= g <= int(hi) >> 8]
    in_window = [i for i, (lo, hi) in enumerate(c) if lo <= ql + 1 <= hi]
    return in_window[0] - in_chunks[0]


_cache: dict = {}


def endslot_group():
    if "pairs" not in _cache:
        _cache["pairs"] = [(t, q) for t, q, _ in endslot_pairs()]
    return _cache["pairs"]


def traces(orc):
    if "traces" not in _cache:
        _cache["traces"] = bm._trace_all(orc, DEFAULT, endslot_group())
    return _cache["traces"]


def expected(orc, name: str, **kw):
    """[(s, n_iter, cigar)] from the oracle, with CIGAR, computed once per group and option set."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        pairs = [budget_pair()] if name == "budget" else endslot_group()
        _cache[key] = orc.align_many(pairs, make_opt(flag=1, **DEFAULT, **kw), threads=bm.ORACLE_THREADS)[0]
    return _cache[key]


def fits(lohi, far, t, q, g):
    """The forced route admits the pair (its length rule is the three-slot geometry's, whichever slot count is forced) and the geometry finishes it."""
    return bm.host_admits(G3, DEFAULT, len(t), len(q)) and bm.fits(g, 1, DEFAULT, lohi, far, len(t), len(q))[1]

