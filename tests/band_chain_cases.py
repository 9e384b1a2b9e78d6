"""Inputs of the tests of the table form's chunk chain (miniwfa_amd/csrc/mwf_band2_kernel.h, kChain / kGeo: a slot's probe geometry — the room bounds rj and the
query's table index of the lane's columns — is computed where the slot's chunk is assigned, remap(), and read from registers for as long as the slot keeps the
chunk; the rare tests of a chunk are laid out behind its straight line).  Built on the CPU from the oracle's CIGAR and band trace:

  stale    pairs of 0.3 - 3 kb whose slot mapping moves: DOWN (a long deletion: the window's start sinks, the slot that wraps takes the chunk at the start, and the
           alignment then runs through that chunk: an exact run of eight or more bases that ends exactly at the end of the target, of the query, of both — rj at tl,
           at ql - d) and UP (the start climbs; the mapping follows behind the ageing period and the slots below it wrap to the chunk NWK further up: pairs of
           0.6 x 8.2 kb whose window climbs thirty chunks and whose last run, clamped like the above, is walked in a chunk that a slot wrapped up to — and the
           climbing pairs of the window-epoch tests)
  multi    unrelated pairs whose windows pass 2048 and 4096 columns: some wave runs two, then three chunks per penalty, for hundreds of penalties
  toggle   a slot starts or stops running between consecutive penalties: the shrink at a multiple of 256 moves an edge inward across a chunk boundary, an edge
           enters a new chunk (tests/band_epoch_cases.py's cross-shrink and both-cross pairs), the pair ends at a penalty at which a wave runs two chunks
  stop     max_s stops a pair at a penalty at which a wave runs two chunks
  runs, tabalign   tests/band_tab_cases.py's run-length and indel groups, unchanged: every probe shape that module lists on the cached geometry

tests/test_band_chain_cpu.py asserts what every case is chosen for; tests/test_band_chain_gpu.py runs them on 512 threads x 3 and x 4 chunk slots."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle.pyoracle import make_opt
import band_matrix as bm
import band_epoch_cases as ec
import band_tab_cases as tc

DEFAULT = tc.DEFAULT
G3, G4 = tc.G3, tc.G4
NW = 8                      # waves of the 512-thread geometry: a window of more than NW chunks gives some wave two running chunks, of more than 2 NW three
AGE = bm.FOLD_MAX_LAG       # kAgeOut of the folded form
MIN_RUN = tc.FULL           # a run the first probe matches whole


def _rand(rng, n):
    return bm._rand(rng, n)


def _mutated(rng, s: bytes, p: float) -> bytes:
    out = bytearray(s)
    for i in np.nonzero(rng.random(len(s)) < p)[0]:
        out[i] = tc._other(rng, s[i])[0]
    return bytes(out)


# ---- the slot mapping, restated from remap() and the bookkeeping behind the barrier ------------------------------------------------------
def slot_chunks(gl: int, nwk: int):
    """Chunk of every slot index r = wave + NW * slot under the mapping that starts at chunk gl."""
    base = gl - gl % nwk
    return [g if g >= gl else g + nwk for g in range(base, base + nwk)]


Event = namedtuple("Event", "s up old new")   # the mapping moves behind penalty s (penalty s + 1 is the first on the new one); old / new: slot_chunks


def mapping_events(lohi, tl: int, nwk: int, age: int = AGE):
    gl, up_wait, up_min, out = max(tl, 1) >> 8, 0, 0, []
    for i, (gl_next, _, _) in enumerate(ec.keys(lohi, tl)):
        if gl_next < gl:
            out.append(Event(i + 1, False, slot_chunks(gl, nwk), slot_chunks(gl_next, nwk)))
            gl, up_wait = gl_next, 0
        elif gl_next > gl:
            up_min = gl_next if up_wait == 0 else min(up_min, gl_next)
            up_wait += 1
            if up_wait > age:
                out.append(Event(i + 1, True, slot_chunks(gl, nwk), slot_chunks(up_min, nwk)))
                gl, up_wait = up_min, 0
        else:
            up_wait = 0
    return out


def assigned_at(events, chunk: int, pen: int):
    """The event that gave its slot the chunk it holds at penalty `pen` (None: held since the start of the pair, or held by no slot)."""
    got = None
    for e in events:
        if e.s >= pen:
            break
        r = e.new.index(chunk) if chunk in e.new else None
        if r is not None and e.old[r] != chunk:
            got = e
        elif r is None:
            got = None
    return got


def match_runs(t: bytes, q: bytes, cigar):
    """[(i, j, n, penalty)] of the alignment's exact runs: start, length, and the penalty whose extension walks the run."""
    out, cur = [], None
    for i, j, s in tc.path_cells(t, q, cigar):
        if t[i] == q[j] and cur and (cur[0] + cur[2], cur[1] + cur[2], cur[3]) == (i, j, s):
            cur[2] += 1
            continue
        if cur:
            out.append(tuple(cur))
        cur = [i, j, 1, s] if t[i] == q[j] else None
    if cur:
        out.append(tuple(cur))
    return out


def clamped_runs_in_new_chunks(t, q, cigar, lohi, nwk: int):
    """[(end, event, run)]: runs of MIN_RUN or more that end exactly at the end of the "target", the "query" or "both", in a chunk that a slot was given by a remap."""
    tl, ql = len(t), len(q)
    ev = mapping_events(lohi, tl, nwk)
    out = []
    for i, j, n, pen in match_runs(t, q, cigar):
        if n < MIN_RUN or pen < 1 or not (i + n == tl or j + n == ql):
            continue
        e = assigned_at(ev, (j - i + tl + 1) >> 8, pen)
        if e is not None:
            out.append(("both" if (i + n == tl and j + n == ql) else "target" if i + n == tl else "query", e, (i, j, n, pen)))
    return out


# ---- stale ------------------------------------------------------------------------------------------------------------------------------
def stale_down_pairs():
    """[(t, q, end)]: 300 bases, a deletion of 700 - 900, 500 more at 3 % whose last forty match, and a tail of thirty bases on the query ("target": the last
    run ends where the target does), on the target ("query"), on neither ("both")."""
    out = []
    for n, (gap, end) in enumerate(((700, "both"), (700, "target"), (700, "query"), (900, "target"), (820, "query"))):
        rng = np.random.default_rng(5100 + n)
        a, x, b = _rand(rng, 300 + n), _rand(rng, gap), _rand(rng, 500 + 3 * n)
        t = a + x + b
        q = _mutated(rng, a, 0.03) + _mutated(rng, b[:-40], 0.03) + b[-40:]
        if end == "target":
            q += tc._other(rng, t[-1]) + _rand(rng, 29)
        elif end == "query":
            t += tc._other(rng, q[-1]) + _rand(rng, 29)
        out.append((t, q, end))
    return out


def stale_up_clamped_pairs():
    """[(t, q, end)]: a target of 0.6 kb whose copy (3 % substitutions, the last forty bases exact) ends a query of 8.2 kb, with a tail of thirty bases on the query
    ("target"), on the target ("query"), on neither ("both").  The alignment pays an insertion of 7.6 kb: the window, ten chunks at its widest, climbs from chunk 0 to
    chunk 32, the mapping follows it up some twenty times, and the last run is walked in chunk 32 — the chunk NWK above chunk 8 (24 chunks) and above chunk 0 (32
    chunks), which its slot was given by a remap upwards."""
    out = []
    for n, (tl, ql, end) in enumerate(((600, 8250, "both"), (640, 8230, "target"), (620, 8270, "query"))):
        rng = np.random.default_rng(6200 + n)
        a = _rand(rng, tl)
        x = _rand(rng, ql - tl)
        t, q = a, x + _mutated(rng, a[:-40], 0.03) + a[-40:]
        if end == "target":
            q += tc._other(rng, t[-1]) + _rand(rng, 29)
        elif end == "query":
            t += tc._other(rng, q[-1]) + _rand(rng, 29)
        out.append((t, q, end))
    return out


def stale_up_pairs(orc):
    """tests/band_epoch_cases.py's climbing pairs on 24 and on 32 chunks, folded."""
    seen, out = set(), []
    for nwk in (24, 32):
        for p in ec.case(orc, f"climb-nwk{nwk}-fold1").pairs:
            if p not in seen:
                seen.add(p)
                out.append(p)
    return out


# ---- multi ------------------------------------------------------------------------------------------------------------------------------
MULTI_LENGTHS = ((1300, 1340), (1500, 1280), (2400, 2450), (2600, 2380))


def multi_pairs():
    rng = np.random.default_rng(2048)
    return [(_rand(rng, tl), _rand(rng, ql)) for tl, ql in MULTI_LENGTHS]


def ends_wide_pairs():
    """Unrelated heads of 2.3 - 2.5 kb and a common tail of 300 bases: the alignment's last run jumps to the end cell while the window still meets more than eight chunks."""
    rng = np.random.default_rng(4097)
    out = []
    for tl, ql in ((2300, 2340), (2500, 2380)):
        tail = _rand(rng, 300)
        out.append((_rand(rng, tl) + b"A" + tail, _rand(rng, ql) + b"C" + tail))
    return out


def chunks_met(lohi, tl: int, ql: int):
    """Chunks [ga, gb] the window of every penalty meets: the header's lo >> 8 and hi >> 8."""
    return [(ga, gb) for _, ga, gb in ec.keys(lohi, tl)]


def penalties_with_running_chunks(lohi, tl: int, ql: int, more_than: int):
    """Penalties at which the window meets more than `more_than` chunks: more than NW — some wave has a later running slot; more than 2 NW — two later ones."""
    return [i + 1 for i, (ga, gb) in enumerate(chunks_met(lohi, tl, ql)) if gb - ga + 1 > more_than]


# ---- toggle -----------------------------------------------------------------------------------------------------------------------------
def toggle_pairs(orc):
    """(pairs, kinds): the cross-shrink and both-cross pairs of the window-epoch tests on 24 and 32 chunks, and ends_wide_pairs (they end at a penalty at which
    a wave runs two chunks)."""
    pairs, kinds = [], []
    for name in ("cross-shrink-nwk24", "cross-shrink-nwk32", "both-cross-nwk24", "both-cross-nwk32"):
        for p in ec.case(orc, name).pairs:
            if p not in pairs:
                pairs.append(p)
                kinds.append(name[:-6])
    for p in ends_wide_pairs():
        pairs.append(p)
        kinds.append("ends-wide")
    return pairs, kinds


# ---- stop -------------------------------------------------------------------------------------------------------------------------------
def stop_case(orc):
    """(pair, {"max_s": s* - 1}, s*): the first `multi` pair, stopped once penalty s* is done, a penalty at which its window meets ten chunks or more."""
    t, q = multi_pairs()[0]
    (lohi, _), = bm._trace_all(orc, DEFAULT, [(t, q)])
    wide = penalties_with_running_chunks(lohi, len(t), len(q), NW + 1)
    s_star = wide[len(wide) // 2]
    return (t, q), dict(max_s=s_star - 1), s_star


GROUPS = ("stale", "multi", "toggle", "runs", "tabalign")
_groups: dict = {}


def group(orc, name: str):
    """[(t, q)] of a group, built once."""
    if name not in _groups:
        if name == "stale":
            _groups[name] = [(t, q) for t, q, _ in stale_down_pairs()] + [(t, q) for t, q, _ in stale_up_clamped_pairs()] + stale_up_pairs(orc)
        elif name == "multi":
            _groups[name] = multi_pairs()
        elif name == "toggle":
            _groups[name] = toggle_pairs(orc)[0]
        else:
            _groups[name] = tc.group(name)
    return _groups[name]


_expected: dict = {}


def expected(orc, name: str, **kw):
    """[(s, n_iter, cigar)] from the oracle, with CIGAR, computed once."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _expected:
        pairs = [stop_case(orc)[0]] if name == "stop" else group(orc, name)
        _expected[key] = orc.align_many(pairs, make_opt(flag=1, **DEFAULT, **kw), threads=bm.ORACLE_THREADS)[0]
    return _expected[key]


_traces: dict = {}


def traces(orc, name: str):
    if name not in _traces:
        _traces[name] = bm._trace_all(orc, DEFAULT, group(orc, name))
    return _traces[name]


def table_kernel_notes():
    """{demangled kernel name: {field: int}} of the kernels of mwf_band2_tab.hip.o, from the metadata notes of its gfx950 code object (band_matrix.device_kernels)."""
    got = bm.device_kernels(tc.TAB_OBJ, "wfa_band2_tab_kernel")
    assert not isinstance(got, str), got
    return {v["name"]: v for part in got for v in part.values()}
