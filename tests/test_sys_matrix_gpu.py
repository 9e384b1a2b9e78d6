"""One test per instantiation of the whole-device kernel and penalty set it runs under (tests/sys_matrix.py: the table, what reaches each entry, the launch records every run must print, and
its inputs), and the edge tests.

Per cell and run (penalty set, mode), on both routes (alone: coop_grid 16; side by side: the default grid), one align on a fresh engine:
  fit       pairs the kernel finishes by the oracle's band trace: the launch records (MWF_DEBUG, stderr: `sys launch:`) are exactly the sequence the table
            states — instantiation, pass, pairs side by side x workgroups each, for every launch of every pair —; n_retries == 0, stats.kernel_kind == 1,
            lowmem_two_pass as the mode says, no "gave up waiting"; s, n_iter and every CIGAR word equal the oracle's
  overflow  (C = 1 cells; sys_c 0, coop_grid 16) pairs the host starts on 64-column slots and whose windows outgrow them: the first record is the cell's
            instantiation, every pair is launched again on the C = 4 twin, n_retries equals the group's size, nothing is re-run on one workgroup, the answers
            equal the oracle's.  (Two-pass runs: n_retries is at least the group's size — an unrelated pair's snapshots also outgrow the arena the host sizes
            from the lengths, which is a re-run of its own; tests/sys_matrix.py, the snapshots rule.)
Score-only cells also equal what their CIGAR twin computed on the same inputs.  Integer work: no tolerance anywhere.

The overflow group of a C = 1 entry is a test of its own (test_overflow_group), so that an entry's two groups are timed apart.

That the cells can fail was tried once — A and B with one test per entry, before the entry tests were split per penalty set (90 tests: 48 entries, 25
overflow groups, 17 edge tests), C on the seg entries, their overflow groups and test_low_memory_steps (24 tests) — with three libraries built from copies of the sources outside the repository, one computed value changed per pass form
(never an address, a bound, a wait or a loop count); nothing faulted or hung:
  A  deferred traceback form: sys_cell breaks the E1 / E2 tie of the traceback code the other way; deferred score-only form and provenance pass: the n_iter sum
     one short per slice.  10 of 90 red.  The four deferred score cells by n_iter in the fit group (default, alone: (1477, 1191883) for (1477, 1193360); a22: n_iter
     5891518 for 5895986) and their two overflow groups ((14893, 115788765) for (14893, 115803658)); sys-E21-TB1-defer-C1 by a CIGAR (default, pair 23); the three
     edge tests that run the default set score-only.  GREEN: sys-E22-TB1-defer-C1 — under (4,4,2,4,2) and its like both pieces cost the same, so the other choice
     at a tie is the same gap and the same CIGAR: the tie can only show under (2,1) — and all fourteen seg cells: the provenance pass's cell count goes to
     stats.cells_pass1, not to n_iter (the reference counts the second pass only), so nothing these tests compare sees it.  Hence library C.
  B  plain form (score-only and traceback): the n_iter sum one over per slice.  82 of 90 red: every plain cell and every seg cell (their runs' second passes are
     plain) by n_iter in the fit group (x2, alone: (413, 87306) for (413, 86893)), sys-E21 / E22-TB0-defer-C4 through their CIGAR twins (four columns with
     traceback are never deferred), every overflow group whose launches include a plain pass, all twelve edge tests, and the rings of 257 rows' 256-row
     counterparts under (1,1), (3,1), (4,2).  Green: the deferred C = 1 cells and their overflow groups, the two deferred 256-row counterparts.
  C  provenance pass only: the same tie broken the other way, which moves the provenance a cell inherits at a tie (an equally good chain of checkpoints).
     2 of 24 red: sys-E31-seg-plain-C1 and -C4, both by a CIGAR under (4,0,3,10,1), pair 8 of the two-pass group, alone — with an open of 0 a gap's first base
     ties with its extension everywhere, and the second pass, collapsed onto the other chain's checkpoints, returns another CIGAR of the same penalty.  Green:
     the twelve other seg entries, the seven seg overflow groups and the three step tests: under their sets no tie on the paths of these pairs changes the
     checkpoints' cells.  A wrong provenance VALUE that is no valid alternative (a cell off the chain) would feed the checkpoint walk an index the unchanged
     kernel cannot produce, which is the kind of mutation this record does not try: beyond the tie, no admissible mutation of the provenance pass was found.

Time (profiles/sys_matrix/durations.txt, one MI355X, one sitting on this tree): the slowest test of tests/test_generic_matrix_gpu.py took 7.19 s; the slowest
here 5.00 s (test_overflow_group[sys-E32-TB0-plain-C1]; the slowest entry test 3.83 s).  A test run by itself (-k) pays the oracle's traces and answers of its
penalty set itself: 5.40 s (sys-E21-TB1-defer-C1-ring256_21), 4.98 s, 2.43 s, and 5.21 s for that overflow group.
"""
import re

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, synth_pair
from oracle.pyoracle import make_opt
import band_matrix as bm
import sys_matrix as sm

SYS_LINE = re.compile(r"\[libmwf_hip\] sys launch: E1 (\d+) E2 (\d+) P (\d+) DEFER (\d+) TB (\d+) C (\d+) SEG (\d+), pass (\d+), groups (\d+) x (\d+), grid (\d+)")

_oracle_cache: dict = {}
_device_cache: dict = {}


def n_cu() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def sys_records(err: str):
    """[(instantiation, pass, pairs side by side, workgroups per pair, grid)] of one align, in launch order."""
    out = []
    for m in SYS_LINE.finditer(err):
        v = list(map(int, m.groups()))
        out.append((sm.SysInst(*v[:7]), v[7], v[8], v[9], v[10]))
    return out


def _show(recs, limit=6):
    return [(sm.inst_id(i), f"pass {p}", f"{n} x {g}") for i, p, n, g, _ in recs[:limit]] + (["... %d in all" % len(recs)] if len(recs) > limit else [])


def oracle_many(orc, pairs, kw: dict, key=None):
    if key is not None and key in _oracle_cache:
        return _oracle_cache[key]
    exp = orc.align_many(pairs, make_opt(**kw), threads=bm.ORACLE_THREADS)[0]
    if key is not None:
        _oracle_cache[key] = exp
    return exp


def run_align(tun, opt_kw: dict, pairs, capfd):
    """One align of `pairs` on a fresh engine with the tunables `tun`: dict(s, it, cig | None, n_retries, kind, two_pass, records, err)."""
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    try:
        for k, v in tun:
            eng.set(k, v)
        o = mw.opt_init(**opt_kw)
        b = eng.upload(pk)
        capfd.readouterr()
        b.align(o)
        s, it, nc = b.results()   # (the re-runs of what was handed back are launched when the results are asked for)
        cig = [b.cigar(i, int(nc[i])).tolist() for i in range(pk.n)] if (o.flag & 1) else None
        st = eng.stats()
        err = capfd.readouterr().err
        out = dict(s=np.array(s).copy(), it=np.array(it).copy(), cig=cig, n_retries=int(st.n_retries), kind=int(st.kernel_kind), two_pass=int(st.lowmem_two_pass),
                   records=sys_records(err), err=err)
        b.free()
        return out
    finally:
        eng.close()


def check_answers(got, exp, label, cigar=None):
    """s, n_iter and — where the run stored traceback and the pair was finished — every CIGAR word."""
    cigar = got["cig"] is not None if cigar is None else cigar
    for i, (es, eit, ecig) in enumerate(exp):
        assert (int(got["s"][i]), int(got["it"][i])) == (es, eit), (label, "pair", i, (int(got["s"][i]), int(got["it"][i])), (es, eit))
        if cigar and es >= 0:
            assert got["cig"][i] == (ecig or []), (label, "pair", i, "CIGAR")


def no_warnings(got, label):
    assert "gave up waiting" not in got["err"] and "one workgroup" not in got["err"], (label, [ln for ln in got["err"].splitlines() if "warning" in ln][:3])


def expected_records(p: dict, mode: str, c: int, pairs, route: str):
    launches = sm.side_by_side([len(t) + len(q) for t, q in pairs], sm.GROUP_WG if route == "alone" else n_cu())
    return [(inst, ps, n, gs, n * gs) for n, gs in launches for inst, ps in sm.records(p, mode, c, c)]


def _report(lines, capfd):
    with capfd.disabled():
        print()
        for ln in lines:
            print(ln)


def cell_run(orc, pen_name: str, mode: str, c: int, route: str, capfd):
    """The fit group of (set, mode, C) on a route: run once (cached by what determines its launches), checked here in full."""
    key = (pen_name, mode, c, route)
    if key in _device_cache:
        return _device_cache[key]
    p = sm.PEN[pen_name]
    G = sm.build_groups(orc, pen_name, c)
    pairs = sm.run_pairs(G, mode)
    low = mode in ("walk", "twopass")
    exp_cand = oracle_many(orc, [(t, q) for _, t, q in sm.candidates(pen_name)], dict(flag=1, step=sm.STEP if low else 0, **p), (pen_name, low))   # (both C share it)
    exp_all = [exp_cand[j] for j in G.idx]
    exp = [exp_all[i] for i in G.twopass] if mode == "twopass" else exp_all
    got = run_align(sm.route_tunables(route, c) + sm.mode_tunables(mode), dict(**sm.mode_opt(mode), **p), pairs, capfd)
    label = f"{pen_name} {mode} C {c} {route}"
    want = expected_records(p, mode, c, pairs, route)
    assert got["records"] == want, (label, "launch records", _show(got["records"]), "expected", _show(want))
    assert sum(r[2] for r in got["records"]) == len(pairs) * len(sm.records(p, mode, c, c)), (label, "not every pair was launched")
    assert got["n_retries"] == 0 and got["kind"] == 1, (label, "fit pairs were run again", got["n_retries"], got["kind"])
    no_warnings(got, label)
    assert got["two_pass"] == (1 if mode == "twopass" else 0), (label, "lowmem_two_pass", got["two_pass"])
    check_answers(got, exp, label)
    _device_cache[key] = got
    return got


def overflow_run(orc, cell, pen_name: str, mode: str, capfd):
    p = sm.PEN[pen_name]
    over = sm.build_overflow(orc, pen_name)
    sm.check_overflow(pen_name, over)
    key = ("overflow", pen_name, mode)
    if key not in _device_cache:
        kw = dict(**sm.overflow_opt(mode), **p)
        exp = oracle_many(orc, over, dict(kw, flag=1), ("overflow", pen_name, kw["step"]))
        got = run_align(sm.overflow_tunables(mode), kw, over, capfd)
        check_answers(got, exp, f"{pen_name} {mode} overflow")
        _device_cache[key] = got
    got = _device_cache[key]
    label = f"{sm.cell_id(cell)} {pen_name} {mode} overflow"
    n, recs = len(over), got["records"]
    step = sm.overflow_opt(mode)["step"]
    c2 = sm.auto_c(p, max(len(t) + len(q) for t, q in over), step)[1]
    assert c2 == sm.auto_c(p, min(len(t) + len(q) for t, q in over), step)[1]
    first = [(i, ps, 1, sm.GROUP_WG, sm.GROUP_WG) for _ in range(n) for i, ps in sm.records(p, mode, 1, c2)]
    again = [(i, ps, 1, sm.GROUP_WG, sm.GROUP_WG) for i, ps in sm.records(p, mode, 4, 4)]
    assert cell.inst in [i for i, _ in sm.records(p, mode, 1, c2)], label   # (the expected first launches are this entry's)
    assert recs[:len(first)] == first, (label, "first launches", _show(recs), "expected", _show(first))
    assert got["kind"] == 1
    no_warnings(got, label)
    assert got["two_pass"] == (1 if mode == "twopass" else 0), (label, "lowmem_two_pass", got["two_pass"])
    assert got["n_retries"] == n, (label, "re-runs", got["n_retries"])
    assert recs[len(first):] == again * n, (label, "re-runs", _show(recs[len(first):], 12), "expected", _show(again * n))
    return got


# one test per entry and penalty set of the entry (a test then pays the oracle's traces and answers of one set, whatever ran before it)
CELL_SETS = [(c, n) for c in sm.MATRIX for n in dict.fromkeys(r[0] for r in c.runs)]


@pytest.mark.gpu
@pytest.mark.parametrize("cell,pen", CELL_SETS, ids=[f"{sm.cell_id(c)}-{n}" for c, n in CELL_SETS])
def test_instantiation(cell, pen, oracle, capfd, monkeypatch):
    """One entry under one of its penalty sets: every run (set, mode) of the table's, on both routes."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    report, inst = [], cell.inst
    try:
        for pen_name, mode in [r for r in cell.runs if r[0] == pen]:
            G = sm.build_groups(oracle, pen_name, inst.C)
            report.append("   " + sm.check_groups(pen_name, inst.C, G))
            for route in sm.ROUTES:
                got = cell_run(oracle, pen_name, mode, inst.C, route, capfd)
                assert any(r[0] == inst for r in got["records"]), (sm.cell_id(cell), pen_name, mode, route, "never launched", _show(got["records"]))
                report.append(f"   {sm.cell_id(cell)} {pen_name} {mode} {route}: {len(sm.run_pairs(G, mode))} pairs, {len(got['records'])} launches {_show(got['records'], 2)}")
                if mode == "score":   # ... and equal what the CIGAR twin computes on the same inputs
                    tw = cell_run(oracle, pen_name, "cigar", inst.C, route, capfd)
                    assert (got["s"] == tw["s"]).all() and (got["it"] == tw["it"]).all(), (sm.cell_id(cell), pen_name, route, "score-only differs from its CIGAR twin")
    finally:
        _report(report, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [c for c in sm.MATRIX if c.inst.C == 1], ids=sm.cell_id)
def test_overflow_group(cell, oracle, capfd, monkeypatch):
    """The overflow group of every C = 1 entry (a test of its own, so that an entry's two groups are timed apart): sys_c 0, coop_grid 16."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    assert cell.over is not None and all(c.over is None for c in sm.MATRIX if c.inst.C == 4)
    pen_name, mode = cell.over
    got = overflow_run(oracle, cell, pen_name, mode, capfd)
    _report([f"   {sm.cell_id(cell)} {pen_name} {mode} overflow: {len(sm.build_overflow(oracle, pen_name))} pairs, re-runs {got['n_retries']}, launches {_show(got['records'], 3)}"], capfd)


# ---- edge tests: one deferred set, one plain set, one deep set ----------------------------------------------------------------------------------
EDGE_SETS = ("default", "x2", "e31")
EDGES = (8, 256, 512)       # the first hand-off block's end, the first and the second epoch's
_edge_cache: dict = {}


def _gapped(L: int, k: int, g: int):
    """spaced_subs plus one deletion of g bases at a third of the pair: penalty k x + the gap's cost."""
    t, q = sm.spaced_subs(L, k) if k else (sm.random_seq(5 + L, L),) * 2
    at = L // 3 + 7
    return t, q[:at] + q[at + g:]


def edge_pairs(orc, pen_name: str):
    """For each of 7, 8, 9, 255, 256, 257, 511, 512, 513 the pair — k spaced substitutions, with or without one short gap: the penalty follows from the costs —
    whose final penalty is that value or, where the set's costs rule it out, the nearest one on the same side of the edge, by the oracle."""
    if pen_name not in _edge_cache:
        p = sm.PEN[pen_name]
        pool = [_gapped(48 * (k + 1) + g, k, g) for k in range(0, 520 // p["x"] + 2) for g in (0, 1, 2, 3, 12, 14)]
        sc = [r[0] for r in oracle_many(orc, pool, dict(flag=0, **p))]
        pick = []
        for e in EDGES:   # the largest penalty below the edge, the smallest from the edge on, and the next one above that
            below = max((s, -j) for j, s in enumerate(sc) if s < e)
            at = min((s, j) for j, s in enumerate(sc) if s >= e)
            above = min((s, j) for j, s in enumerate(sc) if s > at[0])
            pick += [pool[-below[1]], pool[at[1]], pool[above[1]]]
        _edge_cache[pen_name] = pick
    return _edge_cache[pen_name]


@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", EDGE_SETS)
def test_final_penalty_at_block_and_epoch_edges(pen_name, oracle, capfd, monkeypatch):
    """Pairs that end at, just below and just above penalties 8, 256 and 512, in all four modes at one and four columns per lane: the end cell is acted upon at
    the epoch's end, the last block and the last epoch are partial ones."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = sm.PEN[pen_name]
    pairs = edge_pairs(oracle, pen_name)
    s_all = sorted(r[0] for r in oracle_many(oracle, pairs, dict(flag=0, **p)))
    report = [f"   {pen_name}: final penalties {s_all}"]
    try:
        for e in EDGES:   # next to every edge from below, on it (every set here pays 4 or 2 per substitution: 8, 256 and 512 are sums of them), and above
            assert any(e - 4 <= s < e for s in s_all) and e in s_all and any(e < s <= e + 4 for s in s_all), (pen_name, e, s_all)
        for mode in sm.MODES:
            low = mode in ("walk", "twopass")
            exp = oracle_many(oracle, pairs, dict(flag=1, step=sm.STEP if low else 0, **p), ("edge", pen_name, low))
            for c in (1, 4):
                got = run_align(sm.route_tunables("side", c) + sm.mode_tunables(mode), dict(**sm.mode_opt(mode), **p), pairs, capfd)
                label = f"{pen_name} {mode} C {c}"
                check_answers(got, exp, label)
                assert got["kind"] == 1 and got["n_retries"] == 0 and got["two_pass"] == (mode == "twopass"), (label, got["n_retries"], got["two_pass"])
                assert got["records"] == expected_records(p, mode, c, pairs, "side"), (label, _show(got["records"]))
    finally:
        _report(report, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", EDGE_SETS)
def test_stop_rules_at_block_and_epoch_edges(pen_name, oracle, capfd):
    """max_s on and next to 8 and 256, max_iter one below and exactly at the oracle's n_iter of the first pair, in all four modes (two-pass form: the rules apply to
    the second pass only, as in the reference), against the oracle with the same options."""
    p = sm.PEN[pen_name]
    pairs = [synth_pair(820000 + sm._seed(pen_name), 3000, 0.1), synth_pair(820001 + sm._seed(pen_name), 700, 0.05)] + edge_pairs(oracle, pen_name)[3:6]
    bad, n_runs = [], 0
    for mode in sm.MODES:
        low = mode in ("walk", "twopass")
        base = dict(flag=sm.mode_opt(mode)["flag"], step=sm.mode_opt(mode)["step"], **p)
        n_iter0 = oracle_many(oracle, pairs[:1], base)[0][1]
        stops = [dict(max_s=v) for v in (7, 8, 9, 255, 256, 257)] + [dict(max_iter=n_iter0 - 1), dict(max_iter=n_iter0)]
        for j, stop in enumerate(stops):
            kw = dict(base, **stop)
            exp = oracle_many(oracle, pairs, kw)
            c = (1, 4)[(j + low) % 2]
            got = run_align(sm.route_tunables("side", c) + sm.mode_tunables(mode), kw, pairs, capfd)
            n_runs += 1
            assert got["kind"] == 1
            for i, (es, eit, ecig) in enumerate(exp):
                if (int(got["s"][i]), int(got["it"][i])) != (es, eit) or (got["cig"] is not None and es >= 0 and got["cig"][i] != (ecig or [])):
                    bad.append((pen_name, mode, c, stop, i, (int(got["s"][i]), int(got["it"][i])), (es, eit)))
    assert not bad and n_runs == 32, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", EDGE_SETS)
def test_low_memory_steps(pen_name, oracle, capfd):
    """step in {1, 7, 8, 9, 255, 256, 257, s - 1, s, s + 1} on a 3 kb pair, in the walk and the two-pass form, one and four columns per lane: snapshots at every
    penalty, on and next to block and epoch edges, and on the final penalty."""
    p = sm.PEN[pen_name]
    pair = synth_pair(830000 + sm._seed(pen_name), 3000, 0.08)
    s = oracle.align(*pair, make_opt(flag=0, **p))[0]
    assert s > 300
    bad = []
    for step in (1, 7, 8, 9, 255, 256, 257, s - 1, s, s + 1):
        kw = dict(flag=1, step=step, **p)
        exp = oracle_many(oracle, [pair], kw)
        assert exp[0][0] == s
        for mode in ("walk", "twopass"):
            for c in (1, 4):
                got = run_align(sm.route_tunables("alone", c) + sm.mode_tunables(mode), kw, [pair], capfd)
                assert got["kind"] == 1 and got["two_pass"] == (mode == "twopass"), (pen_name, step, mode, c)
                if (int(got["s"][0]), int(got["it"][0])) != exp[0][:2] or got["cig"][0] != exp[0][2]:
                    bad.append((pen_name, step, mode, c, (int(got["s"][0]), int(got["it"][0])), exp[0][:2]))
    assert not bad, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("pen_name", EDGE_SETS)
def test_automatic_columns_per_lane(pen_name, oracle, capfd, monkeypatch):
    """sys_c 0 on 16 workgroups: pairs whose lengths put the first pass's estimate on and one past window_cap(1), and steps that put the second pass's estimate
    there, launch the C the restated rule (sys_matrix.auto_c) says, per pass; the answers equal the oracle's."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = sm.PEN[pen_name]
    cap = sm.window_cap(1)
    ln_at = 5 * cap + 4      # est1 == cap: the last length that takes one column per lane
    assert sm.est1(ln_at) == cap and sm.est1(ln_at + 1) == cap + 1 and (ln_at + 1) // 2 <= 30000
    step_at = (cap - 8) // 2 - 2 * sm.nH(p)
    assert sm.est2(p, ln_at, step_at) <= cap < sm.est2(p, ln_at, step_at + 1)
    t, q = synth_pair(840000 + sm._seed(pen_name), ln_at // 2 + 40, 0.01)
    report = []
    try:
        for ln in (ln_at, ln_at + 1):
            tl = ln // 2
            pair = (t[:tl], q[:ln - tl])
            assert len(pair[0]) + len(pair[1]) == ln
            for mode, step in (("score", 0), ("cigar", 0), ("walk", step_at), ("walk", step_at + 1), ("twopass", step_at), ("twopass", step_at + 1)):
                kw = dict(flag=sm.mode_opt(mode)["flag"], step=step, **p)
                exp = oracle_many(oracle, [pair], dict(kw, flag=1), ("auto", pen_name, ln, step > 0))   # (no snapshot is due before such a step: one answer for both)
                c1, c2 = sm.auto_c(p, ln, step)
                assert (c1, c2) == (1 if ln == ln_at else 4, 4 if step == step_at + 1 else 1)
                got = run_align(sm.route_tunables("alone", 0) + sm.mode_tunables(mode), kw, [pair], capfd)
                label = f"{pen_name} tl + ql {ln} {mode} step {step}"
                want = [(i, ps, 1, sm.GROUP_WG, sm.GROUP_WG) for i, ps in sm.records(p, mode, c1, c2)]
                report.append(f"   {label}: {_show(got['records'])}")
                assert got["records"] == want, (label, _show(got["records"]), "expected", _show(want))
                assert got["kind"] == 1 and got["n_retries"] == 0 and got["two_pass"] == (mode == "twopass"), (label, got["n_retries"])
                check_answers(got, exp, label)
    finally:
        _report(report, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(sm.PEN_BEYOND))
def test_rings_of_257_rows_are_not_the_whole_device_kernels(tag, oracle, capfd):
    """o2 one higher than each 256-row set: refused under force_kind 1, the generic kernel's under default routing — where the 256-row set itself, on the same
    pair, is the whole-device kernel's."""
    pen, pen256 = sm.PEN_BEYOND[tag], sm.PEN[tag.replace("ring257", "ring256")]
    pair = synth_pair(850000, 20000, 0.03)
    eng = mw.Engine(0)
    try:
        eng.set("force_kind", 1)
        b = eng.upload(PackedBatch([pair]))
        with pytest.raises(RuntimeError, match="does not support these penalties"):
            b.align(mw.opt_init(**pen))
        b.free()
    finally:
        eng.close()
    for pp, kind in ((pen, 0), (pen256, 1)):
        exp = oracle_many(oracle, [pair], dict(flag=1, **pp))
        got = run_align((), dict(flag=1, **pp), [pair], capfd)
        assert got["kind"] == kind, (tag, pp, got["kind"])
        check_answers(got, exp, f"{tag} default routing kind {kind}")
