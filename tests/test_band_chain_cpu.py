"""Every case of the chunk-chain tests (tests/band_chain_cases.py) does what it is chosen for, by the sequences, the oracle's CIGAR and its band trace alone; every
case's widest window fits the 23 chunks of the three-slot kernel, so both geometries finish every pair; the four table kernels use no scratch."""
import re

import pytest

import band_matrix as bm
import band_epoch_cases as ec
import band_chain_cases as cc


def _fits_both(lohi, far, t, q, label):
    tl, ql = len(t), len(q)
    assert bm.host_admits(cc.G3, cc.DEFAULT, tl, ql), (label, "the forced route does not admit the pair")
    assert ec.max_chunks(lohi, tl, ql) <= 23, (label, "window beyond 23 chunks", ec.max_chunks(lohi, tl, ql))
    for g in (cc.G3, cc.G4):
        assert bm.fits(g, 1, cc.DEFAULT, lohi, far, tl, ql)[1], (label, g.K, "handed back")


@pytest.mark.parametrize("name", cc.GROUPS)
def test_every_pair_fits_23_chunks(name, oracle):
    pairs = cc.group(oracle, name)
    assert pairs
    for i, ((t, q), (lohi, far)) in enumerate(zip(pairs, cc.traces(oracle, name))):
        _fits_both(lohi, far, t, q, (name, i))


def test_stale_geometry_down(oracle):
    """The mapping moves down, the slot that wraps takes the chunk at the window's start, and a run of eight or more bases that ends at the end of a sequence
    is walked in that chunk — on 24 and on 32 chunks; over the pairs the run ends at the end of the target alone, of the query alone, and of both."""
    cases = cc.stale_down_pairs()
    exp = cc.expected(oracle, "stale")
    tr = cc.traces(oracle, "stale")
    for nwk in (24, 32):
        ends = set()
        for idx, ((t, q, end), (s, _, cig), (lohi, _)) in enumerate(zip(cases, exp, tr)):
            assert len(lohi) == s and 300 <= len(t) <= 3000 and 300 <= len(q) <= 3000, (idx, len(lohi), s)
            ev = cc.mapping_events(lohi, len(t), nwk)
            assert sum(not e.up for e in ev) >= 2, (nwk, idx, "the mapping moves down less than twice")
            hits = [h for h in cc.clamped_runs_in_new_chunks(t, q, cig, lohi, nwk) if not h[1].up]
            assert any(h[0] == end for h in hits), (nwk, idx, end, hits)
            _check_hits(hits, t, q, s, nwk, False, (nwk, idx))
            ends |= {h[0] for h in hits}
        assert ends == {"target", "query", "both"}, (nwk, ends)


def _check_hits(hits, t, q, s, nwk, up, label):
    """Every hit: the chunk is the slot's by that remap — another chunk's before, NWK away — the run is walked later, and it has no room left: rj = min(tl, ql - d) is met."""
    for kind, e, (i, j, n, pen) in hits:
        r = e.new.index((j - i + len(t) + 1) >> 8)
        assert e.up == up and e.old[r] == e.new[r] + (-nwk if up else nwk) and e.s < pen <= s and n >= cc.MIN_RUN, (label, e.s, pen)
        assert min(len(t) - i, len(q) - j) == n
        if kind == "target":
            assert i + n == len(t) and j + n < len(q)
        elif kind == "query":
            assert j + n == len(q) and i + n < len(t)


def test_stale_geometry_up(oracle):
    """The window's start climbs, the mapping follows behind the ageing period, slots wrap to the chunk NWK further up, and the pair runs on.  The first pairs
    then walk a run of eight or more bases, ending at the end of the target alone, of the query alone, and of both, in a chunk that a slot wrapped UP to — where
    a room bound left over from the chunk NWK lower would be NWK x 256 columns too lax — on 24 and on 32 chunks."""
    n_down, clamped = len(cc.stale_down_pairs()), cc.stale_up_clamped_pairs()
    exp, tr = cc.expected(oracle, "stale")[n_down:], cc.traces(oracle, "stale")[n_down:]
    pairs = cc.group(oracle, "stale")[n_down:]
    assert len(pairs) > len(clamped) and pairs[:len(clamped)] == [(t, q) for t, q, _ in clamped]
    for nwk in (24, 32):
        n_up, ends = 0, set()
        for idx, ((t, q), (s, _, cig), (lohi, _)) in enumerate(zip(pairs, exp, tr)):
            ups = [e for e in cc.mapping_events(lohi, len(t), nwk) if e.up]
            assert [e.s for e in ups] == ec.remaps_up(lohi, len(t), cc.AGE)
            for e in ups:
                assert e.s > cc.AGE and any(b == a + nwk for a, b in zip(e.old, e.new)), (nwk, e.s)
            n_up += any(e.s + 8 <= len(lohi) for e in ups)
            if idx < len(clamped):
                end = clamped[idx][2]
                assert len(lohi) == s and len(ups) >= 10, (nwk, idx, len(ups))
                hits = [h for h in cc.clamped_runs_in_new_chunks(t, q, cig, lohi, nwk) if h[1].up]
                assert any(h[0] == end for h in hits), (nwk, idx, end, hits)
                _check_hits(hits, t, q, s, nwk, True, (nwk, idx))
                assert all(((h[2][1] - h[2][0] + len(t) + 1) >> 8) >= nwk for h in hits)   # a chunk of the second round of the slots
                ends |= {h[0] for h in hits}
            else:
                assert 300 <= len(t) <= 3000 and 300 <= len(q) <= 3000
        assert n_up >= 2 + len(clamped), (nwk, n_up)
        assert ends == {"target", "query", "both"}, (nwk, ends)


def test_two_and_three_running_chunks(oracle):
    pairs, tr = cc.group(oracle, "multi"), cc.traces(oracle, "multi")
    widths = []
    for (t, q), (lohi, _) in zip(pairs, tr):
        tl, ql = len(t), len(q)
        widths.append(bm.widest(lohi))
        two, three = cc.penalties_with_running_chunks(lohi, tl, ql, cc.NW), cc.penalties_with_running_chunks(lohi, tl, ql, 2 * cc.NW)
        assert len(two) >= 100, (tl, ql, len(two))
        if widths[-1] > 4096:
            assert len(three) >= 100, (tl, ql, len(three))
    assert sum(2048 < w <= 4096 for w in widths) >= 2 and sum(w > 4096 for w in widths) >= 2, widths


def test_slots_start_and_stop_running(oracle):
    pairs, kinds = cc.toggle_pairs(oracle)
    assert {"cross-shrink", "both-cross", "ends-wide"} <= set(kinds), kinds
    for (t, q), kind, (lohi, _) in zip(pairs, kinds, cc.traces(oracle, "toggle")):
        k = ec.keys(lohi, len(t))
        if kind == "cross-shrink":
            s = ec.cross_then_shrink(lohi, len(t))
            assert s and s % 256 == 0 and (k[s][1] > k[s - 1][1] or k[s][2] < k[s - 1][2]), (kind, s)   # a chunk that ran at s no longer runs at s + 1
        elif kind == "both-cross":
            s = ec.both_cross(lohi, len(t))
            assert s and k[s - 1][2] != k[s - 2][2], (kind, s)   # a chunk runs at s that did not at s - 1
        else:
            assert k[-1][2] - k[-1][1] + 1 > cc.NW, kind   # at the pair's last penalty some wave still runs two chunks


def test_stop_where_a_wave_runs_two_chunks(oracle):
    (t, q), kw, s_star = cc.stop_case(oracle)
    lohi, = [x[0] for x in bm._trace_all(oracle, cc.DEFAULT, [(t, q)])]
    ga, gb = cc.chunks_met(lohi, len(t), len(q))[s_star - 1]
    assert gb - ga + 1 > cc.NW + 1 and kw == {"max_s": s_star - 1} and 1 < s_star < len(lohi)
    free, stopped = cc.expected(oracle, "multi")[0], cc.expected(oracle, "stop", **kw)[0]
    assert stopped[:2] != free[:2], ("the stop rule did not fire", stopped[:2], free[:2])


def test_plain_groups_are_the_table_form_s(oracle):
    import band_tab_cases as tc
    assert cc.group(oracle, "runs") is tc.group("runs") and cc.group(oracle, "tabalign") is tc.group("tabalign")


def test_table_kernels_use_no_scratch():
    notes = cc.table_kernel_notes()
    tab = {k: v for k, v in notes.items() if "wfa_band2_tab_kernel<" in k}
    got = {tuple(re.search(r"<([^>]*)>", k).group(1).replace(" ", "").split(",")[:5]) for k in tab}
    assert got == {("512", str(k), "2", "1", tb) for k in (3, 4) for tb in ("true", "false")}, got
    for k, v in tab.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)
