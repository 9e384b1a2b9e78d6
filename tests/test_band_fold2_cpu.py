"""CPU-side checks of the inputs of tests/test_band_fold2_gpu.py (tests/band_fold2_cases.py): every case holds what it is chosen for — sized from the oracle's
CIGAR and band trace alone —, the penalty sets fall on the side of the routing rule they are meant for, the fixture tests/golden/band_fold2.jsonl (compiled
reference) is reproduced by the oracle, and mwf_band2_tab2.hip.o holds exactly the second fold's two kernels, without scratch or spilled VGPRs."""
import pytest

import band_matrix as bm
import band_epoch_cases as ec
import band_fold2_cases as fc
from conftest import load_golden, golden_inputs
from oracle.pyoracle import make_opt

O2, E2 = fc.DEFAULT["o2"], fc.DEFAULT["e2"]


def test_bound_covers_the_default_and_age_follows_it():
    assert O2 + E2 <= fc.FOLD2_MAX_LAG and fc.supported(fc.DEFAULT)
    assert fc.AGE == fc.FOLD2_MAX_LAG - E2 + max(fc.DEFAULT["e1"], E2) + 1 and fc.AGE >= O2 + 3 > bm.FOLD_MAX_LAG


def _only_gap(t, q, cig):
    ev = fc.gap_events(t, q, cig)
    assert len(ev) == 1, ev
    return ev[0]


def test_gaps_open_where_they_are_meant_to(oracle):
    gaps = fc.gap_pairs()
    exp = fc.expected(oracle, "gaps")
    kinds = set()
    for g, (s, _, cig) in zip(gaps, exp):
        sign, n, col, pen, second = _only_gap(g.t, g.q, cig)
        assert (sign, n, col) == (g.sign, g.n, g.col) and second and pen > 0, (g.kind, g.n, g.sign, (sign, n, col, pen, second))
        if g.kind.startswith("quad"):
            assert col & 3 == int(g.kind[4]) and col >> 8 == (col + sign * n) >> 8, (g.kind, col)
        else:   # the gap's two ends lie in neighbouring chunks: lane 63 of one slot, lane 0 of the next
            assert abs((col >> 8) - ((col + sign * n) >> 8)) == 1, (g.kind, col, n)
        kinds.add((g.kind, g.sign))
    assert kinds == {(k, s) for k in ("quad0", "quad1", "quad2", "quad3", "edge") for s in (1, -1)}
    assert {g.n for g in gaps} == set(fc.GAP_LENGTHS) and min(fc.GAP_LENGTHS) == 12 and max(fc.GAP_LENGTHS) == 40
    assert all(fc.fits_both(oracle, fc.group(oracle, "gaps")))
    assert all(300 <= len(t) <= 3000 and 300 <= len(q) <= 3000 for t, q in fc.group(oracle, "gaps"))


def test_wrap_gaps_cross_the_slot_wrap(oracle):
    gaps = fc.wrap_pairs()
    exp = fc.expected(oracle, "wrap")
    for g, (s, _, cig) in zip(gaps, exp):
        ev = fc.gap_events(g.t, g.q, cig)
        nwk = int(g.kind[4:])
        crossing = [e for e in ev if e[1] == g.n and e[0] == g.sign and e[4] and min(e[2], e[2] + e[0] * e[1]) < 256 * nwk <= max(e[2], e[2] + e[0] * e[1])]
        assert len(crossing) == 1 and crossing[0][2] == g.col, (g.kind, ev)
    assert all(fc.fits_both(oracle, fc.group(oracle, "wrap")))


def test_adjacent_gaps_are_closer_than_o2(oracle):
    pairs = fc.group(oracle, "adjacent")
    signs = set()
    for (t, q), (s, _, cig) in zip(pairs, fc.expected(oracle, "adjacent")):
        ev = fc.gap_events(t, q, cig)
        assert len(ev) == 2 and all(e[4] for e in ev), ev
        (s1, n1, c1, p1, _), (s2, n2, c2, p2, _) = ev
        assert 0 <= p2 - (p1 + O2 + n1 * E2) < O2, ev
        signs.add((s1, s2))
    assert signs == {(1, 1), (-1, -1), (1, -1), (-1, 1)}
    assert all(fc.fits_both(oracle, pairs))


def test_shrinks_take_both_edges_across_a_chunk_boundary(oracle):
    pairs = fc.group(oracle, "shrinks")
    assert 6 <= len(pairs) <= 64
    seen = set()
    for (t, q), (lohi, _) in zip(pairs, fc.traces(oracle, pairs)):
        cr = fc.shrink_crossings(lohi, len(t))
        assert cr, (len(t), len(q))
        # the chunk left behind ages for fc.AGE penalties: the pair runs on for at least that long behind some crossing shrink
        seen |= {(s, side) for s, side in cr if len(lohi) - s > fc.AGE}
    # (no shrink at 256 moves an edge of a pair of these sizes: band_fold2_cases' docstring; 512 is the first that does, for the start and for the end)
    assert seen >= {(512, "start"), (512, "end"), (768, "start"), (768, "end")}, sorted(seen)
    assert all(not [c for c in fc.shrink_crossings(lohi, len(t)) if c[0] == 256] for (t, q), (lohi, _) in zip(pairs, fc.traces(oracle, pairs)))
    assert all(fc.fits_both(oracle, pairs))


def test_climbing_pairs_remap_up_behind_the_new_period(oracle):
    pairs = fc.group(oracle, "climb")
    assert pairs
    for (t, q), (lohi, _) in zip(pairs, fc.traces(oracle, pairs)):
        late, early = ec.remaps_up(lohi, len(t), fc.AGE), ec.remaps_up(lohi, len(t), bm.FOLD_MAX_LAG)
        assert late and late != early, (len(t), len(q), late[:3], early[:3])


@pytest.mark.parametrize("tag", sorted(fc.PENS))
def test_penalty_sets_fall_on_their_side_and_match_the_reference(oracle, tag):
    p = fc.PENS[tag]
    assert fc.supported(p) == fc.TAKES[tag], (tag, p)
    vec = [v for v in load_golden(fc.GOLDEN) if v["id"].startswith(f"fold2-{tag}-")]
    assert len(vec) == len(fc.GOLDEN_SPECS)
    for v in vec:
        t, q = golden_inputs(v)
        s, it, cig = oracle.align(t, q, make_opt(**v["opt"]))
        e = v["expect"]
        assert (s, it, len(cig)) == (e["s"], e["n_iter"], e["n_cigar"]), v["id"]
        if "cigar" in e:
            assert [int(w) for w in cig] == e["cigar"], v["id"]
    assert all(fc.fits_both(oracle, fc.pen_pairs(), p)), tag


def test_rule_edges():
    b = fc.FOLD2_MAX_LAG
    assert fc.PENS["lag_bound"]["o2"] + 1 == b and fc.PENS["lag_above"]["o2"] + 1 == b + 1
    assert fc.PENS["o2_3"]["o2"] == 3 and fc.PENS["o2_2"]["o2"] == 2


def test_stops_and_end_cells(oracle):
    pairs = fc.stop_pairs(oracle)
    by_s, by_iter = fc.stop_opts(oracle)
    full = fc.expected(oracle, "stops")
    for kw in (by_s, by_iter):
        stopped = fc.expected(oracle, "stops", **kw)
        for (s, it, cig), (fs, fit, _) in zip(stopped, full):
            assert it < fit and not cig, (kw, s, it, fs, fit)
    # an end cell in a chunk that has run for more than o2 penalties: every gap pair ends on or next to the main diagonal, whose chunk ran from penalty 1
    gaps = fc.group(oracle, "gaps")
    ages = [fc.end_chunk_age(lohi, len(t), len(q)) for (t, q), (lohi, _) in zip(gaps, fc.traces(oracle, gaps))]
    assert min(ages) > O2, min(ages)


def test_fuzz_pairs(oracle):
    pairs = fc.group(oracle, "fuzz")
    assert len(pairs) == fc.FUZZ_N == 64 and all(300 <= len(t) <= 3000 and 300 <= len(q) <= 3200 for t, q in pairs)
    assert sum(fc.fits_both(oracle, pairs)) >= 60


def test_object_holds_the_two_kernels():
    got = fc.tab2_kernel_notes()
    insts, others = got
    assert not others, sorted(others)
    assert set(insts) == {bm.Inst(512, k, 2, 1, 0, 1, 0, 1) for k in (3, 4)}, sorted(insts)
    for i, n in insts.items():
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0 and n["vgpr_count"] <= 128, (i, n)
