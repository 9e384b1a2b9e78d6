"""Every case of the tests of the table form's every-penalty tail (tests/band_stage_cases.py) does what it is chosen for, by the oracle's band trace alone: where the
iteration budget runs out, which slot's chunk holds the end column at the pair's last penalty, for how long that chunk runs before the window reaches the column;
and the four table kernels still use no scratch and at most 128 VGPRs."""
import band_matrix as bm
import band_chain_cases as cc
import band_stage_cases as sc


def test_budget_runs_out_where_a_wave_runs_two_chunks(oracle):
    (t, q), s_star, cum, cases = sc.budget_cases(oracle)
    assert [c[0] for c in cases] == list(sc.BUDGET_LABELS)
    (lohi, far), = bm._trace_all(oracle, sc.DEFAULT, [(t, q)])
    for g in (sc.G3, sc.G4):
        assert sc.fits(lohi, far, t, q, g), g.K
    ga, gb = cc.chunks_met(lohi, len(t), len(q))[s_star - 1]
    assert gb - ga + 1 > sc.NW + 1 and 1 < s_star < len(lohi) - 1
    free = sc.expected(oracle, "budget")[0]
    assert free[0] == len(lohi) and free[1] == int(cum[-1]), (free[:2], len(lohi), int(cum[-1]))   # n_iter IS the count the budget is compared with
    by = dict(cases)
    assert by["exact"] == int(cum[s_star - 1]) and by["below"] == by["exact"] - 1 and by["above"] == by["exact"] + 1
    assert cum[s_star - 1] > cum[s_star - 2] + 1   # (so "below" still lets penalty s* - 1 pass)
    # the stop rule is "more than max_iter": one below stops at s*, exactly at and one above stop a penalty later; n_iter says where
    for label, at in (("below", s_star), ("exact", s_star + 1), ("above", s_star + 1)):
        s, n_iter, _ = sc.expected(oracle, "budget", max_iter=by[label])[0]
        assert s == -1 and n_iter == int(cum[at - 1]), (label, s, n_iter, int(cum[at - 1]))
    assert by["big"] > 1 << 32 and sc.expected(oracle, "budget", max_iter=by["big"])[0][:2] == free[:2]


def test_end_column_in_every_slot(oracle):
    pairs, tr = sc.endslot_group(), sc.traces(oracle)
    exp = sc.expected(oracle, "endslot")
    seen, leads, cols = set(), [], set()
    for (t, q), (lohi, far), (s, _, _) in zip(pairs, tr, exp):
        tl, ql = len(t), len(q)
        assert s == len(lohi) > 0 and 300 <= tl <= 3000, (tl, ql, s)
        cols.add((ql + 1) & 255)
        for g in (sc.G3, sc.G4):
            if not sc.fits(lohi, far, t, q, g):
                continue
            k, _ = sc.end_slot(lohi, tl, ql, bm.nwk(g))
            seen.add((g.K, k))
        assert sc.fits(lohi, far, t, q, sc.G4), (tl, ql, "handed back on four slots")
        leads.append(sc.bit_lead(lohi, tl, ql))
    assert seen == {(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)}, sorted(seen)
    assert {0, 255} <= cols, cols
    # the chunk of the end column runs for a hundred penalties and more before the window reaches the column (the insertion pairs), and from penalty 1 on (the others)
    assert max(leads) >= 100 and min(leads) == 0, leads


def test_which_pairs_run_on_three_slots(oracle):
    """The GPU test runs a pair on three slots iff this says so: every pair but the one whose window passes 23 chunks."""
    pairs, tr = sc.endslot_group(), sc.traces(oracle)
    on3 = [sc.fits(lohi, far, t, q, sc.G3) for (t, q), (lohi, far) in zip(pairs, tr)]
    assert sum(on3) >= len(pairs) - 1 and all(on3[:4]), on3


def test_table_kernels_registers():
    import band_tab_cases as tc
    got = bm.device_kernels(tc.TAB_OBJ, "wfa_band2_tab_kernel")
    assert not isinstance(got, str), got
    notes = list(got[0].values()) + list(got[1].values())
    scratch = [k["private_segment_fixed_size"] for k in notes]
    vgprs = [k["vgpr_count"] for k in notes]
    spilled = [k["vgpr_spill_count"] for k in notes]
    assert len(scratch) == len(vgprs) == len(spilled) == 4, (scratch, vgprs, spilled)
    assert scratch == [0] * 4 and spilled == [0] * 4 and max(vgprs) <= 128, (scratch, vgprs, spilled)
