"""Every case of the table-form tests (tests/band_tab_cases.py) does what it is chosen for, by the sequences, the oracle's CIGAR and its band trace alone —
run lengths, where the runs end, the chunk, slot, lane and quad column they land in — and mwf_band2_tab.hip.o holds exactly the table form's four kernels."""
import band_matrix as bm
import band_tab_cases as tc


def _trace(oracle, t, q):
    (lohi, far), = bm._trace_all(oracle, tc.DEFAULT, [(t, q)])
    return lohi, far


def _check_runs(oracle, cases, label):
    """Every Run of every pair: exact length, the end it is named for, reached by the alignment behind a mismatch, inside the window of the penalty that reaches
    it; returns [(run, lands(...))]."""
    exp = tc.expected(oracle, label)
    seen = []
    for idx, ((t, q, runs), (s, _, cig)) in enumerate(zip(cases, exp)):
        tl, ql = len(t), len(q)
        lohi, far = _trace(oracle, t, q)
        assert len(lohi) == s, (label, idx, len(lohi), s)
        cells = {(i, j): pen for i, j, pen in tc.path_cells(t, q, cig)}
        # (the block is forced on three AND on four slots — "wide_slots" with a forced block — so the forced route's length rule admits the pair to both)
        assert bm.host_admits(tc.G3, tc.DEFAULT, tl, ql), (label, idx)
        for g in (tc.G3, tc.G4):
            assert bm.fits(g, 1, tc.DEFAULT, lohi, far, tl, ql)[1], (label, idx, g.K, "handed back")
        for r in runs:
            assert t[r.ti - 1] != q[r.qi - 1] and tc.lce(t, q, r.ti, r.qi) == r.n, (label, idx, r)
            room = min(tl - r.ti, ql - r.qi)
            if r.end == "room":
                assert room > r.n
            else:
                assert room == r.n and (tl - r.ti == r.n) == (r.end in ("target", "both")) and (ql - r.qi == r.n) == (r.end in ("query", "both")), (label, idx, r)
            # the alignment takes the substitution in front of the run and then the run's first cell: the run is probed at the penalty the substitution ends in
            assert (r.ti - 1, r.qi - 1) in cells and ((r.ti, r.qi) in cells or r.n == 0), (label, idx, r)
            pen = cells[(r.ti - 1, r.qi - 1)] + tc.DEFAULT["x"]
            assert 1 <= pen <= s, (label, idx, r, pen)
            for g in (tc.G3, tc.G4):
                where = tc.lands(g, lohi, tl, r.qi - r.ti, pen)
                assert where is not None, (label, idx, r, "outside the window of penalty", pen)
                _check_lands(g, lohi, tl, r, pen, where, (label, idx))
                seen.append((r, g.K, where))
    return seen


def _check_lands(g, lohi, tl, r, pen, where, label):
    """The chunk, wave, slot, lane and quad column a run is said to land in, by the kernel's own rules applied forwards: column = diagonal + tl + 1, a chunk is 256
    columns, a lane four; remap(): slot k of wave w holds chunk base + w + NW k, plus NWK when that lies below the mapping's first chunk."""
    chunk, wave, slot, lane, col = where
    c = r.qi - r.ti + tl + 1
    assert (chunk, lane, col) == (c // 256, (c % 256) // 4, c % 4), (label, r, where)
    nw, n = g.T // 64, bm.nwk(g)
    assert 0 <= wave < nw and 0 <= slot < g.K, (label, r, where)
    gl = max(int(lohi[pen - 1][0]) + tl, 1) >> 8
    held = gl - gl % n + wave + nw * slot
    assert (held + n if held < gl else held) == chunk, (label, r, where, gl)
    assert gl <= chunk < gl + n - 1, (label, r, where, "beyond the chunks the geometry holds")


def test_runs_around_full(oracle):
    cases = tc.runs_pairs()
    seen = _check_runs(oracle, cases, "runs")
    by = {(r.n, r.end) for r, _, _ in seen}
    assert by == {(n, e) for n in tc.RUNS for e in ("room",) + tc.ENDS}
    # the lengths straddle the new FULL, the old one, and the hand-over from the per-lane walk to the whole wave's
    assert {tc.FULL - 1, tc.FULL, tc.FULL + 1, tc.FULL_PLAIN - 1, tc.FULL_PLAIN, tc.FULL_PLAIN + 1} <= set(tc.RUNS) and max(tc.RUNS) == tc.WAVE_WALK_FROM + 1
    # every run length with room left lands in each of the four columns of a lane's quad (the two registers' low and high halves)
    for n in tc.RUNS:
        assert {w[4] for r, k, w in seen if r.n == n and r.end == "room" and k == 3} == {0, 1, 2, 3}, n
    assert {w[4] for r, k, w in seen if r.end != "room"} == {0, 1, 2, 3}
    assert len({w[3] for _, _, w in seen}) >= 4   # several lanes
    # chunks and slots: the pairs are 0.35 - 0.6 kb, their main diagonal's column lies in chunk 1 or 2 and in the first slot of wave 1 or 2 on both geometries
    assert {w[0] for _, _, w in seen} == {1, 2} and {(w[0], w[1], w[2]) for _, _, w in seen} <= {(1, 1, 0), (2, 2, 0)}, sorted({w[:3] for _, _, w in seen})


def test_final_runs(oracle):
    cases = tc.final_pairs()
    seen = _check_runs(oracle, cases, "final")
    assert {(r.n, len(q) - len(t)) for (t, q, (r,)) in cases} == {(n, d) for n in range(1, 10) for d in (-3, 0, 3)}
    for t, q, (r,) in cases:   # the run is the alignment's last: it ends in the end cell, on diagonal ql - tl
        assert r.qi - r.ti == len(q) - len(t) and r.ti + r.n == len(t)
    assert {w[4] for _, _, w in seen} == {0, 1, 2, 3}


def test_table_alignment(oracle):
    cases = tc.tabalign_pairs()
    exp = tc.expected(oracle, "tabalign")
    assert sorted(k for _, _, k in cases) == sorted([k for k in range(1, 16)] + [-k for k in range(1, 16)])
    pairs_seen = set()
    for (t, q, k), (s, _, cig) in zip(cases, exp):
        assert len(t) - len(q) == k
        lohi, far = _trace(oracle, t, q)
        assert bm.fits(tc.G3, 1, tc.DEFAULT, lohi, far, len(t), len(q))[1] and bm.fits(tc.G4, 1, tc.DEFAULT, lohi, far, len(t), len(q))[1]
        cells = tc.path_cells(t, q, cig)
        # where the alignment's runs start (behind a mismatch or the gap): target and query position mod 16, shifted against each other by the gap
        starts = [(i, j) for n, (i, j, _) in enumerate(cells) if t[i] == q[j] and (n == 0 or cells[n - 1][:2] != (i - 1, j - 1) or t[i - 1] != q[j - 1])]
        shifted = [(i, j) for i, j in starts if i - j == k]
        assert len(shifted) >= 40, (k, len(shifted))
        assert {i % 16 for i, _ in shifted} == set(range(16)), (k, "target residues")
        pairs_seen |= {(i % 16, j % 16) for i, j in starts}
        # runs that start in the last bases of a 2-bit dword: the eight bases of the table entry come from two dwords
        assert any(i % 16 > 8 for i, _ in shifted) and any(j % 16 > 8 for _, j in shifted)
    # every pair of different residues (equal residues are the main diagonal of the other groups' pairs)
    assert {(a, b) for a in range(16) for b in range(16) if a != b} <= pairs_seen, len(pairs_seen)


def test_long_runs(oracle):
    (ti, qi), (t, q) = tc.long_pairs()
    assert ti == qi and len(ti) == 3000
    r = tc.long_pairs(where=True)
    assert t[r.ti - 1] != q[r.qi - 1] and tc.lce(t, q, r.ti, r.qi) == r.n == 1500
    exp = tc.expected(oracle, "long")
    assert exp[0][0] == 0 and exp[1][0] > 0
    assert (r.ti, r.qi) in {c[:2] for c in tc.path_cells(t, q, exp[1][2])}   # the alignment walks the run: 8 + 64 bases per lane, the rest by the whole wave


def test_fuzz_fits_both_geometries(oracle):
    pairs = tc.fuzz_pairs()
    assert len(pairs) == 64 and all(500 <= len(t) <= 2500 and 500 <= len(q) <= 2500 for t, q in pairs)
    tr = bm._trace_all(oracle, tc.DEFAULT, pairs)
    for (t, q), (lohi, far) in zip(pairs, tr):   # no pair is handed back: a re-run on the GPU would be a finding
        assert bm.host_admits(tc.G3, tc.DEFAULT, len(t), len(q))
        assert bm.fits(tc.G3, 1, tc.DEFAULT, lohi, far, len(t), len(q))[1] and bm.fits(tc.G4, 1, tc.DEFAULT, lohi, far, len(t), len(q))[1]
    assert sum(abs(len(t) - len(q)) > 200 for t, q in pairs) >= 8


def test_object_holds_exactly_the_table_kernels():
    tab, others = tc.tab_object_kernels()
    assert tab == {bm.Inst(512, k, 2, 1, tb, 1, 0, 1) for k in (3, 4) for tb in (0, 1)}, tab
    assert not others, others
