"""The table of the ends-free / extension kernel (tests/ends_matrix.py) without a GPU: the restatements with the shrink can be trusted — against the oracle
where the allowances are zero, against the DP everywhere — and the inputs hold what tests/test_ends_matrix_gpu.py relies on.  Every condition is asserted on
the references alone; none is skipped."""
import multiprocessing
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from oracle.pyoracle import make_opt
import band_matrix as bm
import ends_matrix as em
import ends_ref as er
import ext_ref as xr
from test_ext_cpu import ENDS_KERNELS

FREE = er.FREE


def _pool():
    """The restatements and the DPs (a wide pair's: 4200 rows of 4200 columns, half a second) side by side on fresh host processes."""
    return ProcessPoolExecutor(min(8, bm.ORACLE_THREADS), mp_context=multiprocessing.get_context("spawn"))


@pytest.fixture(scope="module", autouse=True)
def restated():
    """The restatements' answers for every run of the table, computed once for the whole file."""
    with _pool() as ex:
        em.warm(ex)


def _narrowed(shrinks):
    return any((e[1], e[2]) != (e[3], e[4]) for e in shrinks if e[0] == 256)


def test_table_and_launch_rule():
    assert {(i.T, "true" if i.EXT else "false") for i in em.MATRIX} == ENDS_KERNELS and len(set(em.MATRIX)) == 8
    assert {(i.TB, i.EXT) for i in em.MATRIX if i.T == 256} == {(i.TB, i.EXT) for i in em.MATRIX if i.T == 512} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for inst in em.MATRIX:
        assert len(em.cells(inst)) == 12 * (2 if inst.EXT else 5)
        for name, cfg in em.cells(inst):
            p, pairs = em.PEN[name], em.batch(inst, name, cfg)
            assert em.window_block(p, pairs) == inst.T, (em.inst_id(inst), name, cfg)
            if inst.T == 512:   # every pair alone takes the wide form, whatever the others do
                assert 3 - (not inst.EXT and cfg[:2] != (FREE, FREE)) == len(pairs)
                assert all(len(t) + len(q) + 1 >= em.WIDE_WINDOW and 2 * bm.penalty_bound(p, len(t), len(q)) + 3 >= em.WIDE_WINDOW for t, q in pairs), (name, cfg)
            else:
                assert 24 <= len(pairs) <= 32 and all(em.window_block(p, [tq]) == 256 for tq in pairs)
                assert len(pairs) == 28 + len(em._NARROW_EXTRA.get(name, ())) and all(max(len(t), len(q)) <= 640 for t, q in pairs[:28])   # (a gapped pair's longer side)
                assert {(b"", b""), (b"A", b"C"), (b"A", b"A")} <= set(pairs) and any(t == q and len(t) > 100 for t, q in pairs)
                assert any(not t and q for t, q in pairs) and any(t and not q for t, q in pairs)
    w = em._wide()
    assert len(w["b"][0]) + 1 > 8 * 512 and sorted(w["b_rot"][0]) == sorted(w["b"][0]) and w["b_rot"][1] == w["b"][1]


def test_fixture_holds_the_restated_answers():
    """tests/golden/ends_matrix.jsonl, line by line, is what the restatements give today (the GPU tests read it instead of computing it)."""
    runs = em.fixture_runs()
    assert sorted(em._golden()) == sorted(r[0] for r in runs) and len(runs) == 2 * 12 * (5 + 2) + 2
    for key, pairs, pen, ext, cfg in runs:
        assert em._golden()[key] == em.restated(pairs, pen, ext, cfg), key


def test_zero_allowances_equal_the_oracle(oracle):
    """wfa_ends with the shrink: s, n_iter and the band of every penalty are the oracle's, on the narrow batch — pairs beyond 256 and 512 among them — and on the
    wide pairs (a) and (c), under all twelve sets; and wfa_ext without a drop rule sweeps what wfa_ends(0, FREE, 0, FREE) sweeps."""
    n = n256 = n512 = 0
    for name in em.SETS:
        pen, opt = em.pen_tuple(name), make_opt(**em.PEN[name])
        for tq in em.narrow_pairs(name) + em.wide_pairs(0, (0, 0, 0, 0)):
            got, trace, _ = em.ends_full(tq, pen, (0, 0, 0, 0))
            s, n_iter, _ = oracle.align(*tq, opt)
            assert (got[0], got[1], got[2], got[3]) == (s, n_iter, len(tq[0]), len(tq[1])), (name, len(tq[0]), len(tq[1]))
            assert list(trace) == oracle.band_trace(*tq, opt, cap=s + 2), (name, len(tq[0]), len(tq[1]))
            n, n256, n512 = n + 1, n256 + (s >= 257), n512 + (s >= 513)
        for tq in em.narrow_pairs(name):
            A = em.EXT_NARROW[0][0]
            x, e = em.want_ext(tq, pen, A, -1), er.wfa_ends(*tq, pen, (0, FREE, 0, FREE))
            assert (x.s_stop, x.n_iter, x.why) == (e[0], e[1], 0), (name, len(tq[0]), len(tq[1]))
    print(f"{n} pairs against the oracle, {n256} beyond penalty 256, {n512} beyond 512")
    assert n256 >= 100 and n512 >= 40


def test_restatement_equals_the_dp():
    """Restated s == DP optimum for every (pair, set, allowances) of both batches and of the persistent-loop pairs; check_against_dp's conditions for every EXT
    case without a drop rule."""
    ends, ext = {}, {}
    for inst in em.MATRIX:
        for name, cfg in em.cells(inst):
            pen = em.pen_tuple(name)
            for tq in em.batch(inst, name, cfg):
                if not inst.EXT:
                    ends[(tq, pen, cfg)] = None
                elif cfg[1] == -1:
                    ext[(tq, pen, cfg[0])] = None
    for tq in em.loop_pairs():
        ends[(tq, em.LOOP_PEN, em.LOOP_ALLOW)] = None
    ends, ext = list(ends), list(ext)
    cells = [em.want_ext(tq, pen, A, -1) for tq, pen, A in ext]
    with _pool() as ex:   # (the longest first)
        dp_x = ex.map(xr.dp_answer, *zip(*[(tq[0], tq[1], pen, A, r.te, r.qe) for (tq, pen, A), r in zip(ext, cells)]), chunksize=4)
        dp_e = ex.map(er.dp_score, *zip(*[(tq[0], tq[1], pen, allow) for tq, pen, allow in ends]), chunksize=8)
        for (tq, pen, A), r, (V, s_end, D_cell) in zip(ext, cells, dp_x):
            assert (r.V, r.s_stop, r.why) == (V, s_end, 0) and D_cell == r.s and A * (r.te + r.qe) - 2 * r.s == r.V, (len(tq[0]), len(tq[1]), pen, A, tuple(r))
        for (tq, pen, allow), s in zip(ends, dp_e):
            assert em.want_ends(tq, pen, allow)[0] == s, (len(tq[0]), len(tq[1]), pen, allow)
    print(f"{len(ends)} ends-free answers and {len(ext)} extensions against the DP")
    assert len(ends) >= 12 * 5 * 26 and len(ext) >= 12 * 27


def test_coverage_conditions():
    """What the GPU tests are there for, on the restatements alone.

    One condition holds in another form than for the ends-free pass.  An extension's shrink cannot narrow its band: the pass starts from one cell inside the
    matrix, an offset leaves the matrix only through its last row or column, one step at a time, and the pass ends at the first penalty that has a cell ON either —
    so while it runs every live offset is inside the matrix; a column that was live once is live again x penalties later (the mismatch term), within any nH
    slices; and the band only ever grows onto live cells.  Every column of the band is good at every shrink.  What is asserted for EXT is therefore that every
    shrink leaves the band as it was (a kernel whose good words or slice windows are stale WOULD narrow it, and n_iter would show it) and that, per set, at
    least four pairs run through one."""
    s_max, ext_end_513, ext_drop_257 = 0, 0, 0
    for name in em.SETS:
        pen = em.pen_tuple(name)
        pairs = em.narrow_pairs(name)
        beyond = {i for i, tq in enumerate(pairs) for a in em.ALLOW if a != (0, 0, 0, 0) and em.want_ends(tq, pen, a)[0] >= 257}
        assert len(beyond) >= 4, (name, beyond)
        narrowed, x_shrunk = set(), set()
        for i, tq in enumerate(pairs):
            for a in em.ALLOW:
                w = em.want_ends(tq, pen, a)
                s_max = max(s_max, w[0])
                if _narrowed(em.ends_full(tq, pen, a)[2]):
                    narrowed.add(i)
            for A, Z in em.EXT_NARROW:
                r = em.want_ext(tq, pen, A, Z)
                ext_end_513 += r.why == 0 and r.s_stop >= 513
                ext_drop_257 += r.why == 1 and r.s_stop >= 257
                sh = em.ext_full(tq, pen, A, Z)[2]
                assert all((e[1], e[2]) == (e[3], e[4]) for e in sh), (name, i, sh)
                if sh:
                    x_shrunk.add(i)
        print(f"{name}: {len(beyond)} pairs beyond 256 under non-zero allowances; the shrink at 256 narrows the band of {len(narrowed)} pairs (ends form); {len(x_shrunk)} pairs run through a shrink under EXT")
        assert len(narrowed) >= 2 and len(x_shrunk) >= 4, (name, narrowed, x_shrunk)
    print(f"largest s of the narrow batch {s_max}; EXT: {ext_end_513} ends at s_stop >= 513, {ext_drop_257} drops at s_stop >= 257")
    assert s_max >= 513 and ext_end_513 >= 1 and ext_drop_257 >= 1
    # the wide batch: (c) crosses 256 under every set but the cheapest, (b)'s band is cut by a shrink, and the drop of EXT_WIDE ends (c) beyond 256
    w = em._wide()
    A, Z = em.EXT_WIDE[1]
    for name in em.SETS:
        pen = em.pen_tuple(name)
        if name != "edit":
            assert em.want_ends(w["c"], pen, (0, 0, 0, 0))[0] >= 257 and em.want_ext(w["c"], pen, 1, -1).s_stop >= 257, name
        r = em.want_ext(w["c"], pen, A, Z)
        assert (r.why == 1 and r.s_stop >= 257) == (name in em.DROP_WIDE_SETS), (name, tuple(r))
    assert len(em.DROP_WIDE_SETS) == 10
    cut = [name for name in em.SETS if _narrowed(em.ends_full(w["b"], em.pen_tuple(name), (FREE, FREE, 0, 0))[2])]
    print("the shrink at 256 cuts the band of (b), 6201 columns at the origin, under", cut)
    assert len(cut) >= 8 and "default" in cut, cut


def _eq_runs(words):
    """[(target begin, query begin, length)] of a global CIGAR's = runs."""
    j = i = 0
    out = []
    for wd in words:
        op, n = wd & 0xf, wd >> 4
        if op == 7:
            out.append((j, i, n))
        j, i = j + (n if op in (7, 8, 2) else 0), i + (n if op in (7, 8, 1) else 0)
    return out


def test_long_exact_runs(oracle):
    """Pair (a): an = run of at least 1100 bases that begins beyond base 511 of both sequences (the back-match takes whole 512-base trips and ends inside one);
    pair (c): an = run of at least 1400 bases from the begin of both (it leaves the 512-base trips unfinished).  By the oracle's CIGAR under every set."""
    w = em._wide()
    for name in em.SETS:
        opt = make_opt(flag=1, **em.PEN[name])
        runs = _eq_runs(oracle.align(*w["a"], opt)[2])
        assert any(n >= 1100 and j > 511 and i > 511 for j, i, n in runs), (name, max(runs, key=lambda r: r[2]))
        runs = _eq_runs(oracle.align(*w["c"], opt)[2])
        assert runs[0][:2] == (0, 0) and runs[0][2] >= 1400, (name, runs[0])


def test_persistent_loop_pairs():
    pairs = em.loop_pairs()
    assert len(pairs) == 32 and len(set(pairs)) == 32 and sum(max(len(t), len(q)) <= 120 for t, q in pairs) == 26
    s = [em.want_ends(tq, em.LOOP_PEN, em.LOOP_ALLOW)[0] for tq in pairs]
    assert sum(v >= 257 for v in s) >= 6, s
    x = [em.want_ext(tq, em.LOOP_PEN, *em.LOOP_EXT) for tq in pairs]
    assert 4 <= sum(r.why for r in x) <= 28 and any(r.s > 0 for r in x)
    order = em.loop_order()
    assert len(order) == em.LOOP_COPIES and set(order.tolist()) == set(range(32)) and (np.bincount(order) == em.LOOP_COPIES // 32).all()
    assert (order[:32] != np.arange(32)).any()
