"""Every window-epoch case (tests/band_epoch_cases.py) has the property it is named for, by the oracle's band trace alone: a later change of the generators
must not empty a case that tests/test_band_epoch_gpu.py then runs for nothing."""
import numpy as np
import pytest

from oracle.pyoracle import make_opt
import band_matrix as bm
import band_epoch_cases as ec


def _trace(oracle, pen, t, q):
    (lohi, far), = bm._trace_all(oracle, pen, [(t, q)])
    return lohi, far


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_case_has_its_property(name, oracle):
    c = ec.case(oracle, name)
    g = ec.GEOM[c.nwk]
    folded = bool(c.band_fold and bm.pen_folds(c.pen) and g.T >= 512)
    assert c.pairs and len(c.where) == len(c.pairs), name
    for i, (t, q) in enumerate(c.pairs):
        lohi, far = _trace(oracle, c.pen, t, q)
        tl, ql, s = len(t), len(q), c.where[i]
        k = ec.keys(lohi, tl)
        assert bm.host_admits(g, c.pen, tl, ql) and bm.fits(g, folded, c.pen, lohi, far, tl, ql)[1], (name, i, "the geometry would hand the pair back")
        assert 2 <= s <= len(k), (name, i, s)
        if name.startswith("both-cross"):
            assert k[s - 1][:2] != k[s - 2][:2] and k[s - 1][2] != k[s - 2][2], (name, i, s, k[s - 2], k[s - 1])
        elif name.startswith("cross-shrink"):
            assert s % 256 == 0 and k[s - 1] != k[s - 2] and (k[s][1] > k[s - 1][1] or k[s][2] < k[s - 1][2]), (name, i, s, k[s - 2:s + 1])
        elif name.startswith("climb"):
            age = bm.age_out(folded, c.pen["e1"], c.pen["e2"])
            ups = ec.remaps_up(lohi, tl, age)
            # the mapping moves up at s, behind the ageing period, and the pair runs on behind it: those penalties start from a refreshed cache
            assert s in ups and s > age and s + 8 <= len(k), (name, i, s, ups[:3], len(k))
        elif name.startswith("ends-at-change"):
            assert s == len(k) and k[-1] != k[-2], (name, i, k[-2:])
        # several chunk boundaries are crossed on the way
        assert len(ec.change_penalties(lohi, tl)) >= 2, (name, i)
    if c.nwk == 32:   # the batch is of the default routing's 512-thread class: four slots under wide_slots 4
        assert all(bm.host_class(c.pen, len(t), len(q), wide_slots=4) == 1 for t, q in c.pairs), name


@pytest.mark.parametrize("name", ec.STOP_NAMES)
def test_stop_case_stops_at_a_change(name, oracle):
    _, nwk, (t, q), kw, s_star = ec.stop_case(oracle, name)
    lohi, far = _trace(oracle, ec.DEFAULT, t, q)
    k = ec.keys(lohi, len(t))
    assert 1 < s_star < len(k) and k[s_star - 1] != k[s_star - 2], (name, s_star)
    free = oracle.align(t, q, make_opt(**ec.DEFAULT))
    stopped = oracle.align(t, q, make_opt(**ec.DEFAULT, **kw))
    assert stopped[:2] != free[:2], (name, "the stop rule did not fire", stopped[:2], free[:2])
    c = ec.columns(lohi, len(t))
    cum = np.cumsum(c[:, 1] - c[:, 0] + 1)
    if "max_iter" in kw:   # the cells counted through s* - 1 stay within the limit, those through s* pass it
        assert cum[s_star - 2] <= kw["max_iter"] < cum[s_star - 1], (name, kw)
    else:
        assert kw["max_s"] == s_star - 1


def test_overflow_cases_meet_the_chunk_limit_first(oracle):
    for nwk, pairs, where in ec.overflow_cases(oracle):
        g = ec.GEOM[nwk]
        assert len(pairs) >= 3, nwk
        for i, (t, q) in enumerate(pairs):
            lohi, far = _trace(oracle, ec.DEFAULT, t, q)
            s = where[i]
            age = bm.age_out(0, 2, 1)
            assert bm.rule_chunks(g, age, lohi[:s - 1], len(t), len(q)) and not bm.rule_chunks(g, age, lohi[:s], len(t), len(q)), (nwk, i, s)
            assert ec.max_chunks(lohi[:s - 1], len(t), len(q)) <= nwk - 1, (nwk, i)   # every earlier window fits: this is the first that does not


def test_note_batches(oracle):
    narrow, wide = ec.note_batches(oracle)
    assert len(narrow) > 64 and len(wide) == len(narrow) + 1   # (a first align of up to 64 pairs is not started on four slots)
    assert all(bm.host_class(ec.DEFAULT, len(t), len(q)) == 1 for t, q in wide)
    assert max(ec.note_chunks(oracle, narrow)) <= 23
    assert 23 < ec.note_chunks(oracle, wide[-1:])[0] <= 31
