"""The packed band kernel's five- and six-slot copies on biased offsets under the sets beyond (2,1) — (2,2), (1,1), (3,1), (3,2), (4,1): tests/band_biased_matrix.py —
beyond the one test per instantiation (tests/test_band_biased_matrix_gpu.py): the short end of the class, the default routing of the benchmark's shape, the range
check, gap runs across chunk edges and the slot wrap, a fuzz of pairs the class rule sends there, and the guard rails.  s, n_iter and every CIGAR word are compared
with the oracle's (or the compiled reference's stored answers): integer work, no tolerance."""
import numpy as np
import pytest

import band_matrix as bm
import band_deep_matrix as dm
import band_biased_matrix as xm
from conftest import load_golden, golden_inputs
from test_band_deep_cpu import cigar_matches
from test_band_deep_gpu import _launch_lines, _mutated, _check

PEN = xm.PEN
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROUTING = list(bm.COMMON_DEFAULT_ROUTING)   # the lane, mid and whole-device kernels off, no divergence estimate: the class rule alone routes
GOLD = {v["id"]: v for v in load_golden("band_biased.jsonl")}
_exp_cache: dict = {}


def _expected(oracle, key, pairs, kw):
    import fuzzlib as F
    from oracle.pyoracle import make_opt
    k = (key, tuple(sorted(kw.items())))
    if k not in _exp_cache:
        _exp_cache[k] = F.oracle_many(oracle, pairs, make_opt(**kw))
    return _exp_cache[k]


def _folds(tag: str) -> int:
    return int(xm.base.pen_folds(PEN[tag]))


def _copy(tag: str, K: int, tb: int, n: int, fold: int | None = None):
    """The launch record of the 512 x K copy on biased offsets for the set, with n pairs."""
    return (512, K, PEN[tag]["e1"], PEN[tag]["e2"], tb, 1, 1, _folds(tag) if fold is None else fold, n)


def _run(pairs, kw, tun, capfd):
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch
    capfd.readouterr()
    got = F.run_engine(PackedBatch(pairs), kw, tun)
    kinds, bands = _launch_lines(capfd.readouterr().err)
    return got, kinds, bands


# ---- (a) the short end ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a22", "e32"])
def test_short_end_straddles_plain_offsets(oracle, tag, capfd, monkeypatch):
    """e2 == 2: the worst-case penalty is ~4 L, pairs leave plain 16-bit offsets at ~6.55 kb.  Sixteen pairs of 6 300 - 7 000 bases @ 5 % on both sides of
    target length + bound = 32767: the packable ones start on 512 x 3 / 512 x 4, the others on the five-slot copy on biased offsets, none on the span geometry."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = PEN[tag]
    pairs = [synth_pair(820000 + i, 6300 + 40 * i, 0.05) for i in range(15)] + [golden_inputs(GOLD["biased7k-a22-cigar"])]
    packable = [len(t) + xm.base.penalty_bound(p, len(t), len(q)) < 32767 for t, q in pairs]
    assert 5 <= sum(packable) <= 11 and all(xm.base.host_class(p, len(t), len(q)) == (1 if pk else 14) for (t, q), pk in zip(pairs, packable))
    exp = _expected(oracle, ("short", tag), pairs, dict(flag=1, **p))
    for flag in (0, 1):
        got, kinds, bands = _run(pairs, dict(flag=flag, **p), ROUTING, capfd)
        _check(got, exp, f"short end {tag} flag {flag}", pairs)
        assert all(b[0] == 512 for b in bands) and all(k[0] == 2 for k in kinds), (kinds, bands)
        plain = [b for b in bands if b[6] == 0]
        biased = [b for b in bands if b[6] == 1]
        assert [b[1] in (3, 4) and b[8] == sum(packable) for b in plain] == [True], bands
        assert biased == [_copy(tag, 5, flag, len(pairs) - sum(packable))], bands
        assert got[3].n_retries == 0
        if tag == "a22":
            e = GOLD[f"biased7k-a22-{'cigar' if flag else 'score'}"]["expect"]
            assert (int(got[0][15]), int(got[1][15])) == (e["s"], e["n_iter"]) and (not flag or cigar_matches(got[2][15], e))


# ---- (b) default routing of the benchmark's shape -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a22", "e32"])
def test_default_routing_10kb_batch(oracle, tag, capfd, monkeypatch):
    """64 x 10 kb @ 5 % with no tunable set: the first band launch is 512 x 5 on biased offsets with all 64 pairs — folded for (2,2), as band_fold is 1 — and
    finishes them; oracle-equal, and under (2,2) the first pair is the compiled reference's 10 kb vector."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = PEN[tag]
    pairs = [golden_inputs(GOLD["biased10k-a22-cigar"])] + [synth_pair(830000 + i, 10000, 0.05) for i in range(63)]
    exp = _expected(oracle, ("route10k", tag), pairs, dict(flag=1, **p))
    for flag in (0, 1):
        got, kinds, bands = _run(pairs, dict(flag=flag, **p), [], capfd)
        st = got[3]
        assert kinds and kinds[0][0] == 2 and bands and bands[0] == _copy(tag, 5, flag, 64), (kinds[:2], bands[:2])
        assert st.kernel_kind == 2 and st.packed == 1 and st.block == 512 and st.n_retries == 0, (st.kernel_kind, st.packed, st.block, st.n_retries)
        _check(got, exp, f"10 kb {tag} flag {flag}", pairs)
        if tag == "a22":
            e = GOLD[f"biased10k-a22-{'cigar' if flag else 'score'}"]["expect"]
            assert (int(got[0][0]), int(got[1][0])) == (e["s"], e["n_iter"]) and (not flag or cigar_matches(got[2][0], e))
    if tag == "a22":   # band_fold 0: the unfolded copy
        got, kinds, bands = _run(pairs, dict(flag=0, **p), [("band_fold", 0)], capfd)
        assert bands and bands[0] == _copy(tag, 5, 0, 64, fold=0), bands[:2]
        _check(got, exp, "10 kb a22 band_fold 0", pairs)


# ---- (c) the range check ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(PEN))
def test_identical_and_near_identical_pairs(oracle, tag, capfd, monkeypatch):
    """0 % and 1 % divergence at 12 - 14 kb: offsets run to the target's end within a few penalties while everything else is dead — the values the range checks
    of the biased form look at (mwf_band2_kernel.h wide_bias).  The copies finish every pair; the 12 kb reference vector rides along."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = PEN[tag]
    pairs = [synth_pair(840000 + 10 * i + j, L, d) for i, L in enumerate((12000, 13001, 13999)) for j, d in enumerate((0.0, 0.01))] + [golden_inputs(GOLD[f"biased12k-{tag}-cigar"])]
    assert all(xm.base.host_class(p, len(t), len(q)) == 14 for t, q in pairs)
    exp = _expected(oracle, ("range", tag), pairs, dict(flag=1, **p))
    for flag in (0, 1):
        got, kinds, bands = _run(pairs, dict(flag=flag, **p), ROUTING, capfd)
        assert bands == [_copy(tag, 5, flag, len(pairs))] and got[3].n_retries == 0, (kinds, bands, got[3].n_retries)
        _check(got, exp, f"range {tag} flag {flag}", pairs)
        e = GOLD[f"biased12k-{tag}-{'cigar' if flag else 'score'}"]["expect"]
        assert (int(got[0][-1]), int(got[1][-1])) == (e["s"], e["n_iter"]) and (not flag or cigar_matches(got[2][-1], e))


# ---- (d) gap runs across chunk edges and the slot wrap --------------------------------------------------------------------------------------------
def gap_run_pairs(tag: str, col: int):
    """Related pairs (1 % substitutions) with ONE deletion or insertion of every length 1 ... 2 Lx + 3 (Lx: the length from which the second gap piece is the
    cheaper one; the lengths of test_band_deep_gpu.hazard_pairs and one more) and of 300.  Until the indel the path runs on the main diagonal, column tl + 1 of the
    window: target lengths col - 1 and col - 2 put it on the first column of a chunk and on the last of the one below, so a gap run to either side crosses the
    edge at its first step and its E/F pass through the edge table at every age."""
    p = PEN[tag]
    rng = np.random.default_rng(1000 * p["e1"] + 10 * p["e2"] + col)
    pairs = []
    for L in list(range(1, 2 * xm.crossover(p) + 4)) + [300]:
        for tl in (col - 1, col - 2):
            t = ACGT[rng.integers(0, 4, tl)]
            at = int(rng.integers(tl // 3, 2 * tl // 3))
            q = _mutated(rng, t, 0.01)
            pairs.append((t.tobytes(), np.concatenate([q[:at], q[at + L:]]).tobytes()))
            pairs.append((t.tobytes(), np.concatenate([q[:at], ACGT[rng.integers(0, 4, L)], q[at:]]).tobytes()))
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 6])
@pytest.mark.parametrize("tag", sorted(PEN))
def test_gap_runs_across_chunk_edges_and_the_slot_wrap(oracle, tag, K, capfd, monkeypatch):
    """Five slots: 40 chunks, the slot mapping wraps between chunks 39 and 40, column 10 240 — reachable on the main diagonal only where a 10 kb pair has already
    left plain offsets (e2 == 2); the other sets cross the edge of chunk 48 there.  Six slots (one 18 kb pair in the batch makes the launch a six-slot one):
    48 chunks, the wrap at column 12 288.  With and without traceback."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = PEN[tag]
    col = 12288 if K == 6 or p["e2"] == 1 else 10240
    pairs = gap_run_pairs(tag, col) + ([synth_pair(850000, 18000, 0.01)] if K == 6 else [])
    assert all(xm.base.host_class(p, len(t), len(q)) == 14 for t, q in pairs)
    assert (max(len(t) + len(q) for t, q in pairs) > xm.base.BIASED5_MAX_LEN) == (K == 6)
    exp = _expected(oracle, ("gaps", tag, K), pairs, dict(flag=1, **p))
    for flag in (1, 0):
        got, kinds, bands = _run(pairs, dict(flag=flag, **p), ROUTING, capfd)
        assert bands and bands[0] == _copy(tag, K, flag, len(pairs)), (kinds[:2], bands[:2])
        _check(got, exp, f"gap runs {tag} K {K} flag {flag}", pairs)
        assert got[3].n_retries == 0, got[3].n_retries


# ---- (e) fuzz of pairs the class rule sends to the copies ----------------------------------------------------------------------------------------
FUZZ_SEED = {"a22": 31, "edit": 32, "e31": 33, "e32": 34, "e41": 35}


def fuzz_set(tag: str):
    """Pairs of 7 - 14 kb that the class rule gives to the copies under the set: related at 0.5 - 6 %, with long indels, of skewed lengths, one sequence a piece
    of the other (the unrelated pairs are the matrix's: the oracle needs tens of seconds for more of them)."""
    from miniwfa_amd.synth import synth_pair, skewed_pairs, random_seq
    seed, p = FUZZ_SEED[tag], PEN[tag]
    rng = np.random.default_rng(seed)
    cand = [synth_pair(seed * 1000 + i, int(rng.integers(7000, 14000)), float(rng.choice([0.005, 0.02, 0.04, 0.06])), int(i % 3), 400) for i in range(12)]
    cand += skewed_pairs(seed, 2, 7000, 12000)
    a = random_seq(seed + 10, 12000)
    cand += [(a, a[:10800]), (a[1200:], a)]
    return [(t, q) for t, q in cand if xm.base.host_class(p, len(t), len(q)) == 14]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(PEN))
def test_class_fuzz(oracle, tag, capfd, monkeypatch):
    """Score and CIGAR against the oracle; the first launch is the copy with every pair, and what it hands back is bounded by the pairs whose oracle band trace
    leaves its chunks or meets one of its hand-back rules."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    p = PEN[tag]
    pairs = fuzz_set(tag)
    assert len(pairs) >= 8, len(pairs)
    K = 6 if max(len(t) + len(q) for t, q in pairs) > xm.base.BIASED5_MAX_LEN else 5
    bound = xm.not_fit_count(oracle, pairs, p, K)
    exp = _expected(oracle, ("fuzz", tag), pairs, dict(flag=1, **p))
    for flag in (0, 1):
        got, kinds, bands = _run(pairs, dict(flag=flag, **p), ROUTING, capfd)
        assert bands and bands[0] == _copy(tag, K, flag, len(pairs)), (kinds[:2], bands[:2])
        _check(got, exp, f"fuzz {tag} flag {flag}", pairs)
        assert got[3].n_retries <= bound, (tag, flag, got[3].n_retries, bound)


# ---- (f) guard rails ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tun", [("wide_slots", 3), ("band_span", 2)], ids=["wide_slots3", "band_span2"])
def test_tunables_keep_the_batch_on_the_span_geometry(oracle, tun, capfd, monkeypatch):
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(860000 + i, 10000, 0.05) for i in range(16)]
    exp = _expected(oracle, "rails10k", pairs, dict(flag=1, **PEN["a22"]))
    got, kinds, bands = _run(pairs, dict(flag=1, **PEN["a22"]), ROUTING + [tun], capfd)
    assert bands and bands[0][:2] == (1024, 5) and bands[0][8] == len(pairs) and not any(b[6] for b in bands), bands
    _check(got, exp, f"a22 {tun}", pairs)


@pytest.mark.gpu
def test_a_pair_with_an_n_never_takes_the_copies(oracle, capfd, monkeypatch):
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(861000 + i, 10000, 0.03) for i in range(8)]
    pairs[3] = (pairs[3][0][:500] + b"N" + pairs[3][0][501:], pairs[3][1])
    exp = _expected(oracle, "rails-n", pairs, dict(flag=1, **PEN["a22"]))
    got, kinds, bands = _run(pairs, dict(flag=1, **PEN["a22"]), ROUTING, capfd)
    assert _copy("a22", 5, 1, 7) in bands and not any(b[6] and b[8] != 7 for b in bands), (kinds, bands)
    _check(got, exp, "a22 with an N", pairs)


@pytest.mark.gpu
def test_band_pack_0_keeps_everything_off_the_band_kernel(oracle, capfd, monkeypatch):
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(862000 + i, 10000, 0.03) for i in range(8)]
    exp = _expected(oracle, "rails-pack0", pairs, dict(flag=1, **PEN["a22"]))
    got, kinds, bands = _run(pairs, dict(flag=1, **PEN["a22"]), ROUTING + [("band_pack", 0)], capfd)
    assert kinds and not bands, bands[:2]
    _check(got, exp, "a22 band_pack 0", pairs)


@pytest.mark.gpu
def test_42_launches_what_it_launched(oracle, capfd, monkeypatch):
    """(4,2) is not on the band kernel at all: a 10 kb batch launches no band kernel."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pen = dm.NOT_BUILT_PEN["e42"]
    pairs = [synth_pair(863000 + i, 10000, 0.03) for i in range(8)]
    exp = _expected(oracle, "rails-e42", pairs, dict(flag=1, **pen))
    got, kinds, bands = _run(pairs, dict(flag=1, **pen), ROUTING, capfd)
    assert kinds and not bands, bands[:2]
    _check(got, exp, "e42", pairs)


@pytest.mark.gpu
def test_21_class_14_launches_are_unchanged(oracle, capfd, monkeypatch):
    """The default set's copies stay the default unit's: 15 kb pairs start on <512, 5, 2, 1, TB, 1, 1, FOLD 1>, an 18 kb pair in the batch makes it six slots."""
    from miniwfa_amd.synth import synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(864000 + i, 15000, 0.03) for i in range(8)]
    exp = _expected(oracle, "rails-21", pairs, dict(flag=1))
    for flag in (0, 1):
        got, kinds, bands = _run(pairs, dict(flag=flag), ROUTING, capfd)
        assert bands == [(512, 5, 2, 1, flag, 1, 1, 1, 8)], bands
        _check(got, exp, f"default set flag {flag}", pairs)
    long = pairs + [synth_pair(864100, 18000, 0.02)]
    got, kinds, bands = _run(long, dict(flag=0), ROUTING, capfd)
    assert bands and bands[0] == (512, 6, 2, 1, 0, 1, 1, 1, 9), bands
