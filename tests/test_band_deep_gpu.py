"""The packed band kernel under gap extensions of 3 and 4 — (e1, e2) = (3,1), (3,2), (4,1), the sets of tests/band_deep_matrix.py — beyond the one test per
instantiation (tests/test_band_deep_matrix_gpu.py): gap runs around the piece crossover placed on chunk edges, forced-geometry fuzz, the default routing,
chain mode and the guard rails.  s, n_iter and every CIGAR word are compared with the oracle's (or the compiled reference's stored answers): integer work,
no tolerance."""
import re

import numpy as np
import pytest

import band_deep_matrix as dm
from conftest import load_golden, golden_inputs
from test_band_deep_cpu import cigar_matches

PEN = dm.DEEP_PEN
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KIND_LINE = re.compile(r"\[libmwf_hip\] kernel kind (-?\d+): block (\d+) packed (\d+) .* (\d+) pairs")
BAND_LINE = re.compile(r"\[libmwf_hip\] band2 launch: T (\d+) K (\d+) E1 (\d+) E2 (\d+) TB (\d+) S2 (\d+) BI4 (\d+) FOLD (\d+), (\d+) pairs")
_exp_cache: dict = {}


def _expected(oracle, key, pairs, kw):
    """The oracle's answers, computed once per (input set, options) and shared."""
    import fuzzlib as F
    from oracle.pyoracle import make_opt
    k = (key, tuple(sorted(kw.items())))
    if k not in _exp_cache:
        _exp_cache[k] = F.oracle_many(oracle, pairs, make_opt(**kw))
    return _exp_cache[k]


def _check(got, exp, label, pairs):
    import fuzzlib as F
    bad = []
    F.compare(got, exp, label, pairs, bad, False)
    assert not bad, bad[:6]


def _launch_lines(err):
    """([(kind, block, packed, pairs)], [(T, K, E1, E2, TB, S2, BI4, FOLD, pairs)]) of the aligns whose MWF_DEBUG output is `err`."""
    return [tuple(map(int, m.groups())) for m in KIND_LINE.finditer(err)], [tuple(map(int, m.groups())) for m in BAND_LINE.finditer(err)]


# ---- gap-depth hazards -----------------------------------------------------------------------------------------------------------------------
def _mutated(rng, t: np.ndarray, p: float) -> np.ndarray:
    q = t.copy()
    hit = rng.random(len(q)) < p
    q[hit] = ACGT[(np.searchsorted(ACGT, q[hit]) + rng.integers(1, 4, int(hit.sum()))) & 3]
    return q


def hazard_pairs(tag: str, chunk_k: int):
    """Related pairs (1 % substitutions) with ONE deletion or insertion of every length 1 ... 2 Lx + 2 (Lx: the length from which the second gap piece is
    the cheaper one) and of 300.  Until the indel the path runs on the main diagonal, column tl + 1 of the window; the target lengths chunk_k x 256 - 1 and
    - 2 put that column on the first column of a chunk and on the last of the one below, so a gap run to either side leaves the chunk — on the one-wave
    geometry the slot — at its first step, and its E/F pass through the edge table at every age.  Then tandem repeats (unit 1 ... 7: homopolymers among
    them) with whole and broken units missing: every E1/E2, F1/F2 and open-versus-extend tie is live."""
    p = PEN[tag]
    rng = np.random.default_rng(1000 * p["e1"] + 10 * p["e2"] + chunk_k)
    pairs = []
    for L in list(range(1, 2 * dm.crossover(p) + 3)) + [300]:
        for tl in (chunk_k * 256 - 1, chunk_k * 256 - 2):
            t = ACGT[rng.integers(0, 4, tl)]
            at = int(rng.integers(tl // 3, 2 * tl // 3))
            q = _mutated(rng, t, 0.01)
            pairs.append((t.tobytes(), np.concatenate([q[:at], q[at + L:]]).tobytes()))                          # deletion
            pairs.append((t.tobytes(), np.concatenate([q[:at], ACGT[rng.integers(0, 4, L)], q[at:]]).tobytes()))   # insertion
    tl = chunk_k * 256 - 1
    for unit in (1, 2, 3, 5, 7):
        rep = np.resize(ACGT[rng.integers(0, 4, unit)], tl)
        for cut in (1, unit, unit + 1, 3 * unit, dm.crossover(p), dm.crossover(p) + 1, 2 * dm.crossover(p) + unit):
            pairs.append((rep.tobytes(), rep[:tl - cut].tobytes()))
            pairs.append((rep[:tl - cut].tobytes(), rep.tobytes()))
            half = tl // 2
            pairs.append((rep.tobytes(), np.concatenate([rep[:half], rep[half + cut:]]).tobytes()))
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("block,chunk_k", [(512, 8), (64, 2)])
@pytest.mark.parametrize("tag", sorted(PEN))
def test_gap_runs_across_chunk_edges(oracle, tag, block, chunk_k, capfd, monkeypatch):
    """Where a wrong age index of a register history or of the edge table gives the right score with a wrong CIGAR or n_iter."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = hazard_pairs(tag, chunk_k)
    kw = dict(flag=1, **PEN[tag])
    exp = _expected(oracle, ("hazard", tag, chunk_k), pairs, kw)
    capfd.readouterr()
    got = F.run_engine(PackedBatch(pairs), kw, [("force_kind", 2), ("block", block), ("band_pack", 1)])
    kinds, bands = _launch_lines(capfd.readouterr().err)
    # the first launch is the forced geometry's instantiation for this set, with traceback, on 2-bit copies, and holds every pair
    assert kinds and kinds[0][0] == 2 and bands and bands[0] == (block, 3, PEN[tag]["e1"], PEN[tag]["e2"], 1, 1, 0, 0, len(pairs)), (kinds[:2], bands[:2])
    _check(got, exp, f"hazards {tag} block {block}", pairs)
    # most pairs are the geometry's own: what it may hand back is bounded by the oracle's band trace
    bound = dm.not_fit_count(oracle, pairs, PEN[tag], block)
    assert bound < len(pairs) // 2 and got[3].n_retries <= bound, (got[3].n_retries, bound)


# ---- forced-geometry fuzz ---------------------------------------------------------------------------------------------------------------------
_fuzz_set: list = []


def fuzz_set():
    if not _fuzz_set:
        from miniwfa_amd.synth import fuzz_pairs, skewed_pairs, random_seq
        seed = 23
        a = random_seq(seed + 10, 2500)
        _fuzz_set.extend(fuzz_pairs(seed, 28, 3000) + skewed_pairs(seed, 9, 200, 3000))
        _fuzz_set.extend([(a, a), (random_seq(seed + 13, 300), random_seq(seed + 13, 300)), (b"", b""), (b"", a[:700]), (a[:900], b""), (b"A", b"C"),
                          (a, a[:300]), (a[2000:], a),                                         # one sequence a piece of the other
                          (random_seq(seed + 11, 2600), random_seq(seed + 12, 1900))])         # unrelated: both corners of the matrix
    return _fuzz_set


FUZZ_MODES = (dict(flag=0), dict(flag=1), dict(flag=0, max_s=150), dict(flag=1, max_iter=20000), dict(flag=1, step=5000))


@pytest.mark.gpu
@pytest.mark.parametrize("block", [64, 128, 256, 512, 768, 1024])
@pytest.mark.parametrize("tag", sorted(PEN))
def test_forced_geometry_fuzz(oracle, tag, block):
    """Every set on every geometry (block 1024: band_span 2, the span geometry takes every pair it can): score, CIGAR, the max_s / max_iter stop rules and
    step = 5000 (a pair whose worst-case penalty stays below the step is served as high-memory — under default routing by the classes, i.e. block 1024
    here; the rest, and under a forced geometry every pair, is the generic kernel's low-memory pass), against the oracle; in every mode the re-runs are
    bounded by the pairs the geometry may hand back."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch
    pairs = fuzz_set()
    pk = PackedBatch(pairs)
    tun = [("band_span", 2)] if block == 1024 else [("force_kind", 2), ("block", block), ("band_pack", 1)]
    bound = dm.not_fit_count(oracle, pairs, PEN[tag], block)
    for mode in FUZZ_MODES:
        kw = dict(**PEN[tag], **mode)
        exp = _expected(oracle, "fuzz", pairs, kw)
        got = F.run_engine(pk, kw, tun)
        _check(got, exp, f"fuzz {tag} block {block} {mode}", pairs)
        assert got[3].n_retries <= bound, (tag, block, mode, got[3].n_retries, bound)


# ---- default routing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(PEN))
def test_default_routing_10kb_batch(oracle, tag, capfd, monkeypatch):
    """64 x 10 kb @ 5 %: the packed band kernel (kernel_kind 2, packed 1), instantiated for this set's extensions; oracle-equal, and the first pair is the
    compiled reference's 10 kb vector."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    gold = {v["id"]: v for v in load_golden("band_pen.jsonl")}
    pairs = [golden_inputs(gold[f"band10k-{tag}-cigar"])] + [synth_pair(720000 + i, 10000, 0.05) for i in range(63)]
    pk = PackedBatch(pairs)
    exp = _expected(oracle, "route10k", pairs, dict(flag=1, **PEN[tag]))
    for flag in (0, 1):
        capfd.readouterr()
        got = F.run_engine(pk, dict(flag=flag, **PEN[tag]))
        kinds, bands = _launch_lines(capfd.readouterr().err)
        st = got[3]
        assert st.kernel_kind == 2 and st.packed == 1, (tag, flag, st.kernel_kind, st.packed)
        assert bands and all(b[2:4] == (PEN[tag]["e1"], PEN[tag]["e2"]) and b[7] == 0 for b in bands), bands
        assert kinds and kinds[0][0] == 2 and bands[0][8] == len(pairs), (kinds, bands)
        _check(got, exp, f"10 kb {tag} flag {flag}", pairs)
        e = gold[f"band10k-{tag}-{'cigar' if flag else 'score'}"]["expect"]
        assert (int(got[0][0]), int(got[1][0])) == (e["s"], e["n_iter"])
        if flag:
            assert cigar_matches(got[2][0], e)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["e31", "e41"])
def test_default_routing_mixed_batch(oracle, tag, capfd, monkeypatch):
    """Lengths 150 ... 20 000 in one batch: oracle-equal, and the 512-thread class starts on the band kernel, not on the generic one."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    lens = [150, 220, 400, 900, 1500, 2500, 4000, 6000, 9000, 12000, 20000]
    pairs = [synth_pair(730000 + i, lens[i % len(lens)], (0.02, 0.05)[i % 2]) for i in range(66)]
    exp = _expected(oracle, "mixed", pairs, dict(flag=1, **PEN[tag]))
    for flag in (0, 1):
        capfd.readouterr()
        got = F.run_engine(PackedBatch(pairs), dict(flag=flag, **PEN[tag]))
        kinds, bands = _launch_lines(capfd.readouterr().err)
        _check(got, exp, f"mixed {tag} flag {flag}", pairs)
        first = next((k for k in kinds if k[0] == 0 or (k[0] == 2 and k[1] == 512)), None)
        assert first is not None and first[0] == 2, kinds
        assert any(b[0] == 512 and b[2:4] == (PEN[tag]["e1"], PEN[tag]["e2"]) for b in bands), bands


@pytest.mark.gpu
def test_default_routing_span_geometry(oracle, capfd, monkeypatch):
    """40 x 30 kb @ 3 % under e31 with band_span 2: the span geometry (1024 x 5) takes the batch; oracle-equal."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(740000 + i, 30000, 0.03) for i in range(40)]
    exp = _expected(oracle, "span30k", pairs, dict(flag=1, **PEN["e31"]))
    for flag in (0, 1):
        capfd.readouterr()
        got = F.run_engine(PackedBatch(pairs), dict(flag=flag, **PEN["e31"]), [("band_span", 2)])
        kinds, bands = _launch_lines(capfd.readouterr().err)
        assert bands and bands[0][:4] == (1024, 5, 3, 1) and bands[0][8] == len(pairs), (kinds, bands)
        _check(got, exp, f"span e31 flag {flag}", pairs)


# ---- chain mode -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_and_auto_batches_match_the_compiled_reference():
    """mwf_wfa_chain_batch / mwf_wfa_auto_batch under (4,6,3,26,1) — their gap fills are a batch of short and mid-size pairs — against what the compiled
    reference returned for each record (tests/golden/band_pen.jsonl), and against the per-call mwf_wfa_chain / mwf_wfa_auto."""
    import miniwfa_amd as mw
    vec = load_golden("band_pen.jsonl")
    keys = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter", "max_occ", "kmer", "min_len")
    for entry, batch_fn, one_fn in (("chain", mw.wfa_chain_batch, mw.wfa_chain), ("auto", mw.wfa_auto_batch, mw.wfa_auto)):
        vs = [v for v in vec if v["entry"] == entry]
        assert len(vs) == 7
        pairs = [golden_inputs(v) for v in vs]
        o = mw.opt_init(**{k: vs[0]["opt"][k] for k in keys})
        out = batch_fn(pairs, o)
        for v, (t, q), (s, n_iter, cig) in zip(vs, pairs, out):
            e = v["expect"]
            assert s == e["s"] and (e["n_iter"] is None or n_iter == e["n_iter"]), (v["id"], s, e["s"])
            assert cigar_matches(cig, e), v["id"]
            s1, it1, cig1 = one_fn(t, q, o)
            assert s1 == s and (e["n_iter"] is None or it1 == n_iter) and list(cig1) == list(cig), v["id"]


# ---- guard rails ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pen", [dict(x=3, o1=5, e1=3, o2=20, e2=3), dict(x=4, o1=6, e1=5, o2=30, e2=1), dm.NOT_BUILT_PEN["e42"]], ids=["e33", "e51", "e42"])
def test_other_extensions_launch_no_band_kernel(oracle, pen, capfd, monkeypatch):
    """(3,3), (5,1) — and (4,2), which missed its speed gate — keep the lane / mid / generic kernels: a 512 x 2 kb batch launches no band kernel."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    from oracle.pyoracle import make_opt
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(750000 + i, 2000, 0.05) for i in range(512)]
    capfd.readouterr()
    got = F.run_engine(PackedBatch(pairs), dict(flag=1, **pen))
    kinds, bands = _launch_lines(capfd.readouterr().err)
    assert kinds and not bands, bands[:2]
    for i in range(0, 512, 61):
        es, eit, ecig = oracle.align(pairs[i][0], pairs[i][1], make_opt(flag=1, **pen))
        assert (int(got[0][i]), int(got[1][i])) == (es, eit) and got[2][i] == (ecig or []), i


@pytest.mark.gpu
@pytest.mark.parametrize("seq2bit", [1, 0])
def test_bases_outside_acgt_take_the_byte_wise_copy(oracle, seq2bit, capfd, monkeypatch):
    """Pairs with N / lower-case bases under e31, in a batch too big for the mid kernel (more pairs than the device has CUs): the 768 x 2 byte-wise copy for
    (3,1), no error, oracle-equal."""
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = []
    for i in range(320):
        t, q = synth_pair(760000 + i, 1800 + 40 * (i % 7), 0.05)
        if i % 3 == 0:
            t = t[:100] + b"N" + t[101:]
            q = q[:50] + b"n" + q[51:300] + b"acgt" + q[304:]
        pairs.append((t, q))
    exp = _expected(oracle, "nonacgt", pairs, dict(flag=1, **PEN["e31"]))
    capfd.readouterr()
    got = F.run_engine(PackedBatch(pairs), dict(flag=1, **PEN["e31"]), [("seq2bit", seq2bit)])
    kinds, bands = _launch_lines(capfd.readouterr().err)
    _check(got, exp, f"non-ACGT seq2bit {seq2bit}", pairs)
    assert any(b[:4] == (768, 2, 3, 1) and b[5] == 0 for b in bands), bands


@pytest.mark.gpu
def test_band_pack_0_keeps_the_new_sets_off_the_band_kernel(oracle, capfd, monkeypatch):
    import fuzzlib as F
    from miniwfa_amd.synth import PackedBatch, synth_pair
    monkeypatch.setenv("MWF_DEBUG", "1")
    pairs = [synth_pair(770500 + i, 3000, 0.05) for i in range(64)]
    exp = _expected(oracle, "pack0", pairs, dict(flag=1, **PEN["e31"]))
    capfd.readouterr()
    got = F.run_engine(PackedBatch(pairs), dict(flag=1, **PEN["e31"]), [("band_pack", 0)])
    kinds, bands = _launch_lines(capfd.readouterr().err)
    assert kinds and not bands, bands[:2]
    _check(got, exp, "band_pack 0", pairs)
