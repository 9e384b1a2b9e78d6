"""The whole-device kernel (mwf_sys.hip / mwf_sys_deep.hip) under gap extensions of 3 and 4 — (e1, e2) in {3, 4} x {1, 2}, minimap2's asm5-like
sets among them.  The reference has one loop for any x, o1, e1, o2, e2 (miniwfa.c:243-259, :390-393); before these instantiations a long pair
under such penalties fell to the one-workgroup-per-pair generic kernel (stats.kernel_kind 0).

Anchors: tests/golden/long_pairs_pen.jsonl — the 150 kb and 5 Mb pairs of long_pairs.jsonl and a 100 kb chain-mode pair, run through the
COMPILED reference by tests/golden/make_golden_long_pen.py — and the oracle's restatement for everything small enough to recompute.
s, n_iter, n_cigar and the CIGAR (through its SHA-256 where it is long) are compared for equality: integer work, no tolerance."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, golden_inputs

VEC = load_golden("long_pairs_pen.jsonl")
C4 = [v for v in VEC if v["id"].startswith("c4-")]
OPT_KEYS = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter")
# one penalty set per new pair of gap extensions (the sets of the golden vectors)
PEN = {"e31": dict(x=4, o1=6, e1=3, o2=26, e2=1), "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2),
       "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1), "e42": dict(x=2, o1=4, e1=4, o2=24, e2=2)}


def _sha(words) -> str:
    return hashlib.sha256(np.asarray(words, dtype="<u4").tobytes()).hexdigest()


def _vec(vid):
    return next(v for v in VEC if v["id"] == vid)


def _check_answer(got, exp, what):
    s, n_iter, cig = got
    assert (s, n_iter) == (exp["s"], exp["n_iter"]), what
    assert (None if cig is None else len(cig)) == exp["n_cigar"], what
    if cig is not None:
        assert _sha(cig) == exp["cigar_sha256"], what


# ---- CPU: the fixtures ---------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_every_new_set_and_mode():
    ids = {v["id"] for v in VEC}
    assert {f"c4-{p}-{m}" for p in PEN for m in ("score", "cigar", "lowmem", "lowmem1000")} <= ids
    assert {"mhc-e31-score", "mhc-e31-lowmem", "chain-e31-cigar", "chain-e31-score", "auto-e31-cigar"} <= ids
    for v in VEC:
        if v["entry"] != "exact":
            continue
        tag = v["id"].split("-")[1]
        assert {k: v["opt"][k] for k in ("x", "o1", "e1", "o2", "e2")} == PEN[tag], v["id"]
        assert v["tl"] == (150000 if v["id"].startswith("c4-") else 5000000)
        if v["opt"]["step"] > 0:   # a low-memory vector that takes no snapshot would test the high-memory path twice
            assert v["opt"]["flag"] == 1 and v["expect"]["s"] >= v["opt"]["step"], v["id"]


@pytest.mark.parametrize("vid", [v["id"] for v in C4])
def test_oracle_matches_reference_on_the_150kb_pair(oracle, vid):
    """CPU: the restatement reproduces the compiled reference on every 150 kb vector (seconds each; the 5 Mb vectors take minutes of one core and are
    checked on the GPU side only)."""
    from oracle.pyoracle import make_opt
    v = _vec(vid)
    t, q = golden_inputs(v)
    _check_answer(oracle.align(t, q, make_opt(**v["opt"])), v["expect"], vid)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _engine_run(pairs, opt_kw, tunables=()):
    """One align on a fresh engine: ([(s, n_iter, cigar words | None)], stats)."""
    import miniwfa_amd as mw
    from miniwfa_amd.synth import PackedBatch
    eng = mw.Engine(0)
    try:
        for k, val in tunables:
            eng.set(k, val)
        o = mw.opt_init(**opt_kw)
        b = eng.upload(PackedBatch(pairs))
        b.align(o)
        s, it, nc = b.results()
        out = [(int(s[i]), int(it[i]), b.cigar(i, int(nc[i])).tolist() if (o.flag & 1) else None) for i in range(len(pairs))]
        st = eng.stats()
        b.free()
        return out, st
    finally:
        eng.close()


def _same(got, exp, cigar=True):
    """(s, n_iter[, CIGAR]) of an engine run equal the oracle's."""
    return (got[0], got[1]) == (exp[0], exp[1]) and (not cigar or list(got[2]) == list(exp[2] or []))


_default_two_pass = {}


def _two_pass_of_default_set(t, q, flag, step):
    """stats.lowmem_two_pass of the same pair and mode under the default penalties (which form of the low-memory mode the plan takes depends on
    lengths and budget, not on the penalties)."""
    key = (len(t), len(q), flag, step)
    if key not in _default_two_pass:
        _, st = _engine_run([(t, q)], dict(flag=flag, step=step))
        assert st.kernel_kind == 1
        _default_two_pass[key] = st.lowmem_two_pass
    return _default_two_pass[key]


@pytest.mark.gpu
@pytest.mark.parametrize("vid", [v["id"] for v in C4])
def test_150kb_pair_runs_on_the_whole_device_kernel_and_matches_reference(vid):
    """Default routing: a 150 kb pair under each new set, score / CIGAR / low-memory with steps 5000 and 1000, is the whole-device kernel's, runs once,
    takes the same form of the low-memory mode as under the default set, and returns the reference's answer — through the engine and through mwf_wfa_exact."""
    import miniwfa_amd as mw
    v = _vec(vid)
    t, q = golden_inputs(v)
    kw = {k: v["opt"][k] for k in OPT_KEYS}
    out, st = _engine_run([(t, q)], kw)
    print(f"{vid}: kernel_kind {st.kernel_kind} kernel_ms {st.kernel_ms:.2f} launches {st.n_launches} re-runs {st.n_retries} two_pass {st.lowmem_two_pass}")
    _check_answer(out[0], v["expect"], vid)
    assert st.kernel_kind == 1 and st.n_retries == 0, (vid, st.kernel_kind, st.n_retries)
    assert st.lowmem_two_pass == _two_pass_of_default_set(t, q, kw["flag"], kw["step"]), vid
    o = mw.opt_init(**kw)
    s, n_iter, cig = mw.wfa_exact(t, q, o)
    _check_answer((s, n_iter, None if cig is None else list(cig)), v["expect"], vid + " (mwf_wfa_exact)")
    if cig is not None:
        assert mw.cigar2score(o, cig) == (s, len(t), len(q))


def _n_slices(o):
    """Array-slices of a low-memory snapshot: the H ring and the E/F histories (reference wf_snapshot1, miniwfa.c:451-474)."""
    return max(o["x"], o["o1"] + o["e1"], o["o2"] + o["e2"]) + 1 + 2 * o["e1"] + 2 * o["e2"]


@pytest.mark.gpu
def test_5mb_pair_matches_reference_score_and_low_memory():
    """The MHC-like 5 Mb pair under the asm5-like set (4,6,3,26,1): score-only, and with step = 5000 in the reference's two-pass form on the whole-device
    kernel (provenance pass wfa_sys_seg_kernel<3,1,...>, snapshot trace, second pass).

    Memory bound: the default set's contract is 8 GB (tests/test_long_pairs.py).  Two parts of the footprint grow with the penalties, everything else (the
    second pass's traceback of s_guess x 2 (step + 2 nH) bytes, sequences, logs) is as under the default set:
      * the snapshot arena: nH + 2 e1 + 2 e2 array-slices (36 here, 23 by default) of the window at each of the s / step snapshots; the window after S
        penalties is at most 2 S + 1 columns wide (one column per side and penalty), so at most slices x sum_j (2 j step + 1) ints, with the reference's
        own s of both runs (long_pairs_pen.jsonl, long_pairs.jsonl);
      * the H ring and its provenance ring: nH rows of 256 ints per chunk slot, sixteen slots per workgroup.
    Bound = 8 GB + the growth of these two over the default set (about 9.5 GB)."""
    vs, vl = _vec("mhc-e31-score"), _vec("mhc-e31-lowmem")
    t, q = golden_inputs(vs)
    out, st = _engine_run([(t, q)], {k: vs["opt"][k] for k in OPT_KEYS})
    print(f"mhc-e31-score: kernel_kind {st.kernel_kind} kernel_ms {st.kernel_ms:.1f} re-runs {st.n_retries} dev_bytes_peak {st.dev_bytes_peak}")
    _check_answer(out[0], vs["expect"], "mhc-e31-score")
    assert st.kernel_kind == 1
    out, st = _engine_run([(t, q)], {k: vl["opt"][k] for k in OPT_KEYS})
    default = next(v for v in load_golden("long_pairs.jsonl") if v["id"] == "mhc-lowmem")

    def snap_ints(v):
        step = vl["opt"]["step"]
        return _n_slices(v["opt"]) * sum(2 * j * step + 1 for j in range(1, v["expect"]["s"] // step + 1))

    def n_h(o):
        return max(o["x"], o["o1"] + o["e1"], o["o2"] + o["e2"]) + 1
    rings = 2 * (st.grid * 16) * 256 * 4 * (n_h(vl["opt"]) - n_h(default["opt"]))
    bound = 8e9 + 4 * (snap_ints(vl) - snap_ints(default)) + rings
    print(f"mhc-e31-lowmem: kernel_kind {st.kernel_kind} two_pass {st.lowmem_two_pass} kernel_ms {st.kernel_ms:.1f} re-runs {st.n_retries} "
          f"dev_bytes_peak {st.dev_bytes_peak} bound {bound:.3e}")
    _check_answer(out[0], vl["expect"], "mhc-e31-lowmem")
    assert st.kernel_kind == 1 and st.lowmem_two_pass == 1
    assert st.dev_bytes_peak <= bound, (st.dev_bytes_peak, bound)


def _fuzz_set(seed):
    """Small and mid pairs for the forced whole-device kernel: the band kernels' corner cases (miniwfa_amd.synth.fuzz_pairs: granularity lengths,
    homopolymers, tandem repeats, every seventh unrelated), length-skewed pairs whose window moves, unrelated, identical and empty sequences."""
    from miniwfa_amd.synth import fuzz_pairs, skewed_pairs, synth_pair, random_seq
    pairs = fuzz_pairs(seed, 28, 3000) + skewed_pairs(seed + 3, 9, 200, 3000)
    a = random_seq(seed + 10, 2500)
    pairs += [(random_seq(seed + 11, 5200), random_seq(seed + 12, 3900)),           # unrelated, both corners of the matrix
              (a, a), (random_seq(seed + 13, 300), random_seq(seed + 13, 300)),     # identical: the origin's extension is the alignment
              (b"", b""), (b"", a[:700]), (a[:900], b""), (b"A", b"C"),             # empty sequences
              (a, a[:300]), (a[2000:], a),                                          # one sequence a piece of the other
              synth_pair(seed + 20, 6000, 0.04), synth_pair(seed + 21, 9000, 0.1, 2, 500)]
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(PEN))
def test_forced_whole_device_kernel_fuzz_against_oracle(oracle, tag):
    """force_kind 1 on every run, so that nothing can be routed away or skipped: each new set x one and four columns per lane x score / CIGAR /
    low-memory (step = 97: a snapshot in almost every pair) and the max_s / max_iter stop rules, against the oracle."""
    import fuzzlib as F
    from oracle.pyoracle import make_opt
    pairs = _fuzz_set(11)
    bad = []
    modes = (dict(flag=0), dict(flag=1), dict(flag=1, step=97), dict(flag=0, max_s=150), dict(flag=1, max_iter=20000))
    for mode in modes:
        kw = dict(**PEN[tag], **mode)
        exp = F.oracle_many(oracle, pairs, make_opt(**kw))
        for c in (1, 4):
            out, st = _engine_run(pairs, kw, [("force_kind", 1), ("sys_c", c)])
            assert st.kernel_kind == 1
            for i, (got, e) in enumerate(zip(out, exp)):
                es, eit, ecig = e
                if (got[0], got[1]) != (es, eit) or (got[2] is not None and es >= 0 and got[2] != (ecig or [])):
                    bad.append((tag, mode, c, i, len(pairs[i][0]), len(pairs[i][1]), got[:2], (es, eit)))
    assert not bad, bad[:8]


def _two_pass_set(seed):
    """Pairs for the forced two-pass low-memory mode: mid-size pairs past several band shrinks, long indels, length-skewed and unrelated pairs,
    identical and empty sequences — fourteen, so that a batch runs side by side (run_coop_group) and the first of them alone (run_coop_pair)."""
    from miniwfa_amd.synth import skewed_pairs, synth_pair, random_seq
    a = random_seq(seed + 10, 2500)
    return [synth_pair(seed, 20000, 0.04), synth_pair(seed + 1, 30000, 0.03, 1, 4000), synth_pair(seed + 2, 9000, 0.2), synth_pair(seed + 3, 15000, 0.01, 3, 2000),
            synth_pair(seed + 4, 3000, 0.05), synth_pair(seed + 5, 300, 0.1), (random_seq(seed + 11, 5200), random_seq(seed + 12, 3900)),
            (a, a), (b"", a[:700]), (a[:900], b""), (a[2000:], a), (b"A" * 1200, b"C" * 1100)] + skewed_pairs(seed + 6, 2, 2000, 8000)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("tag", sorted(PEN))
def test_forced_two_pass_low_memory_mode_against_oracle(oracle, tag, c):
    """The provenance pass (wfa_sys_seg_kernel<E1,E2,8,false,C>), the snapshots' flat indices, sys_trace_kernel's decoding of E/F ages, the parked
    provenance registers and the shadow halves of the hand-off boxes, for every new set at one and four columns per lane: a 1 MB budget for the walk
    variant forces the two-pass form (as tests/test_gpu_parity.py::test_whole_device_kernel_true_low_memory_mode does for the default set).  Fourteen
    pairs side by side and one pair alone; steps from 7 (a snapshot every few penalties) to 5000 (beyond most pairs' penalty)."""
    import fuzzlib as F
    from oracle.pyoracle import make_opt
    cases = _two_pass_set(31)
    tun = [("force_kind", 1), ("sys_c", c), ("lowmem_budget_mb", 1)]
    bad = []
    for step in (7, 97, 700, 5000):
        pairs = [p for p in cases if len(p[0]) <= 9000] if step < 10 else cases   # (a snapshot every seven penalties: keep it to seconds)
        kw = dict(flag=1, step=step, **PEN[tag])
        exp = F.oracle_many(oracle, pairs, make_opt(**kw))
        for sub, e in ((pairs, exp), (pairs[:1], exp[:1])):
            out, st = _engine_run(sub, kw, tun)
            assert st.kernel_kind == 1 and st.lowmem_two_pass == 1, (tag, c, step, st.kernel_kind, st.lowmem_two_pass)
            for i, (got, ee) in enumerate(zip(out, e)):
                if not _same(got, ee):
                    bad.append((tag, c, step, len(sub), i, len(sub[i][0]), len(sub[i][1]), got[:2], tuple(ee[:2])))
    assert not bad, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["e31", "e42"])
@pytest.mark.parametrize("p", [0.03, 0.08])
def test_pairs_side_by_side_against_oracle(oracle, tag, p):
    """12 x 25 kb under default routing: pairs side by side on groups of workgroups (run_coop_group), score-only and with CIGAR."""
    import fuzzlib as F
    from miniwfa_amd.synth import synth_pair
    from oracle.pyoracle import make_opt
    pairs = [synth_pair(640000 + int(p * 1000) * 100 + i, 25000, p) for i in range(12)]
    exp = F.oracle_many(oracle, pairs, make_opt(flag=1, **PEN[tag]))
    for flag in (0, 1):
        out, st = _engine_run(pairs, dict(flag=flag, **PEN[tag]))
        print(f"12 x 25 kb @ {p} {tag} flag {flag}: kernel_kind {st.kernel_kind} kernel_ms {st.kernel_ms:.2f} grid {st.grid} re-runs {st.n_retries}")
        assert st.kernel_kind == 1, (tag, p, flag)
        for i, (got, e) in enumerate(zip(out, exp)):
            assert got[:2] == e[:2], (tag, p, flag, i)
            if flag:
                assert got[2] == e[2], (tag, p, flag, i)


@pytest.mark.gpu
def test_chain_and_auto_with_a_long_gap_fill_match_the_compiled_reference(oracle):
    """mwf_wfa_chain / mwf_wfa_auto under (4,6,3,26,1) on a 100 kb pair whose middle is one gap fill of 9500 x 9800 unrelated bases (just below the 10 kb
    from which the reference bridges instead of aligning, miniwfa.c:869), against what the compiled reference returned (long_pairs_pen.jsonl).  That gap
    fill is a single pair of 19.3 kb with CIGAR: under default routing the whole-device kernel's — checked on the blocks themselves."""
    import miniwfa_amd as mw
    from miniwfa_amd.synth import synth_diverged_block, random_seq
    from oracle.pyoracle import make_opt
    keys = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter", "max_occ", "kmer", "min_len")
    for vid in ("chain-e31-cigar", "chain-e31-score", "auto-e31-cigar"):
        v = _vec(vid)
        t, q = synth_diverged_block(*v["args"])
        assert (len(t), len(q)) == (v["tl"], v["ql"])
        o = mw.opt_init(**{k: v["opt"][k] for k in keys})
        s, n_iter, cig = (mw.wfa_chain if v["entry"] == "chain" else mw.wfa_auto)(t, q, o)
        exp = v["expect"]
        assert s == exp["s"], vid
        if exp["n_iter"] is not None:
            assert n_iter == exp["n_iter"], vid
        assert (None if cig is None else len(cig)) == exp["n_cigar"], vid
        if cig is not None:
            assert _sha(cig) == exp["cigar_sha256"], vid
    seed, _, block_t, block_q, _ = _vec("chain-e31-cigar")["args"]
    gap = (random_seq(seed + 2, block_t), random_seq(seed + 3, block_q))
    out, st = _engine_run([gap], dict(flag=1, **PEN["e31"]))
    assert st.kernel_kind == 1
    assert _same(out[0], oracle.align(gap[0], gap[1], make_opt(flag=1, **PEN["e31"])))


@pytest.mark.gpu
def test_other_extensions_and_big_batches_keep_their_kernels(oracle):
    """Guard rails: gap extensions the kernel is not built for — (3,3), (5,1) — keep the generic kernel under default routing and the refusal under
    force_kind 1; a big batch of short pairs under a new set is never the whole-device kernel's."""
    import miniwfa_amd as mw
    from miniwfa_amd.synth import PackedBatch, synth_pair
    from oracle.pyoracle import make_opt
    pair = synth_pair(650001, 40000, 0.03)
    for pen in (dict(x=3, o1=5, e1=3, o2=20, e2=3), dict(x=4, o1=6, e1=5, o2=30, e2=1)):
        out, st = _engine_run([pair], dict(flag=1, **pen))
        assert st.kernel_kind == 0, pen
        assert _same(out[0], oracle.align(pair[0], pair[1], make_opt(flag=1, **pen))), pen
    eng = mw.Engine(0)
    try:
        eng.set("force_kind", 1)
        b = eng.upload(PackedBatch([pair]))
        with pytest.raises(RuntimeError, match="does not support these penalties"):
            b.align(mw.opt_init(x=3, o1=5, e1=3, o2=20, e2=3))
        b.free()
    finally:
        eng.close()
    pairs = [synth_pair(660000 + i, 2000, 0.05) for i in range(1024)]
    for flag in (0, 1):
        out, st = _engine_run(pairs, dict(flag=flag, **PEN["e31"]))
        assert st.kernel_kind != 1, flag
        for i in range(0, 1024, 97):
            assert _same(out[i], oracle.align(pairs[i][0], pairs[i][1], make_opt(flag=1, **PEN["e31"])), cigar=bool(flag)), (flag, i)
