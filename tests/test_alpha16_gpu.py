"""GPU tests of the "alpha16" tunable (include/miniwfa.h; kernels csrc/mwf_alphabet.hip and csrc/mwf_band2_nib.hip): together with "alpha_remap" 1, a pair of 5 to 16
distinct bytes is class 3, is copied into the batch's arena as 0x40 | code and — under gap extensions (2,1) — runs on the packed band kernel's 4-bit form.  Inputs:
tests/alpha16_cases.py; tests/test_alpha16_cpu.py checks from the oracle alone that every case is what it is chosen for.  Expected answers: the oracle on the original bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
from oracle.pyoracle import make_opt
import alpha16_cases as c16

pytestmark = pytest.mark.gpu

ROUTE = ("kernel_kind", "packed", "block", "grid", "n_retries")
_cache = {}


def engine(alpha16=1, remap=1, tun=()):
    eng = mw.Engine(0)
    for name, v in tun:
        eng.set(name, v)
    eng.set("alpha_remap", remap)
    eng.set("alpha16", alpha16)
    return eng


def check_answers(b, exp, label, cigar=True):
    s, it, nc = b.results()
    for i, (es, eit, ecig) in enumerate(exp):
        assert (int(s[i]), int(it[i])) == (es, eit), (label, i)
        if cigar and ecig is not None:
            assert b.cigar(i, int(nc[i])).tolist() == ecig, (label, i)


def route(eng):
    st = eng.stats()
    return {k: getattr(st, k) for k in ROUTE}


def host_classes(pk):
    return [mw.alphabet_class16(*pk.pair(i))[0] for i in range(pk.n)]


def routing_batches():
    """(64 x 3 kb at 5 %, 4 x 16 kb at 3 %), one run of ten N in every target and three N in every query."""
    if "routing" not in _cache:
        _cache["routing"] = (c16.routing_pairs(64, 3000, 0.05, 71000), c16.routing_pairs(4, 16000, 0.03, 72000))
    return _cache["routing"]


# ---- (a) classes and answers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pen", ["default", "a22"])
@pytest.mark.parametrize("flag", [0, 1])
def test_classes_and_answers(oracle, pen, flag):
    """One uploaded batch of 42 pairs: alphabets of 4 (lower case), 5 (ACGTN), 6 with bytes 0x00 and 0xff, 8 (mixed case), 16 and 17 symbols at lengths 1 ... 6500, empty
    sequences, sequences at odd byte offsets, three queries on one target range.  Batch.alphabet() equals the host twin's classes; (s, n_iter, CIGAR) equal the oracle's on
    the original bytes; a second align replays the copies without raising dev_bytes_peak."""
    pk, names = c16.gpu_batch_a()
    pairs = [pk.pair(i) for i in range(pk.n)]
    kw = {} if pen == "default" else dict(o2=4, e2=2)
    exp = c16.expected(oracle, "a", pairs, flag=flag, **kw)
    eng = engine()
    b = eng.upload(pk)
    b.align(mw.opt_init(flag=flag, **kw))
    check_answers(b, exp, (pen, flag))
    cls = b.alphabet().tolist()
    assert cls == host_classes(pk), [(n, c) for n, c in zip(names, cls)]
    assert {0, 1, 2, 3} <= set(cls)
    peak = eng.stats().dev_bytes_peak
    b.align(mw.opt_init(flag=flag, **kw))
    check_answers(b, exp, (pen, flag, "again"))
    assert eng.stats().dev_bytes_peak == peak
    b.free()
    eng.close()


# ---- (b) the same through a wrapped batch, once per workgroup size of the classify / copy kernels -------------------------------------------------------------
@pytest.mark.parametrize("which", ["short", "a", "long"])
def test_wrapped_classes_and_answers(oracle, which):
    """"short": pairs of up to 900 bases, 64 threads; "a": batch (a), 256 threads; "long": three pairs of 34 kb, 1024 threads.  Each holds a class-3 pair, a class-2
    pair and a fifth symbol in the last byte of a query."""
    import torch
    pk, names = {"short": c16.gpu_batch_short, "a": c16.gpu_batch_a, "long": c16.gpu_batch_long}[which]()
    pairs = [pk.pair(i) for i in range(pk.n)]
    want = host_classes(pk)
    assert {2, 3} <= set(want) and any(n.startswith("n_last_q") for n in names)
    exp = c16.expected(oracle, which, pairs)
    eng = engine()
    b = eng.wrap_packed(pk, torch.device("cuda", 0))
    b.align(mw.opt_init(flag=1))
    check_answers(b, exp, ("wrapped", which))
    cls = b.alphabet().tolist()
    assert cls == want, [(n, c, w) for n, c, w in zip(names, cls, want) if c != w]
    b.free()
    eng.close()


# ---- (c) routing: fails without the feature (set("alpha16", ...) is an error there) -----------------------------------------------------------------------
def _run(pairs, alpha16, tun=(), flag=0, **pen):
    eng = engine(alpha16=alpha16, tun=tun)
    b = eng.upload(PackedBatch(pairs))
    b.align(mw.opt_init(flag=flag, **pen))
    res = b.results()
    r = route(eng)
    b.free()
    eng.close()
    return r, res


def test_routing_mid_size_pairs_take_the_4bit_512_geometry(oracle, capsys):
    """64 x 3 kb at 5 % with N in every pair, "mid_max_pairs" 0.  alpha16 1: the packed band kernel (kind 2, packed 1) on 512 threads — with 0: 768 — and no more re-runs
    than with 0 (block 768 holds the same 24 chunks).  Answers: the oracle's."""
    small, _ = routing_batches()
    exp = c16.expected(oracle, "small", small, flag=0)
    r1, res1 = _run(small, 1, tun=(("mid_max_pairs", 0),))
    r0, res0 = _run(small, 0, tun=(("mid_max_pairs", 0),))
    with capsys.disabled():
        print(f"\n   64 x 3 kb with N: alpha16 1 {r1}  alpha16 0 {r0}")
    for res in (res1, res0):
        assert [(int(s), int(it)) for s, it in zip(res[0], res[1])] == [(s, it) for s, it, _ in exp]
    assert (r1["kernel_kind"], r1["packed"], r1["block"]) == (2, 1, 512), r1
    assert r1["n_retries"] <= r0["n_retries"], (r1, r0)
    assert (r0["kernel_kind"], r0["packed"], r0["block"]) == (2, 1, 768), r0


def test_routing_long_pairs_take_the_4bit_span_geometry(oracle, capsys):
    """4 x 16 kb at 3 % with N, "coop_min_len" beyond them.  alpha16 1: kind 2 on 1024 threads; 0: the generic kernel."""
    _, long_ = routing_batches()
    exp = c16.expected(oracle, "long", long_, flag=0)
    r1, res1 = _run(long_, 1, tun=(("coop_min_len", 1 << 30),))
    r0, res0 = _run(long_, 0, tun=(("coop_min_len", 1 << 30),))
    with capsys.disabled():
        print(f"\n   4 x 16 kb with N: alpha16 1 {r1}  alpha16 0 {r0}")
    for res in (res1, res0):
        assert [(int(s), int(it)) for s, it in zip(res[0], res[1])] == [(s, it) for s, it, _ in exp]
    assert (r1["kernel_kind"], r1["packed"], r1["block"]) == (2, 1, 1024), r1
    assert r0["kernel_kind"] == 0, r0


def test_routing_other_penalties_stay_byte_wise(oracle):
    """The 64 x 3 kb batch under (2,2) with alpha16 1: block 768, as without it, and the oracle's answers (the byte-wise kernel compares the image bytes)."""
    small, _ = routing_batches()
    exp = c16.expected(oracle, "small", small, flag=0, o2=4, e2=2)
    r1, res1 = _run(small, 1, tun=(("mid_max_pairs", 0),), o2=4, e2=2)
    assert [(int(s), int(it)) for s, it in zip(res1[0], res1[1])] == [(s, it) for s, it, _ in exp]
    assert (r1["kernel_kind"], r1["packed"], r1["block"]) == (2, 1, 768), r1


def test_512_thread_4bit_kernels_keep_two_workgroups_per_cu(capfd, monkeypatch):
    """The 64 x 3 kb batch on three and on four slots, score-only and with CIGAR: the launch is wfa_band2_nib_kernel's on 512 threads, and the planner's occupancy
    query (cached_occupancy, printed with MWF_DEBUG) reports two resident workgroups per CU for each of the four kernels."""
    small, _ = routing_batches()
    monkeypatch.setenv("MWF_DEBUG", "1")
    for slots in (3, 4):
        for flag in (0, 1):
            eng = engine(tun=(("mid_max_pairs", 0), ("wide_slots", slots)))
            b = eng.upload(PackedBatch(small))
            b.align(mw.opt_init(flag=flag))
            b.results()
            b.free()
            eng.close()
            err = capfd.readouterr().err
            lines = [ln for ln in err.splitlines() if "kernel kind 2: block 512" in ln]
            assert lines and all(", 2 workgroup(s) per CU" in ln for ln in lines), (slots, flag, err[-1500:])
            assert f"wfa_band2_nib_kernel T 512 K {slots} E1 2 E2 1 TB {flag} " in err, (slots, flag, err[-1500:])


# ---- (d) edge cases of the 4-bit probe and walks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["score-folded", "score-unfolded", "cigar"])
@pytest.mark.parametrize("geom", list(c16.GEOMS))
def test_edge_cases(oracle, geom, mode):
    """Every edge pair (exact-match runs of 0 ... 1030 bases behind a mismatch with room left and ending at the end of the target, the query, both; sequence lengths with
    len % 8 in {0, 1, 7}; codes 0 and 15 side by side; an identical pair; a CIGAR whose back-match crosses dword boundaries) on 512 x 3, 512 x 4 and the span geometry,
    score-only folded, score-only unfolded and with CIGAR: the oracle's answers, on the 4-bit kernel, with no pair handed back."""
    cases = c16.edge()
    pairs = [(t, q) for _, t, q, _ in cases]
    exp = c16.expected(oracle, "edge", pairs)
    eng = engine(tun=c16.tunables(geom, 0 if mode == "score-unfolded" else 1))
    b = eng.upload(PackedBatch(pairs))
    b.align(mw.opt_init(flag=1 if mode == "cigar" else 0))
    s, it, nc = b.results()
    bad = [(cases[i][0], int(s[i]), int(it[i]), exp[i][0], exp[i][1]) for i in range(len(pairs)) if (int(s[i]), int(it[i])) != exp[i][:2]]
    assert not bad, (geom, mode, bad[:6])
    if mode == "cigar":
        for i in range(len(pairs)):
            assert b.cigar(i, int(nc[i])).tolist() == exp[i][2], (geom, cases[i][0])
    r = route(eng)
    assert (r["kernel_kind"], r["packed"], r["block"], r["n_retries"]) == (2, 1, 1024 if geom == "span" else 512, 0), (geom, mode, r)
    assert set(b.alphabet().tolist()) == {3}
    b.free()
    eng.close()


# ---- (e) wrapped batch: classes follow the current contents -----------------------------------------------------------------------------------------------
def test_wrapped_batch_follows_its_contents(oracle):
    """Overwrite the sequence tensor in place: pairs move between classes 3 (ACGT+N), 1 (lower case) and 2 (seventeen symbols); classes and answers follow at the next align."""
    import torch
    dev = torch.device("cuda", 0)
    base = [c16.base_pair(73000 + i, 2000, 0.05) for i in range(12)]
    first = [c16.recode("acgtn", t, q, 73100 + i) for i, (t, q) in enumerate(base)]
    second = [(t.lower(), q.lower()) if i % 3 == 0 else c16.recode("sym17", t, q, 73200 + i) if i % 3 == 1 else f for i, ((t, q), f) in enumerate(zip(base, first))]
    third = [c16.recode("sym16", t, q, 73300 + i) if i % 2 else (t, q) for i, (t, q) in enumerate(base)]
    eng = engine(tun=(("mid_max_pairs", 0),))
    pk = PackedBatch(first)
    b = eng.wrap_packed(pk, dev)
    seqs = b._keep[0]
    for label, pairs in (("first", first), ("second", second), ("third", third), ("first again", first)):
        assert all((len(t), len(q)) == (len(t0), len(q0)) for (t, q), (t0, q0) in zip(pairs, first))
        seqs.copy_(torch.from_numpy(c16.seq_buffer(pk, pairs)).to(dev))
        torch.cuda.synchronize(dev)
        b.align(mw.opt_init(flag=1))
        check_answers(b, c16.expected(oracle, "follow-" + label.split()[0], pairs), label)
        want = [mw.alphabet_class16(t, q)[0] for t, q in pairs]
        assert b.alphabet().tolist() == want, label
        if label == "second":
            assert set(want) == {1, 2, 3}
    b.free()
    eng.close()


# ---- (f) summaries and maps read the original bytes -------------------------------------------------------------------------------------------------------
def test_summaries_and_maps_read_the_original_bytes():
    small, _ = routing_batches()
    got = []
    for alpha16 in (1, 0):
        eng = engine(alpha16=alpha16, tun=(("mid_max_pairs", 0),))
        b = eng.upload(PackedBatch(small))
        b.align(mw.opt_init(flag=1))
        b.results()
        assert set(b.alphabet().tolist()) == ({3} if alpha16 else {2})
        summ = b.summary()
        vals, off = b.coord_map(0)
        got.append((summ.copy(), vals.copy(), off.copy()))
        b.free()
        eng.close()
    assert (got[0][0]["first_bad"] == -1).all() and (got[1][0]["first_bad"] == -1).all() and (got[0][0]["flags"] == 1).all()
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])


# ---- (g) off means off ------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """alpha16 1 with alpha_remap 0: route and dev_bytes_peak of an engine that never heard of either; alpha16 2 raises."""
    small, _ = routing_batches()
    seen = []
    for touch in (False, True):
        eng = mw.Engine(0)
        eng.set("mid_max_pairs", 0)
        if touch:
            eng.set("alpha_remap", 0)
            eng.set("alpha16", 1)
        b = eng.upload(PackedBatch(small))
        b.align(mw.opt_init(flag=1))
        b.results()
        with pytest.raises(RuntimeError, match="alpha_remap"):
            b.alphabet()
        assert eng.alpha_ms() == (0.0, 0.0)
        seen.append((route(eng), eng.stats().dev_bytes_peak))
        b.free()
        eng.close()
    assert seen[0] == seen[1], seen
    assert seen[0][0]["block"] == 768
    eng = mw.Engine(0)
    for bad in (2, -1):
        with pytest.raises(ValueError):
            eng.set("alpha16", bad)
    with pytest.raises(ValueError):
        eng.set("alpha_remap", 2)
    eng.close()


def test_arena_fallback(oracle):
    """"alpha_arena_budget" (test hook) of one byte: the arena "does not fit" — byte-wise route on the original bytes, same answers, classes still reported; without the
    hook the same batch takes the 4-bit route."""
    small, _ = routing_batches()
    exp = c16.expected(oracle, "small", small, flag=1)
    for budget in (1, -1):
        eng = engine(tun=(("mid_max_pairs", 0), ("alpha_arena_budget", budget)))
        b = eng.upload(PackedBatch(small))
        b.align(mw.opt_init(flag=1))
        check_answers(b, exp, ("budget", budget))
        assert set(b.alphabet().tolist()) == {3}
        r = route(eng)
        assert (r["kernel_kind"], r["packed"]) == (2, 1) and r["block"] == (768 if budget == 1 else 512), (budget, r)
        b.free()
        eng.close()


# ---- (h) MWF_ALPHA16: the engines the drop-in calls create ----------------------------------------------------------------------------------------------------
_CHILD = """
import json, sys
try:
    import torch
except ImportError:
    pass
sys.path.insert(0, sys.argv[1])
import miniwfa_amd as mw
import alpha16_cases as c16
pairs = c16.routing_pairs(17, 12000, 0.03, 74000)
r = mw.wfa_batch(pairs, mw.opt_init(flag=1))
print(json.dumps([[s, it, c] for s, it, c in r]))
"""


def test_environment_variable_reaches_the_drop_in_calls(oracle):
    """mwf_wfa_batch of 17 pairs of 12 kb with N (too many for the whole-device kernel, too long for plain 16-bit offsets) in a child process, with and without
    MWF_ALPHA16=1: the oracle's answers both times; with it the launches are wfa_band2_nib_kernel's (kind 2), without it the generic kernel's (kind 0) — read off the
    library's MWF_DEBUG lines."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = c16.routing_pairs(17, 12000, 0.03, 74000)
    exp = c16.expected(oracle, "env", pairs)
    for on in (True, False):
        env = {k: v for k, v in os.environ.items() if k not in ("MWF_ALPHA16", "MWF_ALPHA_REMAP")}
        env.update({"MWF_DEBUG": "1", "PYTHONPATH": root + os.pathsep + env.get("PYTHONPATH", "")}, **({"MWF_ALPHA16": "1"} if on else {}))
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(root, "tests")], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert [(s, it, c) for s, it, c in got] == [(s, it, c) for s, it, c in exp], on
        kinds = {ln.split("kernel kind ")[1][0] for ln in r.stderr.splitlines() if "kernel kind " in ln}
        assert kinds == ({"2"} if on else {"0"}), (on, kinds, r.stderr[-1500:])
        assert ("wfa_band2_nib_kernel" in r.stderr) == on
