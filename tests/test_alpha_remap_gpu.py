"""GPU tests of the "alpha_remap" tunable (include/miniwfa.h; kernels csrc/mwf_alphabet.hip): with 1, a pair of at most four distinct bytes is
copied into a per-batch arena with its bytes mapped onto A/C/G/T and planned and aligned as a plain pair.  Inputs: tests/alpha_remap_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
from oracle.pyoracle import make_opt
import alpha_remap_cases as ac

pytestmark = pytest.mark.gpu

OPT_KEYS = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter")
ROUTE = ("kernel_kind", "packed", "block", "grid", "n_retries")
_cache = {}


def gopt(o):
    return mw.opt_init(**{k: getattr(o, k) for k in OPT_KEYS})


def expected(oracle, key, pairs, o):
    """The oracle's (s, n_iter, CIGAR) of every pair, computed once per (batch, option set) and left alone."""
    k = (key, o.flag, o.x, o.o1, o.e1, o.o2, o.e2)
    if k not in _cache:
        _cache[k] = [oracle.align(t, q, o) for t, q in pairs]
    return _cache[k]


def check_answers(b, exp, label):
    s, it, nc = b.results()
    for i, (es, eit, ecig) in enumerate(exp):
        assert (int(s[i]), int(it[i])) == (es, eit), (label, i)
        if ecig is not None:
            assert b.cigar(i, int(nc[i])).tolist() == ecig, (label, i)


def route(eng):
    st = eng.stats()
    return {k: getattr(st, k) for k in ROUTE}


def routing_batches():
    """(64 x 3 kb at 5 %, 4 x 16 kb at 3 %): upper-case pairs; ac.lower() of them is the batch under test."""
    if "routing" not in _cache:
        _cache["routing"] = (ac.routing_pairs(64, 3000, 0.05, 61000), ac.routing_pairs(4, 16000, 0.03, 62000))
    return _cache["routing"]


def host_classes(pk):
    return [mw.alphabet_class(*pk.pair(i))[0] for i in range(pk.n)]


# ---- (a) classes and answers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pen", ["default", "a22"])
@pytest.mark.parametrize("flag", [0, 1])
def test_classes_and_answers(oracle, pen, flag):
    """One uploaded batch of 42 pairs: every alphabet case at lengths 1 ... 6500, empty sequences, sequences at odd byte offsets, three queries on
    one target range.  Batch.alphabet() equals the host twin's classes; (s, n_iter, CIGAR) equal the oracle's on the original bytes."""
    pk, names = ac.gpu_batch_a()
    pairs = [pk.pair(i) for i in range(pk.n)]
    o = make_opt(flag=flag, **({} if pen == "default" else dict(o2=4, e2=2)))
    eng = mw.Engine(0)
    eng.set("alpha_remap", 1)
    b = eng.upload(pk)
    b.align(gopt(o))
    check_answers(b, expected(oracle, "a", pairs, o), (pen, flag))
    cls = b.alphabet().tolist()
    assert cls == host_classes(pk), [(n, c) for n, c in zip(names, cls)]
    assert {0, 1, 2} <= set(cls)
    # a second align of the same batch replays the copies (an uploaded batch is remapped once)
    peak = eng.stats().dev_bytes_peak
    b.align(gopt(o))
    check_answers(b, expected(oracle, "a", pairs, o), (pen, flag, "again"))
    assert eng.stats().dev_bytes_peak == peak
    b.free()
    eng.close()


@pytest.mark.parametrize("which", ["short", "a", "long"])
def test_wrapped_classes_and_answers(oracle, which):
    """The same through the device's own classification (a wrapped batch: nobody looked at the bytes on the host), once per workgroup size of
    mwf_alphabet.hip: "short" — the pairs of (a) of up to 900 bases, 64 threads; "a" — batch (a) as it is, 256 threads; "long" — three pairs of 34 kb,
    1024 threads.  Each holds a fifth symbol in the last byte of a query, sequences at odd offsets and a class-1 pair; "short" and "a" lengths 1, 15 ... 65,
    empty sequences and a shared target.  Batch.alphabet() equals the host twin's classes, the answers the oracle's on the original bytes."""
    import torch
    pk, names = {"short": ac.gpu_batch_short, "a": ac.gpu_batch_a, "long": ac.gpu_batch_long}[which]()
    pairs = [pk.pair(i) for i in range(pk.n)]
    want = host_classes(pk)
    assert {1, 2} <= set(want) and any(n.startswith("fifth_last_q") for n in names)
    o = make_opt(flag=1)
    eng = mw.Engine(0)
    eng.set("alpha_remap", 1)
    b = eng.wrap_packed(pk, torch.device("cuda", 0))
    b.align(gopt(o))
    check_answers(b, expected(oracle, which, pairs, o), ("wrapped", which))
    cls = b.alphabet().tolist()
    assert cls == want, [(n, c, w) for n, c, w in zip(names, cls, want) if c != w]
    b.free()
    eng.close()


def test_empty_batch_reports_no_classes():
    eng = mw.Engine(0)
    eng.set("alpha_remap", 1)
    b = eng.upload(PackedBatch([]))
    b.align(mw.opt_init())
    assert b.alphabet().tolist() == []
    b.free()
    eng.close()


# ---- (b) routing: fails without the feature (set("alpha_remap", ...) is an error there) ----------------------------------------------------
def _routes(pairs_upper, tun=(), flag=0):
    """route of: the lower-case batch with alpha_remap 1, its upper-case twin with 1, the lower-case batch with 0."""
    out = []
    for pairs, remap in ((ac.lower(pairs_upper), 1), (pairs_upper, 1), (ac.lower(pairs_upper), 0)):
        eng = mw.Engine(0)
        for name, v in tun:
            eng.set(name, v)
        eng.set("alpha_remap", remap)
        b = eng.upload(PackedBatch(pairs))
        b.align(mw.opt_init(flag=flag))
        b.results()
        out.append(route(eng))
        b.free()
        eng.close()
    return out


def test_routing_lower_case_reads_like_its_twin(capsys):
    """64 x 3 kb at 5 %, all lower case: with alpha_remap 1 the align reports the kernel, geometry, grid and re-run count of its upper-cased
    twin; with 0 the byte-wise geometry, 768 threads.  ("mid_max_pairs" 0: a batch of 64 pairs would otherwise go to the one-workgroup-per-pair
    LDS kernel, which has a byte-wise form of its own at the same workgroup size — the band classes are what this test is about.)"""
    small, _ = routing_batches()
    low1, up1, low0 = _routes(small, tun=(("mid_max_pairs", 0),))
    with capsys.disabled():
        print(f"\n   64 x 3 kb: lower/1 {low1}  upper {up1}  lower/0 {low0}")
    assert low1 == up1
    assert (up1["kernel_kind"], up1["packed"]) == (2, 1) and up1["block"] in (128, 256, 512)
    # ... and on the route the batch takes with every tunable at its default (the LDS kernel): again the twin's
    dlow1, dup1, _ = _routes(small)
    with capsys.disabled():
        print(f"   64 x 3 kb, defaults: lower/1 {dlow1}  upper {dup1}")
    assert dlow1 == dup1
    assert (low0["kernel_kind"], low0["packed"], low0["block"]) == (2, 1, 768)


def test_routing_long_lower_case_pairs_keep_the_biased_geometry(capsys):
    """4 x 16 kb at 3 %, lower case ("coop_min_len" beyond them: four pairs this long would otherwise share the whole-device kernel, which reads
    bytes whatever the alphabet).  With 1: kernel_kind, packed and block of the upper-cased twin — the packed band kernel's 512-thread copy on
    biased offsets (block 512), which has no byte-wise form; with 0 the generic kernel, kernel_kind 0."""
    _, long_ = routing_batches()
    low1, up1, low0 = _routes(long_, tun=(("coop_min_len", 1 << 30),))
    with capsys.disabled():
        print(f"\n   4 x 16 kb: lower/1 {low1}  upper {up1}  lower/0 {low0}")
    assert [low1[k] for k in ROUTE[:3]] == [up1[k] for k in ROUTE[:3]]
    assert (up1["kernel_kind"], up1["packed"], up1["block"]) == (2, 1, 512)
    assert low0["kernel_kind"] == 0
    # ... and on the route the batch takes with every tunable at its default (the whole-device kernel): again the twin's
    dlow1, dup1, _ = _routes(long_)
    with capsys.disabled():
        print(f"   4 x 16 kb, defaults: lower/1 {dlow1}  upper {dup1}")
    assert dlow1 == dup1


# ---- (c) summaries over a remapped pair ------------------------------------------------------------------------------------------------------
def test_summaries_and_maps_read_the_original_bytes():
    small, _ = routing_batches()
    got = []
    for pairs in (ac.lower(small), small):
        eng = mw.Engine(0)
        eng.set("alpha_remap", 1)
        b = eng.upload(PackedBatch(pairs))
        b.align(mw.opt_init(flag=1))
        b.results()
        if pairs is not small:
            assert set(b.alphabet().tolist()) == {1}
        summ = b.summary()
        vals, off = b.coord_map(0)
        got.append((summ.copy(), vals.copy(), off.copy()))
        b.free()
        eng.close()
    assert (got[0][0]["first_bad"] == -1).all() and (got[1][0]["first_bad"] == -1).all() and (got[0][0]["flags"] == 1).all()
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])


# ---- (d) wrapped batch: classes follow the current contents ----------------------------------------------------------------------------------
def test_wrapped_batch_follows_its_contents(oracle):
    import torch
    small, _ = routing_batches()
    dev = torch.device("cuda", 0)
    o = make_opt(flag=1)
    retries = {}
    for name, pairs, remap in (("lower1", ac.lower(small), 1), ("upper1", small, 1), ("lower0", ac.lower(small), 0)):
        eng = mw.Engine(0)
        eng.set("alpha_remap", remap)
        b = eng.wrap_packed(PackedBatch(pairs), dev)
        b.align(gopt(o))
        check_answers(b, expected(oracle, name[:5], pairs, o), name)
        retries[name] = eng.stats().n_retries
        if remap:
            assert set(b.alphabet().tolist()) == ({1} if name == "lower1" else {0})
        b.free()
        eng.close()
    # (with 0 nobody has looked at the bytes: every pair is run, handed back as "not plain A/C/G/T" and run again)
    assert retries["lower1"] == retries["upper1"] and retries["lower0"] >= len(small) and retries["lower0"] > retries["lower1"], retries
    # overwrite the sequence tensor in place: other sequences of the same lengths coded 0..3, then the same with an N in eight pairs
    eng = mw.Engine(0)
    eng.set("alpha_remap", 1)
    pk = PackedBatch(ac.lower(small))
    b = eng.wrap_packed(pk, dev)
    seqs = b._keep[0]
    b.align(gopt(o))
    check_answers(b, expected(oracle, "lower", ac.lower(small), o), "wrapped, first contents")
    second = ac.other_same_lengths(small, 63000)
    third = [(t[:1500] + b"N" + t[1501:], q) if i % 8 == 3 else (t, q) for i, (t, q) in enumerate(second)]
    for label, pairs, want in (("second", second, [1] * len(small)), ("third", third, [2 if i % 8 == 3 else 1 for i in range(len(small))])):
        seqs.copy_(torch.from_numpy(ac.seq_buffer(pk, pairs)).to(dev))
        torch.cuda.synchronize(dev)
        b.align(gopt(o))
        check_answers(b, expected(oracle, label, pairs, o), label)
        assert b.alphabet().tolist() == want, label
    assert sum(c == 2 for c in b.alphabet().tolist()) == 8
    b.free()
    eng.close()


# ---- (e) off means off -----------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    small, _ = routing_batches()
    peaks = []
    for explicit in (False, True):
        eng = mw.Engine(0)
        if explicit:
            eng.set("alpha_remap", 0)
        b = eng.upload(PackedBatch(ac.lower(small)))
        with pytest.raises(RuntimeError, match="not aligned"):
            b.alphabet()
        b.align(mw.opt_init(flag=1))
        b.results()
        with pytest.raises(RuntimeError, match="alpha_remap"):
            b.alphabet()
        peaks.append(eng.stats().dev_bytes_peak)
        b.free()
        eng.close()
    assert peaks[0] == peaks[1], peaks
    eng = mw.Engine(0)
    with pytest.raises(ValueError):
        eng.set("alpha_remap", 2)
    eng.close()


# ---- (f) the arena does not fit --------------------------------------------------------------------------------------------------------------
def test_arena_fallback(oracle):
    """"alpha_arena_budget" (test hook) of one byte: the arena "does not fit".  Same answers, classes reported, byte-wise routing; without the hook the same
    batch takes the 2-bit route."""
    small, _ = routing_batches()
    pairs = ac.lower(small)
    o = make_opt(flag=1)
    for budget in (1, -1):
        eng = mw.Engine(0)
        eng.set("mid_max_pairs", 0)
        eng.set("alpha_remap", 1)
        eng.set("alpha_arena_budget", budget)
        b = eng.upload(PackedBatch(pairs))
        b.align(gopt(o))
        check_answers(b, expected(oracle, "lower", pairs, o), ("budget", budget))
        assert set(b.alphabet().tolist()) == {1}
        r = route(eng)
        assert (r["kernel_kind"], r["packed"]) == (2, 1) and (r["block"] == 768) == (budget == 1), (budget, r)
        b.free()
        eng.close()


# ---- MWF_ALPHA_REMAP: the engines the drop-in calls create -----------------------------------------------------------------------------------
_CHILD = """
import json, sys
try:
    import torch
except ImportError:
    pass
import miniwfa_amd as mw
from miniwfa_amd.synth import synth_pair
pairs = [synth_pair(64000 + i, 12000, 0.03) for i in range(17)]
r = mw.wfa_batch([(t.lower(), q.lower()) for t, q in pairs], mw.opt_init(flag=1))
print(json.dumps([[s, it, c] for s, it, c in r]))
"""


def test_environment_variable_reaches_the_drop_in_calls(oracle):
    """mwf_wfa_batch of 17 lower-case pairs of 12 kb (too many for the whole-device kernel, too long for plain 16-bit offsets) in a child process, with
    and without MWF_ALPHA_REMAP=1: the oracle's answers both times; with it the launches are the packed band kernel's (kind 2), without it the generic
    kernel's (kind 0) — read off the library's MWF_DEBUG lines."""
    from miniwfa_amd.synth import synth_pair
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = [tuple(x.lower() for x in synth_pair(64000 + i, 12000, 0.03)) for i in range(17)]
    exp = expected(oracle, "env", pairs, make_opt(flag=1))
    for on in (True, False):
        env = {k: v for k, v in os.environ.items() if k != "MWF_ALPHA_REMAP"}
        env.update({"MWF_DEBUG": "1", "PYTHONPATH": root + os.pathsep + env.get("PYTHONPATH", "")}, **({"MWF_ALPHA_REMAP": "1"} if on else {}))
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert [(s, it, c) for s, it, c in got] == [(s, it, c) for s, it, c in exp], on
        kinds = {ln.split("kernel kind ")[1][0] for ln in r.stderr.splitlines() if "kernel kind " in ln}
        assert kinds == ({"2"} if on else {"0"}), (on, kinds, r.stderr[-1500:])
