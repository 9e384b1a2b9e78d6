"""One test per entry of tests/ends_matrix.py — the bodies ends_pass<T, TB, EXT> of wfa_ends_kernel<T, EXT> (miniwfa_amd/csrc/mwf_ends.hip) — and the edge
tests of that kernel.

Per entry, penalty set (all twelve shapes of the generic kernel's table) and allowance set (ends form, five) or (A, Z) (EXT, two), one align of the entry's batch:
  - the launch record (MWF_DEBUG, stderr: `kernel kind 3` and `ends-free launch:` / `extension launch:`) is the align's only launch, names this form and this
    workgroup size and carries every pair of the batch; n_retries does not move
  - s, n_iter, the end cell and, for EXT, info equal the restatement's (tests/golden/ends_matrix.jsonl, which tests/test_ends_matrix_cpu.py recomputes and checks
    against the oracle and the DP), bit for bit — integer work, no tolerance
  - with traceback the CIGAR passes ends_ref.check_cigar / ext_ref.check_ext_cigar on every pair and, under zero allowances, its words are the oracle's
  - score-only: n_cigar == 0, the begin ranges are -1 (ends form) or 0 (EXT), and s, n_iter, the end cell and info equal the traceback twin's run of the same cell
Device results are shared between the twins (_device_cache): the traceback run of a cell is executed by whichever test asks for it first.  A test checks every one
of its cells and fails with the list of all that are red.
On an MI355X: 336 aligns in the eight entry tests, largest s 2104 (T256 ends), 642 (T256 ext), 1725 (T512 ends), 889 (T512 ext); 8192 pairs on 1792 workgroups; 2.4 s in all.

That the table can fail was tried once with three libraries built from copies of mwf_ends.hip in which one computed value was changed (never an address or a
bound on an access); nothing faulted:
  A  track_good one slice short (< nH - 1): the four ends-form entries red (39 of 60 cells at 256 threads, 10 of 60 at 512), by n_iter; the EXT entries green —
     an extension's shrink finds every column of its band good in the other slices too (tests/test_ends_matrix_cpu.py::test_coverage_conditions)
  D  ext_take's V > B made V >= B (a later penalty's equal V replaces the remembered cell): the four EXT entries red (15 of 24 cells, 4 of 24), the others green
  E  the edge flags (flags[.][0], [.][1]) not cleared when a pair starts: all eight entries and both persistent-loop tests red
"""
import ctypes as C
import re

import pytest

import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch
from oracle.pyoracle import make_opt

import ends_matrix as em
import ends_ref as er
import ext_ref as xr

pytestmark = pytest.mark.gpu

FREE = er.FREE
KIND_LINE = re.compile(r"\[libmwf_hip\] kernel kind (-?\d+): block (\d+), .* (\d+) pairs; grid (\d+)")
ENDS_LINE = re.compile(r"\[libmwf_hip\] (ends-free|extension) launch: T (\d+), (\d+) pairs, grid (\d+), allowances (-?\d+) (-?\d+) (-?\d+) (-?\d+), match (-?\d+), zdrop (-?\d+)")

_device_cache: dict = {}
_oracle_cigars: dict = {}


@pytest.fixture(scope="module")
def eng():
    e = mw.Engine(0)
    yield e
    e.close()


def launches(err: str):
    """([kernel kind, block, pairs, grid] of every launch, [form, T, pairs, grid, allowances, match, zdrop] of every launch of this kernel) of one align."""
    kinds = [tuple(map(int, m.groups())) for m in map(KIND_LINE.search, err.splitlines()) if m]
    ends = [(m.group(1),) + tuple(map(int, m.groups()[1:])) for m in map(ENDS_LINE.search, err.splitlines()) if m]
    return kinds, ends


def run(eng, pairs, pen, cigar: bool, ext: int, cfg, capfd, **okw):
    """One align of `pairs`: dict(s, it, nc, cig, rng, info, retries, kinds, ends)."""
    x, o1, e1, o2, e2 = pen
    opt = mw.opt_init(flag=mw.MWF_F_CIGAR if cigar else 0, x=x, o1=o1, e1=e1, o2=o2, e2=e2, **okw)
    b = eng.upload(PackedBatch(list(pairs)))
    try:
        r0 = int(eng.stats().n_retries)
        capfd.readouterr()
        if ext:
            b.align_ext(opt, *cfg)
        else:
            b.align_ends(opt, *cfg)
        s, it, nc = b.results()   # (a re-run of what was handed back would be launched here)
        cig = None
        if cigar:
            b.fetch_cigars()
            cig = [b.cigar(i, int(nc[i])).tolist() for i in range(b.n)]
        rng = b.ranges().tolist()
        info = b.ext_info().tolist() if ext else None
        kinds, ends = launches(capfd.readouterr().err)
        return dict(opt=opt, s=s.tolist(), it=it.tolist(), nc=nc.tolist(), cig=cig, rng=rng, info=info, retries=int(eng.stats().n_retries) - r0, kinds=kinds, ends=ends)
    finally:
        b.free()


def check_launch(got, T: int, ext: int, cfg, n_pairs: int, label):
    """The align's only launch: this kernel, this form, this many threads, every pair; nothing was run again."""
    assert len(got["kinds"]) == 1 and got["kinds"][0][:3] == (3, T, n_pairs), (label, got["kinds"])
    assert len(got["ends"]) == 1, (label, got["ends"])
    form, t, n, grid = got["ends"][0][:4]
    assert (form, t, n) == ("extension" if ext else "ends-free", T, n_pairs) and 1 <= grid <= n_pairs, (label, got["ends"])
    if ext:
        assert got["ends"][0][4:] == (0, FREE, 0, FREE) + tuple(cfg), (label, got["ends"])
    else:
        assert got["ends"][0][4:8] == tuple(cfg), (label, got["ends"])
    assert got["retries"] == 0, (label, "pairs were run again", got["retries"])


def check_answers(got, exp, pairs, ext: int, cfg, cigar: bool, label, oracle=None, pen_name=None):
    """Every pair against the restatement's answer; the CIGAR through the checker and, under zero allowances, against the oracle's words."""
    assert len(exp) == len(pairs) == len(got["s"]), label
    for i, ((t, q), w) in enumerate(zip(pairs, exp)):
        rng = got["rng"][i]
        assert (got["s"][i], got["it"][i], rng[1], rng[3]) == tuple(w[:4]), (label, i, (got["s"][i], got["it"][i], rng), w)
        if ext:
            assert tuple(got["info"][i]) == tuple(w[4:8]), (label, i, got["info"][i], w)
        if not cigar:
            assert got["nc"][i] == 0 and (rng[0], rng[2]) == ((0, 0) if ext else (-1, -1)), (label, i, rng)
            continue
        assert len(got["cig"][i]) == got["nc"][i], (label, i)
        if ext:
            xr.check_ext_cigar(mw, got["opt"], t, q, got["cig"][i], rng, got["s"][i])
        else:
            er.check_cigar(mw, got["opt"], t, q, got["cig"][i], rng, cfg, got["s"][i])
            if tuple(cfg) == (0, 0, 0, 0):
                key = (t, q, pen_name)
                if key not in _oracle_cigars:
                    _oracle_cigars[key] = oracle.align(t, q, make_opt(flag=1, **em.PEN[pen_name]))[2] or []
                assert got["cig"][i] == _oracle_cigars[key], (label, i, "the CIGAR words differ from the oracle's")


def _device(eng, inst, pen_name, cfg, capfd):
    key = (inst, pen_name, cfg)
    if key not in _device_cache:
        _device_cache[key] = run(eng, em.batch(inst, pen_name, cfg), em.pen_tuple(pen_name), bool(inst.TB), inst.EXT, cfg, capfd)
    return _device_cache[key]


def _check_cell(eng, oracle, capfd, inst, pen_name, cfg):
    label = f"{em.inst_id(inst)} {pen_name} {em.run_key(inst.T, inst.EXT, pen_name, cfg)}"
    pairs = em.batch(inst, pen_name, cfg)
    got = _device(eng, inst, pen_name, cfg, capfd)
    check_launch(got, inst.T, inst.EXT, cfg, len(pairs), label)
    check_answers(got, em.expected(inst, pen_name, cfg), pairs, inst.EXT, cfg, bool(inst.TB), label, oracle, pen_name)
    if not inst.TB:   # ... and what the traceback twin computes on the same inputs
        tw = _device(eng, inst._replace(TB=1), pen_name, cfg, capfd)
        assert got["s"] == tw["s"] and got["it"] == tw["it"] and got["info"] == tw["info"], (label, "score-only differs from its traceback twin")
        assert [(r[1], r[3]) for r in got["rng"]] == [(r[1], r[3]) for r in tw["rng"]], (label, "end cells differ from the traceback twin's")
    return max(got["s"])


@pytest.mark.parametrize("inst", em.MATRIX, ids=em.inst_id)
def test_ends_instantiation(inst, eng, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MWF_DEBUG", "1")
    red, s_max = [], -1
    cells = em.cells(inst)
    for pen_name, cfg in cells:   # every cell is checked, whatever an earlier one found
        try:
            s_max = max(s_max, _check_cell(eng, oracle, capfd, inst, pen_name, cfg))
        except AssertionError as e:   # (an error of the library ends the test: nothing more is launched after it)
            red.append(f"{em.run_key(inst.T, inst.EXT, pen_name, cfg)}: {str(e).splitlines()[0][:300] if str(e) else 'assert'}")
    with capfd.disabled():
        print(f"\n   {em.inst_id(inst)}: {len(cells)} cells, largest s {s_max}, {len(red)} red")
    assert not red, (em.inst_id(inst), f"{len(red)} of {len(cells)} cells", red)


# ---- the stop rules inside the 512-thread form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [0, 1], ids=["ends", "ext"])
@pytest.mark.parametrize("cigar", [False, True], ids=["score", "cigar"])
def test_stops_in_the_wide_form(eng, ext, cigar, capfd, monkeypatch):
    """max_iter stops pair (c) — and max_s = 4095, which leaves the window the plan sizes the launch by at 2 x 4096 + 3 columns, stops pair (b) under zero
    allowances, a gap of 4200 bases (ends form; an extension of (b) ends below that penalty) — inside a launch on 512 threads: s == -1, ranges and info -1, no CIGAR."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    w = em._wide()
    pen = em.pen_tuple("default")
    cfg = em.EXT_WIDE[0] if ext else (0, 0, 0, 0)
    assert em.expected(em.Inst(512, ext, 0), "default", cfg)[-1][1] > 4 * 20000   # (c)'s n_iter
    stops = [([w["c"]], dict(max_iter=20000))] + ([] if ext else [([w["b"]], dict(max_s=4095))])
    for pairs, kw in stops:
        assert em.window_block(em.PEN["default"], pairs, kw.get("max_s", 0)) == 512
        got = run(eng, pairs, pen, cigar, ext, cfg, capfd, **kw)
        check_launch(got, 512, ext, cfg, 1, kw)
        assert got["s"] == [-1] and got["nc"] == [0] and got["rng"] == [[-1] * 4] and (got["info"] == [[-1] * 4] if ext else got["info"] is None), (kw, got)
        if "max_iter" in kw:
            assert got["it"][0] > kw["max_iter"], got["it"]


# ---- ring depth 256 against 257 ----------------------------------------------------------------------------------------------------------
def test_ring_257_is_refused(eng, oracle, capfd, monkeypatch):
    """nH = 256 (o2 = 254) is the deepest ring the kernel takes — the entry tests run it — and nH = 257 is refused by both entry points with the existing message;
    the engine's next align is right."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    inst = em.Inst(256, 0, 1)
    pairs = em.batch(inst, "default", (0, 0, 0, 0))
    p = em.PEN[em.REFUSED]
    opt = mw.opt_init(flag=mw.MWF_F_CIGAR, **p)
    L = mw.lib()
    b = eng.upload(PackedBatch(list(pairs)))
    try:
        rc = L.mwf_gpu_batch_align_ends(eng.h, b.h, C.byref(opt), C.byref(mw.MwfEnds(7, 0, 0, 1000)))
        assert rc == -2 and "256" in eng.error(), (rc, eng.error())
        rc = L.mwf_gpu_batch_align_ext(eng.h, b.h, C.byref(opt), C.byref(mw.MwfExt(1, -1)))
        assert rc == -2 and "256" in eng.error(), (rc, eng.error())
    finally:
        b.free()
    for ext, cfg in ((0, (7, 0, 0, 1000)), (1, em.EXT_NARROW[1])):
        got = run(eng, pairs, em.pen_tuple("ring256"), True, ext, cfg, capfd)
        check_launch(got, 256, ext, cfg, len(pairs), "after the refusal")
        check_answers(got, em.expected(em.Inst(256, ext, 1), "ring256", cfg), pairs, ext, cfg, True, "after the refusal", oracle, "ring256")


# ---- a workgroup's second and later pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [0, 1], ids=["ends", "ext"])
def test_persistent_loop(eng, ext, capfd, monkeypatch):
    """8192 pairs — 32 distinct ones, six of them beyond penalty 256 under these allowances, 256 times each in a seeded shuffled order — on at most 2048 workgroups:
    every workgroup aligns four or more pairs one after the other, each on what the one before left in LDS, in the ring rows and in the good words.  Every copy's
    s, n_iter, ranges, info and CIGAR words are those of the 32 pairs aligned as a batch of their own, which are the restatement's."""
    monkeypatch.setenv("MWF_DEBUG", "1")
    base, order = em.loop_pairs(), em.loop_order()
    cfg = em.LOOP_EXT if ext else em.LOOP_ALLOW
    small = run(eng, base, em.LOOP_PEN, True, ext, cfg, capfd)
    check_launch(small, 256, ext, cfg, 32, "the 32 pairs")
    check_answers(small, em.expected("loop", "default", cfg), base, ext, cfg, True, "the 32 pairs")
    got = run(eng, [base[k] for k in order], em.LOOP_PEN, True, ext, cfg, capfd)
    check_launch(got, 256, ext, cfg, em.LOOP_COPIES, "the 8192 pairs")
    grid = got["ends"][0][3]
    with capfd.disabled():
        print(f"\n   {'extension' if ext else 'ends-free'}: {em.LOOP_COPIES} pairs on {grid} workgroups")
    assert em.LOOP_COPIES >= 2 * grid, grid
    for field in ("s", "it", "nc", "rng", "cig") + (("info",) if ext else ()):
        bad = [i for i, k in enumerate(order) if got[field][i] != small[field][k]]
        assert not bad, (field, len(bad), bad[:8], [int(order[i]) for i in bad[:8]])
