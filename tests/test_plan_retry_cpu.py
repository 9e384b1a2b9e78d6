"""The retry layer's route table and re-route rule (miniwfa_amd/csrc/mwf_plan_retry.h), checked on the CPU: a stand-alone program (tests/host/plan_retry.cpp, built
with -fsanitize=address,undefined; nothing is loaded into python) prints the table and the rule's decision for a pair.  The table is pinned against what the seven
re-run calls and the ends-free re-run of finalize() passed before there was a table, the rule against a hand-written list: one pair per branch of the if / else chain
finalize() held before there was a rule, and one on each side of every limit in it.  This is the only coverage of the whole-device kernel's "gave up" and
span-overflow branches."""
import os
import subprocess

import pytest

from conftest import ROOT

# mwf_internal.h, mwf_plan_classes.h
ST_TB, ST_ROWS, ST_CIGAR, ST_SNAP, ST_INTERNAL, ST_PENDING, ST_BAND, ST_ALPHABET = 2, 3, 4, 5, 6, 7, 8, 9
GENERIC, WIDE, SMALL, TINY, MICRO, SPAN = 0, 1, 2, 3, 4, 13
STEP0, SHARED, GAVE_UP, COOP_WIDE, NARROW, THREE = 1, 2, 8, 16, 32, 64
GEOM_CHOOSE, GEOM_SPAN = 0, 7
COPY_2BIT, COPY_BYTES = 0, 1
WIDE4 = (8 * 4 - 1) * 256 - 64      # kBandWide4Window
SPAN_WINDOW = (80 - 1) * 256 - 64   # band_window(band2_span_chunks())
SPAN_MAX_SEQ = 62000                # kBandSpanMaxSeq
assert (WIDE4, SPAN_WINDOW) == (7872, 20160)

# the routes, in launch order, then the failures
COOP_ALONE, ENDS_FEWER, TO_GENERIC, TO_GENERIC32, BAND_WIDE, BAND_SPAN, BAND_BYTES, FEWER_GENERIC, FEWER_BAND, FAIL_TB, FAIL_SNAP, FAIL_STATUS = range(12)
LAUNCH_PAIR, LAUNCH_ENDS, LAUNCH_COOP = 0, 1, 2
SLOTS_GRID0, SLOTS_ALL, SLOTS_TB = 0, 1, 2
WARN_GAVE_UP, WARN_SPAN = 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan_retry") / "plan_retry"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "miniwfa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "plan_retry.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(out)


def test_route_table(exe):
    r = subprocess.run([exe, "table"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    keys = ("launch", "want_kind", "slots", "use_forecast", "geom", "span_if_all", "copy", "nib_split", "ring16_allowed", "fewer")
    rows = []
    for ln in r.stdout.splitlines():
        num, name, *vals = ln.split()
        assert int(num) == len(rows)
        rows.append((name, dict(zip(keys, map(int, vals)))))
    # launch order within a round: the whole-device kernel alone, the ends-free re-run, then
    #   rerun(to_generic[z], z, 0, grid0)
    #   rerun(to_generic32[z], z, 0, grid0, false, GEOM_CHOOSE, COPY_2BIT, false)
    #   rerun(to_band_wide[z], z, 2, wide, true)
    #   rerun(to_band_span[z], z, 2, wide, false, GEOM_SPAN)
    #   rerun(to_band_bytes[z], z, 2, wide, false, GEOM_CHOOSE, COPY_BYTES)
    #   rerun(same_fewer[0][z], z, 0, max(1, min(tb_slots, size)))
    #   rerun(same_fewer[2][z], z, 2, max(1, min(tb_slots, size)), false, all_span ? GEOM_SPAN : GEOM_CHOOSE)
    # with the defaults use_forecast = false, geom = GEOM_CHOOSE, copy = COPY_2BIT, ring16_allowed = true; rerun() split a list into class-3 pairs and the rest
    # unless want_kind != 2 or copy == COPY_BYTES.
    def pair_row(want_kind, slots, use_forecast=0, geom=GEOM_CHOOSE, copy=COPY_2BIT, ring16_allowed=1, span_if_all=0):
        return dict(launch=LAUNCH_PAIR, want_kind=want_kind, slots=slots, use_forecast=use_forecast, geom=geom, span_if_all=span_if_all, copy=copy,
                    nib_split=int(want_kind == 2 and copy != COPY_BYTES), ring16_allowed=ring16_allowed, fewer=int(slots == SLOTS_TB))
    assert [name for name, _ in rows] == ["coop-alone", "ends-fewer", "generic", "generic32", "band-wide", "band-span", "band-bytes", "fewer-generic", "fewer-band"]
    assert rows[COOP_ALONE][1]["launch"] == LAUNCH_COOP and rows[COOP_ALONE][1]["fewer"] == 0
    # run_ends_kernel(..., max(1, min(tb_slots, size)), G, false): no forecast, no split
    ends = rows[ENDS_FEWER][1]
    assert (ends["launch"], ends["slots"], ends["use_forecast"], ends["nib_split"], ends["span_if_all"], ends["fewer"]) == (LAUNCH_ENDS, SLOTS_TB, 0, 0, 0, 1)
    assert rows[TO_GENERIC][1] == pair_row(0, SLOTS_GRID0)
    assert rows[TO_GENERIC32][1] == pair_row(0, SLOTS_GRID0, ring16_allowed=0)
    assert rows[BAND_WIDE][1] == pair_row(2, SLOTS_ALL, use_forecast=1)
    assert rows[BAND_SPAN][1] == pair_row(2, SLOTS_ALL, geom=GEOM_SPAN)
    assert rows[BAND_BYTES][1] == pair_row(2, SLOTS_ALL, copy=COPY_BYTES)
    assert rows[FEWER_GENERIC][1] == pair_row(0, SLOTS_TB)
    assert rows[FEWER_BAND][1] == pair_row(2, SLOTS_TB, span_if_all=1)


RULE = dict(band_span=1, seq2bit=1, force_kind=-1, block=0, tb_budget_mb=0, coop_tb_mult=1, step=0, span_window=SPAN_WINDOW, tb_slots=8, can_grow=1)


def pair(status, kind, cls=GENERIC, flags=0, n_iter=1000, tl=1000, ql=1000, **rule):
    assert set(rule) <= set(RULE)
    return dict(RULE, **rule), dict(tl=tl, ql=ql, status=status, kind=kind, cls=cls, flags=flags, n_iter=n_iter)


def went(route, step0=0, cls=None, flags=None, four=0, grow=0, warn=0, asked=0):
    return dict(route=route, step0=step0, cls=cls, flags=flags, four=four, grow=grow, warn=warn, asked=asked)


def band_overflow_cases():
    """ST_BAND_OVERFLOW on the band kernel: the forecast on each side of the four-slot window, from each kind of class, with and without FLAG_THREE_SLOTS."""
    out = []
    for three in (0, THREE):
        for keep in (0, STEP0):
            f = three | keep
            for n_iter, est in ((0, 0), (5000, 0), (-WIDE4, WIDE4), (-(WIDE4 + 1), WIDE4 + 1)):
                four = int(bool(three) and est == 0)
                small = est <= WIDE4
                # neither generic nor wide: the wide class while the forecast fits four slots, else the span geometry (a band size class) or the generic kernel (CLS_SPAN)
                out.append((pair(ST_BAND, 2, MICRO, f, n_iter), went(BAND_WIDE if small else BAND_SPAN, keep, WIDE if small else SPAN, keep, four)))
                out.append((pair(ST_BAND, 2, SMALL, f, n_iter), went(BAND_WIDE if small else BAND_SPAN, keep, WIDE if small else SPAN, keep, four)))
                out.append((pair(ST_BAND, 2, SPAN, f, n_iter), went(BAND_WIDE if small else TO_GENERIC, keep, WIDE if small else GENERIC, keep, four)))
                # wide: the span geometry whatever the forecast; generic: the generic kernel
                out.append((pair(ST_BAND, 2, WIDE, f, n_iter), went(BAND_SPAN, keep, SPAN, keep, four)))
                out.append((pair(ST_BAND, 2, GENERIC, f, n_iter), went(TO_GENERIC, keep, GENERIC, keep, four)))
    return out


def cases():
    c = []
    # ---- ends-free pairs
    c.append((pair(ST_TB, 3, tb_slots=8), went(ENDS_FEWER, 0, GENERIC, 0)))
    c.append((pair(ST_TB, 3, tb_slots=2), went(ENDS_FEWER, 0, GENERIC, 0)))
    c.append((pair(ST_TB, 3, tb_slots=1), went(FAIL_TB)))
    for st in (ST_ROWS, ST_CIGAR, ST_SNAP, ST_INTERNAL, ST_PENDING, ST_BAND, ST_ALPHABET):
        c.append((pair(st, 3), went(FAIL_STATUS)))
    # ---- generic pairs: 16-bit ring rows outgrown
    c.append((pair(ST_BAND, 0), went(TO_GENERIC32, 0, GENERIC, 0)))
    c.append((pair(ST_BAND, 0, WIDE, STEP0), went(TO_GENERIC32, 1, WIDE, STEP0)))
    # ---- band pairs: not plain A/C/G/T
    c.append((pair(ST_ALPHABET, 2, SPAN), went(TO_GENERIC, 0, GENERIC, 0)))
    c.append((pair(ST_ALPHABET, 2, SPAN, STEP0), went(TO_GENERIC, 1, GENERIC, STEP0)))
    for cls in (WIDE, SMALL, TINY, MICRO, GENERIC):
        c.append((pair(ST_ALPHABET, 2, cls), went(BAND_BYTES, 0, cls, 0)))
    c.append((pair(ST_ALPHABET, 2, MICRO, STEP0 | THREE), went(BAND_BYTES, 1, MICRO, STEP0 | THREE)))
    # ---- band pairs: window overflow
    c += band_overflow_cases()
    # span_ok, term by term: a wide pair with a forecast beyond the four-slot window
    beyond = -(WIDE4 + 1)
    c.append((pair(ST_BAND, 2, WIDE, 0, beyond), went(BAND_SPAN, 0, SPAN, 0)))
    for off in (dict(band_span=0), dict(seq2bit=0), dict(force_kind=2), dict(force_kind=0), dict(block=512), dict(block=64)):
        c.append((pair(ST_BAND, 2, WIDE, 0, beyond, **off), went(TO_GENERIC, 0, GENERIC, 0)))
    c.append((pair(ST_BAND, 2, WIDE, 0, beyond, tl=SPAN_MAX_SEQ, ql=SPAN_MAX_SEQ), went(BAND_SPAN, 0, SPAN, 0)))
    c.append((pair(ST_BAND, 2, WIDE, 0, beyond, tl=1000, ql=SPAN_MAX_SEQ + 1), went(TO_GENERIC, 0, GENERIC, 0)))
    # (a target that long and half the forecast: beyond 16-bit ring rows as well)
    assert SPAN_MAX_SEQ + 1 + (WIDE4 + 1) // 2 + 64 > 65000
    c.append((pair(ST_BAND, 2, WIDE, 0, beyond, tl=SPAN_MAX_SEQ + 1, ql=1000), went(TO_GENERIC32, 0, GENERIC, 0)))
    c.append((pair(ST_BAND, 2, WIDE, 0, 5000, tl=SPAN_MAX_SEQ + 1, ql=1000), went(TO_GENERIC, 0, GENERIC, 0)))   # (no forecast: the 16-bit rows are tried)
    c.append((pair(ST_BAND, 2, WIDE, 0, -SPAN_WINDOW), went(BAND_SPAN, 0, SPAN, 0)))
    c.append((pair(ST_BAND, 2, WIDE, 0, -(SPAN_WINDOW + 1)), went(TO_GENERIC, 0, GENERIC, 0)))
    c.append((pair(ST_BAND, 2, MICRO, 0, -(SPAN_WINDOW + 1)), went(TO_GENERIC, 0, GENERIC, 0)))
    c.append((pair(ST_BAND, 2, WIDE, 0, -1000, span_window=999), went(TO_GENERIC, 0, GENERIC, 0)))
    # tl + est / 2 + 64 against 65000 (integer division)
    for est, route in ((29872, TO_GENERIC), (29873, TO_GENERIC), (29874, TO_GENERIC32)):
        assert 50000 + est // 2 + 64 == (65000 if route == TO_GENERIC else 65001)
        c.append((pair(ST_BAND, 2, GENERIC, 0, -est, tl=50000, ql=50000), went(route, 0, GENERIC, 0)))
        c.append((pair(ST_BAND, 2, WIDE, STEP0, -est, tl=50000, ql=50000), went(route, 1, GENERIC, STEP0)))   # (the forecast is beyond the span window)
    c.append((pair(ST_BAND, 2, GENERIC, 0, 0, tl=64990, ql=100), went(TO_GENERIC, 0, GENERIC, 0)))
    # ---- whole-device pairs
    c.append((pair(ST_INTERNAL, 1), went(TO_GENERIC, 0, GENERIC, GAVE_UP, warn=WARN_GAVE_UP)))
    c.append((pair(ST_INTERNAL, 1, GENERIC, STEP0 | SHARED), went(TO_GENERIC, 1, GENERIC, STEP0 | SHARED | GAVE_UP, warn=WARN_GAVE_UP)))
    c.append((pair(ST_INTERNAL, 1, GENERIC, GAVE_UP), went(FAIL_STATUS)))
    for st in (ST_BAND, ST_TB, ST_SNAP):
        c.append((pair(st, 1, GENERIC, SHARED), went(COOP_ALONE, 0, GENERIC, SHARED)))
        c.append((pair(st, 1, GENERIC, SHARED | STEP0 | NARROW, can_grow=0), went(COOP_ALONE, 0, GENERIC, SHARED | STEP0 | NARROW)))
    c.append((pair(ST_BAND, 1, GENERIC, NARROW), went(COOP_ALONE, 0, GENERIC, NARROW | COOP_WIDE)))
    c.append((pair(ST_BAND, 1, GENERIC, NARROW | COOP_WIDE), went(TO_GENERIC, 0, GENERIC, NARROW | COOP_WIDE, warn=WARN_SPAN)))
    c.append((pair(ST_BAND, 1, GENERIC, 0), went(TO_GENERIC, 0, GENERIC, 0, warn=WARN_SPAN)))
    c.append((pair(ST_BAND, 1, GENERIC, STEP0 | COOP_WIDE), went(TO_GENERIC, 1, GENERIC, STEP0 | COOP_WIDE, warn=WARN_SPAN)))
    for st in (ST_TB, ST_SNAP):
        c.append((pair(st, 1, GENERIC, 0), went(COOP_ALONE, 0, GENERIC, 0, grow=1, asked=1)))
        c.append((pair(st, 1, GENERIC, NARROW | STEP0, coop_tb_mult=(1 << 20) - 1), went(COOP_ALONE, 0, GENERIC, NARROW | STEP0, grow=1, asked=1)))
        # growth refused: by the device, by a fixed budget (not asked), by the multiplier's limit (not asked)
        c.append((pair(st, 1, can_grow=0), went(FAIL_TB, asked=1)))
        c.append((pair(st, 1, tb_budget_mb=1), went(FAIL_TB, asked=0)))
        c.append((pair(st, 1, coop_tb_mult=1 << 20), went(FAIL_TB, asked=0)))
        # ... in low-memory mode: the generic kernel's true two-pass form, unless the pair runs as high-memory
        c.append((pair(st, 1, can_grow=0, step=400), went(TO_GENERIC, 0, GENERIC, 0, asked=1)))
        c.append((pair(st, 1, GENERIC, STEP0, can_grow=0, step=400), went(FAIL_TB, asked=1)))
        c.append((pair(st, 1, tb_budget_mb=64, step=400), went(TO_GENERIC, 0, GENERIC, 0, asked=0)))
    # ---- traceback / snapshot arena of the one-workgroup-per-pair kernels
    for st, fail in ((ST_TB, FAIL_TB), (ST_SNAP, FAIL_SNAP)):
        for kind, route in ((0, FEWER_GENERIC), (2, FEWER_BAND)):
            c.append((pair(st, kind, SPAN, 0, tb_slots=8), went(route, 0, SPAN, 0)))
            c.append((pair(st, kind, WIDE, STEP0 | THREE, tb_slots=2), went(route, 1, WIDE, STEP0 | THREE)))
            c.append((pair(st, kind, tb_slots=1), went(fail)))
    # ---- statuses no re-run answers
    for st in (ST_ROWS, ST_CIGAR, ST_PENDING, 12):
        for kind in (0, 1, 2):
            c.append((pair(st, kind), went(FAIL_STATUS)))
    c.append((pair(ST_ALPHABET, 0), went(FAIL_STATUS)))
    c.append((pair(ST_ALPHABET, 1), went(FAIL_STATUS)))
    c.append((pair(ST_INTERNAL, 0), went(FAIL_STATUS)))
    c.append((pair(ST_INTERNAL, 2), went(FAIL_STATUS)))
    return c


def test_reroute_rule(exe):
    cs = cases()
    text = "".join("%d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d\n" % (
        R["band_span"], R["seq2bit"], R["force_kind"], R["block"], R["tb_budget_mb"], R["coop_tb_mult"], R["step"], R["span_window"], R["tb_slots"], R["can_grow"],
        p["tl"], p["ql"], p["status"], p["kind"], p["cls"], p["flags"], p["n_iter"]) for (R, p), _ in cs)
    r = subprocess.run([exe, "reroute"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [dict(zip(("route", "step0", "cls", "flags", "four", "grow", "warn", "asked"), map(int, ln.split()))) for ln in r.stdout.splitlines()]
    assert len(got) == len(cs)
    bad = []
    for ((R, p), want), g in zip(cs, got):
        if want["route"] >= FAIL_TB:   # the call ends there: only the kind of failure (and whether the device was asked) matters
            ok = (g["route"], g["asked"]) == (want["route"], want["asked"])
        else:
            ok = g == want
        if not ok:
            bad.append((p, {k: v for k, v in R.items() if RULE[k] != v}, want, g))
    assert not bad, bad[:8]
    seen = {g["route"] for g in got}
    assert seen == set(range(12)), "every route and every failure is reached"
    assert {g["warn"] for g in got} == {0, WARN_GAVE_UP, WARN_SPAN}
