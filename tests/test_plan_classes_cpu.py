"""The plan layer's class table and per-pair rule (miniwfa_amd/csrc/mwf_plan_classes.h), checked on the CPU: a stand-alone program
(tests/host/plan_classes.cpp, built with -fsanitize=address,undefined; nothing is loaded into python) prints the class the C++ rule gives a pair, and
that is compared with the Python restatements the GPU matrices are built on — band_matrix.host_class, band_biased_matrix's override of it and
lane_mid_matrix.lane_admits — at every limit of the rule.  The mid kernel is off here (its LDS size lives in a .hip unit): its admission stays with
tests/test_lane_mid_matrix_gpu.py."""
import os
import re
import subprocess

import pytest

import band_matrix as bm
import band_biased_matrix as bbm
import lane_mid_matrix as lm
from conftest import ROOT

CLS = dict(generic=0, wide=1, small=2, tiny=3, micro=4, lowmem=5, wide_bytes=6, small_bytes=7, tiny_bytes=8, micro_bytes=9, lane=10, mid=11, lane_bytes=12,
           span=13, biased=14, wide_nib=15, span_nib=16)
GEOM_CHOOSE, GEOM_LANE, GEOM_MID = 0, 4, 5
COPY_2BIT, COPY_BYTES, COPY_NIB = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan_classes") / "plan_classes"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "miniwfa_amd", "csrc"), os.path.join(ROOT, "tests", "host", "plan_classes.cpp"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(out)


def _chunks():
    """(band2_biased512_chunks(), band2_span_chunks()) as mwf_band2.hip computes them from the kernel header's constants — read from the sources, so that the rule
    is checked with the numbers the library is built with."""
    csrc = os.path.join(ROOT, "miniwfa_amd", "csrc")
    unit, hdr = open(os.path.join(csrc, "mwf_band2.hip")).read(), open(os.path.join(csrc, "mwf_band2_kernel.h")).read()
    assert "int band2_span_chunks() { return kSpanT / 64 * kSpanK; }" in unit and "int band2_biased512_chunks() { return 8 * kW4K; }" in unit
    k = {n: int(re.search(r"constexpr int " + n + r" = (\d+);", hdr).group(1)) for n in ("kSpanT", "kSpanK", "kW4K")}
    return 8 * k["kW4K"], k["kSpanT"] // 64 * k["kSpanK"]


BIASED_CHUNKS, SPAN_CHUNKS = _chunks()
# (the Python restatements spell the same numbers as literals: 48 = biased + 8 chunks, 80 span chunks, 20160 its window)
assert (BIASED_CHUNKS + 8, SPAN_CHUNKS, (SPAN_CHUNKS - 1) * 256 - 64) == (48, 80, 20160)


def classify(exe, rows):
    """rows: (penalties, band2, lane, biased512, wide_slots, band_span, lane_max_len, tl, ql) -> [(class, fallback)]"""
    text = "".join("%d %d %d %d %d  %d %d %d  %d %d  %d %d %d  %d %d\n" % (p["x"], p["o1"], p["e1"], p["o2"], p["e2"], b2, ln, bi, BIASED_CHUNKS, SPAN_CHUNKS, ws, bs, lml, tl, ql)
                   for p, b2, ln, bi, ws, bs, lml, tl, ql in rows)
    r = subprocess.run([exe, "classify"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert len(out) == len(rows)
    return out


def _split(total, skew=0):
    """(tl, ql) with tl + ql == total and ql - tl == skew (or one less, where the parities differ)."""
    tl = (total - skew) // 2
    return max(tl, 0), total - max(tl, 0)


_limit_pairs = {}


def limit_pairs(p):
    """Pairs on both sides of every limit of the rule, for one penalty set."""
    key = tuple(sorted(p.items()))
    if key not in _limit_pairs:
        _limit_pairs[key] = _make_limit_pairs(p)
    return _limit_pairs[key]


def _make_limit_pairs(p):
    pairs = set()
    # limits on tl + ql + 1 (the weighed length of an even pair is its length): the four band classes, the biased and the span geometry; and its window limit
    for lim in (1400, 3600, 8200, 4 * 8 * 3 * 256, 7 * (48 * 256) // 2, 7 * 80 * 256, 20160):
        for d in (-1, 0, 1):
            pairs.add(_split(lim - 1 + d))          # equal lengths (or one apart)
            pairs.add(_split(lim - 1 + d, 1))
    # window limits: a lone gap is all skew, so only the window can admit it (window = tl + ql + 1 while the penalty bound allows that many columns)
    for win in (448, 1216, 2752, 5824, 20160):
        for d in (-1, 0, 1):
            pairs.add((0, win - 1 + d)), pairs.add((win - 1 + d, 0)), pairs.add((7, win - 8 + d))
    # plain 16-bit offsets: tl + penalty bound = 32766 / 32767 (a fixed target, the query grown across the limit), in the wide class's and in the long classes' lengths
    for tl in (9000, 10000, 14000):
        ql = next((q for q in range(1, 60000) if tl + bm.penalty_bound(p, tl, q) >= 32767), None)
        if ql is not None:
            for d in (-2, -1, 0, 1):
                pairs.add((tl, max(1, ql + d)))
    # kBandSpanMaxSeq, either sequence
    for a in (61999, 62000, 62001):
        for b_ in (61999, 62000, 62001, 30000):
            pairs.add((a, b_)), pairs.add((b_, a))
    # skew on each side of len / 16, just below each length limit (beyond it every base of skew counts six-fold)
    for total in (1380, 1381, 3580, 3581, 8180, 8181, 24500, 24501):
        for s in range(total // 16 - 2, total // 16 + 8):
            tl, ql = _split(total, s)
            pairs.add((tl, ql)), pairs.add((ql, tl))
    # equal lengths across the classes
    for L in (1, 100, 699, 700, 1800, 4100, 12288, 21503, 21504, 40000, 62000):
        pairs.add((L, L))
    pairs.add((0, 0))
    return sorted(pairs)


def test_class_table(exe):
    r = subprocess.run([exe, "table"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    rows = {}
    for ln in lines[:-1]:
        c, name, geom, copy, want, fallback, by_work, wide, slot = ln.split()
        rows[int(c)] = dict(name=name, geom=int(geom), copy=int(copy), want=int(want), fallback=int(fallback), by_work=int(by_work), wide=int(wide), slot=int(slot))
    assert sorted(rows) == list(range(17)) and len({r_["name"] for r_ in rows.values()}) == 17
    assert {r_["name"].replace("-", "_").replace("low_mem", "lowmem"): c for c, r_ in rows.items()} == CLS   # the numbers PlanCache::cls0 has always held
    head, *order = lines[-1].split()
    order = [int(c) for c in order]
    assert head == "order" and sorted(order) == list(range(17)), "the run order is a permutation of the classes"
    assert order == [5, 0, 13, 14, 16, 1, 15, 6, 2, 7, 3, 8, 4, 9, 11, 10, 12]
    by_work = [rows[c]["by_work"] for c in order]
    assert sum(by_work) == 6 and "".join(map(str, by_work)).strip("0") == "1" * 6, "the classes dealt by predicted work are contiguous in the run order"
    assert {c for c in rows if rows[c]["by_work"]} == {CLS[k] for k in ("span", "biased", "span_nib", "wide", "wide_nib", "wide_bytes")}
    assert {c for c in rows if rows[c]["wide"]} == {CLS["wide"], CLS["wide_nib"]}
    # every byte-wise and 4-bit twin: its plain class's geometry, its own copy form
    for twin, plain, copy in (("wide_bytes", "wide", COPY_BYTES), ("small_bytes", "small", COPY_BYTES), ("tiny_bytes", "tiny", COPY_BYTES), ("micro_bytes", "micro", COPY_BYTES),
                              ("lane_bytes", "lane", COPY_BYTES), ("wide_nib", "wide", COPY_NIB), ("span_nib", "span", COPY_NIB)):
        assert rows[CLS[twin]]["geom"] == rows[CLS[plain]]["geom"], twin
        assert rows[CLS[twin]]["copy"] == copy and rows[CLS[plain]]["copy"] == COPY_2BIT, twin
        assert rows[CLS[twin]]["fallback"] == rows[CLS[plain]]["fallback"], twin
    assert len({rows[CLS[k]]["geom"] for k in ("wide", "small", "tiny", "micro", "lane", "mid", "span", "biased")}) == 8
    assert rows[CLS["lane"]]["geom"] == GEOM_LANE and rows[CLS["mid"]]["geom"] == GEOM_MID and rows[CLS["wide"]]["geom"] == GEOM_CHOOSE
    # where a pair starts again: a band class, the span geometry or generic — and such a class falls back to itself
    allowed = {CLS[k] for k in ("generic", "wide", "small", "tiny", "micro", "span")}
    for c, r_ in rows.items():
        assert r_["fallback"] in allowed, r_
        assert rows[r_["fallback"]]["fallback"] == r_["fallback"], r_
    assert all(r_["want"] == (0 if r_["name"] in ("generic", "low-mem") else 2) for r_ in rows.values())
    assert {r_["name"]: r_["slot"] for r_ in rows.values() if r_["slot"] >= 0} == {"lane": 0, "lane-bytes": 1}


@pytest.mark.parametrize("wide_slots", [0, 3, 4])
@pytest.mark.parametrize("band_span", [1, 2])
def test_rule_equals_host_class(exe, wide_slots, band_span):
    """COMMON_DEFAULT_ROUTING (lane, mid and whole-device kernels off, div_aware 0): the C++ rule against band_matrix.host_class — which admits the biased class
    for gap extensions (2,1) alone — and against band_biased_matrix's, which admits it for every set whose copies are built; every set of band_matrix.PEN."""
    assert dict(bm.COMMON_DEFAULT_ROUTING)["lane_max_len"] == 0 and dict(bm.COMMON_DEFAULT_ROUTING)["mid_max_pairs"] == 0 and dict(bm.COMMON_DEFAULT_ROUTING)["div_aware"] == 0
    rows, want = [], []
    for name, p in sorted(bm.PEN.items()):
        ext = (p["e1"], p["e2"])
        assert ext in bbm.BUILT_EXT
        for tl, ql in limit_pairs(p):
            rows.append((p, 1, 0, int(ext == (2, 1)), wide_slots, band_span, 0, tl, ql))
            want.append((name, tl, ql, "band_matrix", bm.host_class(p, tl, ql, wide_slots=wide_slots, band_span=band_span)))
            rows.append((p, 1, 0, 1, wide_slots, band_span, 0, tl, ql))
            want.append((name, tl, ql, "band_biased_matrix", bbm.base.host_class(p, tl, ql, wide_slots=wide_slots, band_span=band_span)))
    got = classify(exe, rows)
    bad = [(w, g) for w, g in zip(want, got) if w[4] != g[0]]
    assert not bad, bad[:10]
    # h_class: the class itself, except that a biased pair starts again from the wide class
    assert all(g[1] == (CLS["wide"] if g[0] == CLS["biased"] else g[0]) for g in got)
    seen = {g[0] for g in got}
    assert seen >= ({CLS["span"], CLS["generic"]} if band_span == 2 else {CLS[k] for k in ("generic", "wide", "small", "tiny", "micro", "span")} | ({CLS["biased"]} if wide_slots != 3 else set())), seen
    if wide_slots == 3:
        assert CLS["biased"] not in seen


def test_rule_equals_lane_admits(exe):
    """lane_mid_matrix.lane_admits at lane_max_len - 1, lane_max_len, lane_max_len + 1 and skew 24 / 25, whether or not the band kernel has the set (the lengths' band
    class admits the pair either way)."""
    L = lm.LANE_MAX_LEN
    pairs = set()
    for long_ in (L - 1, L, L + 1):
        for skew in (0, 1, lm.LANE_MAX_SKEW, lm.LANE_MAX_SKEW + 1):
            pairs.add((long_, long_ - skew)), pairs.add((long_ - skew, long_))
    pairs |= {(1, 1), (0, 20), (150, 150), (30, 60)}
    rows, want = [], []
    for name, p in sorted({**lm.PEN, **lm.PEN_BEYOND}.items()):
        for band2 in (0, 1):
            for tl, ql in sorted(pairs):
                rows.append((p, band2, int(lm.lane_supported(p)), 0, 0, 1, L, tl, ql))
                want.append((name, band2, tl, ql, lm.lane_admits(p, tl, ql)))
    got = classify(exe, rows)
    bad = [(w, g) for w, g in zip(want, got) if w[4] != (g[0] == CLS["lane"])]
    assert not bad, bad[:10]
    assert any(w[4] for w in want) and not all(w[4] for w in want)
    # an overflow goes to the 64-thread class where the band kernel has the set, else to whatever choose_kernel has (fallback small)
    assert all(g[1] == (CLS["micro"] if w[1] else CLS["small"]) for w, g in zip(want, got) if g[0] == CLS["lane"])
