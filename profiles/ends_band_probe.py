"""What per-pair parameters cost the old calls, and what a diagonal band buys (mwf_ends.hip; include/miniwfa.h, mwf_band_t).  Method of profiles/ends_probe.py and
profiles/ext_probe.py: HIP-event time around the kernels (GpuStats.kernel_ms), one process, 3 warm-ups, the sides of a comparison alternating align by align,
median [min, max].

  gate    align_ends(0, 0, 0, 0) and align_ext(1, -1) of this tree against the same calls of the PARENT commit's library loaded beside it, on the four batches
          of DESIGN.md section 4.7's gate table: 256 x 2 kb and 1024 x 300 bp at 5 %, score-only and with CIGAR.  The kernels now take the limits of a slice's
          growth from two scalars instead of from constants; the bar is the project's 1.25 x.  The parent is a built checkout of the parent commit:
          --parent DIR (the directory that holds its miniwfa_amd/).  Without it the gate is skipped.
  report  read-in-window batches, 1024 x (2 kb in 2.4 kb) and 4096 x (150 bp in 250 bp) at 5 %, allowances (free, free, 0, 0): bands of +-32, +-100 and +-400
          around each read's true diagonal against no band; time, summed n_iter, traceback bytes per pair (n_iter is one byte per cell) and how many
          pairs keep the unbanded s.

    python profiles/ends_band_probe.py [--parent DIR] [--aligns 20] [--out profiles/ends_band]

Writes ends_band_probe.json and ends_band_probe.txt (the tables of DESIGN.md section 4.7.3) into --out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

try:
    import torch  # noqa: F401  (its HIP runtime first, as tests/conftest.py)
except ImportError:
    pass

import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import PackedBatch, mutate, random_seq, synth_batch  # noqa: E402
from ext_probe import load_parent  # noqa: E402

FREE = mw.ENDS_FREE
WINDOW = (FREE, FREE, 0, 0)
WIDTHS = (32, 100, 400)


def window_batch(seed, n, tl, ql, p):
    """n (window, read) pairs and the diagonal each read was drawn on."""
    rng = np.random.default_rng(seed)
    win, diag = [], []
    for k in range(n):
        t = random_seq(seed * 100000 + k, tl)
        a = int(rng.integers(0, tl - ql + 1))
        win.append((t, mutate(t[a:a + ql], seed * 100000 + 50000 + k, p)))
        diag.append(-a)
    return win, diag


def timed(side):
    """side = (label, engine, batch, align): align(batch) enqueues -> (ms, re-runs, s, n_iter)."""
    label, eng, batch, align = side
    align(batch)
    s, it, _ = batch.results()
    st = eng.stats()
    return float(st.kernel_ms), int(st.n_retries), np.asarray(s, dtype=np.int64), np.asarray(it, dtype=np.int64)


def compare(name, sides, aligns, warmup=3):
    """Alternates the sides align by align; -> one record, ratios against the LAST side."""
    times = {s[0]: [] for s in sides}
    last = {}
    for k in range(warmup + aligns):
        for side in sides:
            ms, retries, s, it = timed(side)
            if k >= warmup:
                times[side[0]].append(ms)
            last[side[0]] = (retries, s, it)
    base_s = last[sides[-1][0]][1]
    rec = dict(name=name, aligns=aligns, sides=[s[0] for s in sides])
    for label, v in times.items():
        retries, s, it = last[label]
        rec[label] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n_retries=retries, s_sum=int(s.sum()), n_iter_sum=int(it.sum()),
                          tb_bytes_per_pair=float(it.mean()), same_s_as_last_side=int((s == base_s).sum()), n_stopped=int((s < 0).sum()))
    base = rec[sides[-1][0]]["median_ms"]
    rec["ratio"] = {s[0]: rec[s[0]]["median_ms"] / base for s in sides[:-1]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aligns", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends_band"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    parent = load_parent(a.parent) if a.parent else None
    mw.lib()
    eng = mw.Engine(0)
    peng = parent.Engine(0) if parent else None
    out = dict(gate=[], report=[], parent=bool(parent))
    if parent:
        for n, tl in ((256, 2000), (1024, 300)):
            pk = PackedBatch(synth_batch(1234, n, tl, 0.05))
            bn, bp = eng.upload(pk), peng.upload(pk)
            for cigar in (0, 1):
                opt, popt = mw.opt_init(flag=cigar), parent.opt_init(flag=cigar)
                for what in ("ends", "ext"):
                    new = (lambda b, o=opt: b.align_ends(o, 0, 0, 0, 0)) if what == "ends" else (lambda b, o=opt: b.align_ext(o, 1, -1))
                    old = (lambda b, o=popt: b.align_ends(o, 0, 0, 0, 0)) if what == "ends" else (lambda b, o=popt: b.align_ext(o, 1, -1))
                    r = compare(f"{what}: {n} x {tl} bp @ 5 %, {'CIGAR' if cigar else 'score'}", [("this_tree", eng, bn, new), ("parent", peng, bp, old)], a.aligns)
                    assert r["this_tree"]["s_sum"] == r["parent"]["s_sum"] and r["this_tree"]["n_iter_sum"] == r["parent"]["n_iter_sum"], r
                    out["gate"].append(r)
                    print(r["name"], r["ratio"], flush=True)
            bn.free(), bp.free()
    for n, tl, ql in ((4096, 250, 150), (1024, 2400, 2000)):
        win, diag = window_batch(77, n, tl, ql, 0.05)
        b = eng.upload(PackedBatch(win))
        for cigar in (0, 1):
            opt = mw.opt_init(flag=cigar)
            sides = []
            for w in WIDTHS:
                band = np.array([(d - w, d + w) for d in diag], dtype=np.int32)
                sides.append((f"band_{w}", eng, b, lambda bb, o=opt, bd=band: bb.align_ends_pp(o, WINDOW, bd)))
            sides.append(("no_band", eng, b, lambda bb, o=opt: bb.align_ends(o, *WINDOW)))
            r = compare(f"{n} x ({ql} bp in {tl} bp) @ 5 %, {'CIGAR' if cigar else 'score'}", sides, a.aligns)
            out["report"].append(r)
            print(r["name"], r["ratio"], flush=True)
        b.free()
    lines = []
    for kind in ("gate", "report"):
        lines.append(f"{kind}: median ms [min, max] over {a.aligns} aligns, the sides alternating; ratios against the last side")
        for r in out[kind]:
            lines.append(f"  {r['name']}")
            for k in r["sides"]:
                v = r[k]
                lines.append(f"    {k:<10} {v['median_ms']:.3f} [{v['min_ms']:.3f}, {v['max_ms']:.3f}] ms   re-runs {v['n_retries']}   n_iter {v['n_iter_sum']}   "
                             f"bytes/pair {v['tb_bytes_per_pair']:.0f}   same s {v['same_s_as_last_side']}   stopped {v['n_stopped']}"
                             + (f"   ratio {r['ratio'][k]:.3f}" if k in r["ratio"] else ""))
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(a.out, "ends_band_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "ends_band_probe.txt"), "w") as f:
        f.write(text + "\n")
    for e in (eng, peng):
        if e:
            e.close()


if __name__ == "__main__":
    main()
