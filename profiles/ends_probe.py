"""What the ends-free kernel (mwf_ends.hip) costs.  Two measurements, HIP-event time around the kernels (GpuStats.kernel_ms), one process, the two sides of
a comparison alternating align by align after a warm-up:

  gate    ends-free with four zero allowances against the generic kernel's one-column-per-lane form (hooks force_kind 0, scalar_generic 1, ring16 0) on
          the same batch: the same loads and stores per cell plus the end test.  256 x 2 kb and 1024 x 300 bp at 5 %, score-only and with CIGAR.
  report  read-in-window batches — 4096 x (150 bp in 250 bp), 1024 x (2 kb in 2.4 kb), allowances (free, free, 0, 0) — next to the plain align of the
          same reads against their true intervals under the default routing.

    python profiles/ends_probe.py [--aligns 20] [--out profiles/ends]

Writes ends_probe.json and ends_probe.txt (the tables of DESIGN.md) into --out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (its HIP runtime first, as tests/conftest.py)
except ImportError:
    pass

import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import PackedBatch, mutate, random_seq, synth_batch  # noqa: E402

FREE = mw.ENDS_FREE


def window_batch(seed, n, tl, ql, p):
    """n (window, read) pairs and the same reads against the interval they were drawn from."""
    rng = np.random.default_rng(seed)
    win, true = [], []
    for k in range(n):
        t = random_seq(seed * 100000 + k, tl)
        a = int(rng.integers(0, tl - ql + 1))
        q = mutate(t[a:a + ql], seed * 100000 + 50000 + k, p)
        win.append((t, q))
        true.append((t[a:a + ql], q))
    return win, true


def timed(eng, batch, opt, ends):
    if ends is None:
        batch.align(opt)
    else:
        batch.align_ends(opt, *ends)
    s, _, _ = batch.results()
    st = eng.stats()
    return float(st.kernel_ms), int(st.n_retries), int(np.asarray(s, dtype=np.int64).sum())


def compare(name, side_a, side_b, aligns, warmup=3):
    """side = (label, engine, batch, opt, ends).  Alternates a, b, a, b ...; -> one record."""
    times = {side_a[0]: [], side_b[0]: []}
    extra = {}
    for k in range(warmup + aligns):
        for label, eng, batch, opt, ends in (side_a, side_b):
            ms, retries, ssum = timed(eng, batch, opt, ends)
            if k >= warmup:
                times[label].append(ms)
            extra[label] = dict(n_retries=retries, s_sum=ssum)
    rec = dict(name=name, aligns=aligns)
    for label, v in times.items():
        rec[label] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), **extra[label])
    rec["ratio"] = rec[side_a[0]]["median_ms"] / rec[side_b[0]]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aligns", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ends"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    new = mw.Engine(0)
    old = mw.Engine(0)
    for k, v in (("force_kind", 0), ("scalar_generic", 1), ("ring16", 0)):
        old.set(k, v)
    dflt = mw.Engine(0)
    out = dict(gate=[], report=[])
    lines = []
    for n, tl in ((256, 2000), (1024, 300)):
        pk = PackedBatch(synth_batch(1234, n, tl, 0.05))
        bn, bo = new.upload(pk), old.upload(pk)
        for cigar in (0, 1):
            opt = mw.opt_init(flag=cigar)
            r = compare(f"{n} x {tl} bp @ 5 %, {'CIGAR' if cigar else 'score'}", ("ends", new, bn, opt, (0, 0, 0, 0)), ("generic_scalar", old, bo, opt, None), a.aligns)
            assert r["ends"]["s_sum"] == r["generic_scalar"]["s_sum"], r
            out["gate"].append(r)
        bn.free(), bo.free()
    for n, tl, ql in ((4096, 250, 150), (1024, 2400, 2000)):
        win, true = window_batch(77, n, tl, ql, 0.05)
        bw, bt = new.upload(PackedBatch(win)), dflt.upload(PackedBatch(true))
        for cigar in (0, 1):
            opt = mw.opt_init(flag=cigar)
            r = compare(f"{n} x ({ql} bp in {tl} bp) @ 5 %, {'CIGAR' if cigar else 'score'}", ("ends_window", new, bw, opt, (FREE, FREE, 0, 0)), ("plain_true_interval", dflt, bt, opt, None), a.aligns)
            out["report"].append(r)
        bw.free(), bt.free()
    for kind in ("gate", "report"):
        lines.append(f"{kind}: median ms [min, max] over {a.aligns} aligns, the two sides alternating")
        for r in out[kind]:
            (la, ra), (lb, rb) = [(k, v) for k, v in r.items() if isinstance(v, dict)]
            lines.append(f"  {r['name']:<44} {la} {ra['median_ms']:.3f} [{ra['min_ms']:.3f}, {ra['max_ms']:.3f}] (re-runs {ra['n_retries']})   "
                         f"{lb} {rb['median_ms']:.3f} [{rb['min_ms']:.3f}, {rb['max_ms']:.3f}] (re-runs {rb['n_retries']})   ratio {r['ratio']:.2f}")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(a.out, "ends_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "ends_probe.txt"), "w") as f:
        f.write(text + "\n")
    for e in (new, old, dflt):
        e.close()


if __name__ == "__main__":
    main()
