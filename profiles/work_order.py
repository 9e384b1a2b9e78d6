#!/usr/bin/env python3
"""Deal order of the band classes on the shared work counter (mwf_gpu_test_hook "work_order"): the four headline batches of bench.py
(1024 x 10 kb @ 5 %, base seeds 50000 + 10000 k, device-resident, score-only) timed in each mode, the modes interleaved round by round.

    0 length     longest first (the order before the per-pair sketch)
    1 predicted  (tl + ql) x d from the per-pair 8-mer sketch (the default)
    2 oracle     by the n_iter the previous align returned (the bound any prediction can reach)
    3 reversed   shortest first

Run with MWF_HIP_LIB=profiles/_timeline_libmwf_hip.so (profiles/build_band2_timeline.sh) for the per-pair timeline as well: each mode's last align
of every batch records when each pair was taken and done and on which CU; the drain is the time from the counter running dry (the last pair taken)
to the end of the launch, and the busy share is the fraction of the launch's workgroups still aligning over that time.

    python profiles/work_order.py [--rounds 3] [--reps 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {0: "length", 1: "predicted", 2: "oracle", 3: "reversed"}


def drain(tl: np.ndarray, grid: int) -> dict:
    """Timeline [pair][start, end, cu, workgroup] (100 MHz wall clock) -> launch span, drain and the busy share of the workgroups over the drain."""
    st, en = tl[:, 0].astype(np.float64), tl[:, 1].astype(np.float64)
    t0, dry, t1 = st.min(), st.max(), en.max()
    d = max(t1 - dry, 1.0)
    busy = np.clip(np.minimum(en, t1) - np.maximum(st, dry), 0, None).sum() / (grid * d)
    cus = len(np.unique(tl[:, 2]))
    # how many workgroups were still aligning when 90 % of the drain had passed
    late = int(((en > dry + 0.9 * d) & (st <= dry + 0.9 * d)).sum())
    return {"span_ms": (t1 - t0) / 1e5, "drain_ms": d / 1e5, "drain_frac": d / max(t1 - t0, 1.0), "busy_share_in_drain": float(busy),
            "cus_seen": cus, "workgroups": grid, "busy_at_90pct_of_drain": late}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="0,1,2,3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import miniwfa_amd as mw
    from miniwfa_amd.synth import synth_pair, PackedBatch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    eng = mw.Engine(0, stream.cuda_stream)
    timeline = "timeline" in os.environ.get("MWF_HIP_LIB", "")
    batches = []
    for k in range(4):
        pk = PackedBatch([synth_pair(50000 + 10000 * k + i, 10000, 0.05) for i in range(1024)])
        batches.append(eng.wrap_packed(pk, dev))
    opt = mw.opt_init()
    modes = [int(m) for m in args.modes.split(",")]
    tl_buf = torch.zeros((1024, 4), dtype=torch.int64, device=dev) if timeline else None
    kern = {m: [[] for _ in batches] for m in modes}
    ref = {}
    lines = {}
    for r in range(args.rounds):
        for m in modes:
            eng.set("work_order", m)  # (the oracle reads the previous align's n_iter: every batch has one from any mode)
            if timeline:  # (set before the warm-up: a hook re-plans, and the records then describe a timed align)
                eng.set("timeline", tl_buf.data_ptr())
            for k, b in enumerate(batches):
                for _ in range(2):  # the plan (and the sketch) and the wide class's measuring align
                    b.align(opt)
                    b.results()
                for _ in range(args.reps):
                    b.align(opt)
                    s, it, _ = b.results()
                    kern[m][k].append(eng.stats().kernel_ms)
                if k in ref:
                    assert np.array_equal(ref[k][0], s) and np.array_equal(ref[k][1], it), f"mode {m} changed the results of batch {k}"
                else:
                    ref[k] = (s.copy(), it.copy())
                if timeline and r == args.rounds - 1:  # (every align rewrites every pair's record: these are the last timed align's)
                    lines.setdefault(MODES[m], []).append(drain(tl_buf.cpu().numpy(), int(eng.stats().grid)))
            if timeline:
                eng.set("timeline", 0)
        print(f"round {r}: " + "  ".join(f"{MODES[m]} {np.mean([np.mean(x[-args.reps:]) for x in kern[m]]):.3f}" for m in modes), flush=True)
    res = {"batch": "4 x 1024 x 10 kb @ 5 % (bench.py headline), score-only", "rounds": args.rounds, "reps": args.reps, "modes": {}}
    base = np.mean([np.mean(x) for x in kern[modes[0]]])
    for m in modes:
        per_seed = [float(np.mean(x)) for x in kern[m]]
        res["modes"][MODES[m]] = {"kernel_ms_per_seed": per_seed, "kernel_ms_mean": float(np.mean(per_seed)),
                                  "min_per_seed": [float(np.min(x)) for x in kern[m]], "vs_first_mode": float(np.mean(per_seed) / base)}
        if MODES[m] in lines:
            res["modes"][MODES[m]]["timeline_per_seed"] = lines[MODES[m]]
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
