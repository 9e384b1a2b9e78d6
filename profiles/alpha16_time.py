"""What "alpha16" costs and buys: five batch shapes in which every pair has one run of ten N in the target and three single N in the query, each
uploaded and wrapped, score-only and with CIGAR, aligned under three settings in turn in one session:

    a16/0   "alpha_remap" 1, "alpha16" 0 on that batch — the baseline: what the library did before the tunable existed, from the same library
    a16/1   "alpha_remap" 1, "alpha16" 1
    twin    the N-free twin batch (every N replaced by A) under "alpha_remap" 1 — for orientation only: the 2-bit kernels on nearly the same relation

Per cell: the host clock around align -> results() (re-runs happen in results()), one warm-up then the median of nine, and kernel ms (mwf_gpu_get_stats: HIP events around
the align call's own launches, not the re-runs); the classify / copy kernels' own time (Engine.alpha_ms).  An uploaded batch is copied by its first align only, so every
repetition of an uploaded cell aligns a fresh upload (outside the clock, for every setting alike); a wrapped batch is classified and copied at every align.

The gate (1.15 x, the bar of DESIGN.md 4.6 (4)): a16/0 over a16/1 on the host clock — the 512 x 3 / x 4 group on the 10k and 2k shapes, the span group on 15k and 50k.
The read shape (150bp) must not get slower than "alpha_remap" 1 alone makes it: the tunable is not for read batches.

    python profiles/alpha16_time.py [--shapes 10k,2k,15k,50k,150bp] [--reps 9] [--modes score,cigar] [--paths uploaded,wrapped]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: its HIP runtime must be the one the process loads)

import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import PackedBatch, synth_pair  # noqa: E402

SHAPES = {"10k": (1024, 10000, 0.05), "15k": (512, 15000, 0.05), "50k": (1250, 50000, 0.03), "2k": (512, 2000, 0.05), "150bp": (40000, 150, 0.05)}


def with_n(t: bytes, q: bytes, seed: int):
    rng = np.random.default_rng(seed)
    a = int(rng.integers(0, max(1, len(t) - 10)))
    t2 = (t[:a] + b"N" * 10 + t[a + 10:])[:len(t)]
    q2 = bytearray(q)
    for p in rng.integers(0, len(q), 3):
        q2[int(p)] = ord("N")
    return t2, bytes(q2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10k,2k,15k,50k,150bp")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--modes", default="score,cigar")
    ap.add_argument("--paths", default="uploaded,wrapped")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"# alpha16_time: reps {a.reps} (+1 warm-up), median; libmwf_hip.so {os.path.getsize(mw.api._build.LIB)} bytes", flush=True)
    for shape in a.shapes.split(","):
        n, length, p = SHAPES[shape]
        t0 = time.perf_counter()
        plain = [synth_pair(434300 + i, length, p) for i in range(n)]
        withn = [with_n(t, q, 535300 + i) for i, (t, q) in enumerate(plain)]
        twin = [(t.replace(b"N", b"A"), q.replace(b"N", b"A")) for t, q in withn]
        pk = {"n": PackedBatch(withn), "twin": PackedBatch(twin)}
        print(f"\n## {n} x {length} @ {p:g}: {pk['n'].bases} bases (generated in {time.perf_counter() - t0:.1f} s)", flush=True)
        for path in a.paths.split(","):
            for mode in a.modes.split(","):
                opt = mw.opt_init(flag=mw.MWF_F_CIGAR if mode == "cigar" else 0)
                variants = (("a16/0", "n", 0), ("a16/1", "n", 1), ("twin", "twin", 0))
                engs = {}
                for name, _, a16 in variants:
                    engs[name] = mw.Engine(0)
                    engs[name].set("alpha_remap", 1)
                    engs[name].set("alpha16", a16)
                held = {name: engs[name].wrap_packed(pk[which], dev) for name, which, _ in variants} if path == "wrapped" else {}
                rec = {name: {"kernel": [], "host": [], "cls": [], "copy": [], "route": None} for name, _, _ in variants}
                for rep in range(a.reps + 1):
                    for name, which, _ in variants:   # the three settings in turn
                        eng = engs[name]
                        b = held[name] if path == "wrapped" else eng.upload(pk[which])
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        b.align(opt)
                        b.results()
                        host = (time.perf_counter() - t0) * 1e3
                        st = eng.stats()
                        ms = eng.alpha_ms()
                        if path == "uploaded":
                            b.free()
                        if rep == 0:
                            rec[name]["route"] = (st.kernel_kind, st.packed, st.block, st.grid, st.n_retries)
                            continue
                        r = rec[name]
                        r["kernel"].append(st.kernel_ms), r["host"].append(host), r["cls"].append(ms[0]), r["copy"].append(ms[1])
                med = {name: {k: statistics.median(v) for k, v in r.items() if k != "route"} for name, r in rec.items()}
                print(f"{shape} {path} {mode}:", flush=True)
                for name, _, _ in variants:
                    m = med[name]
                    print(f"   {name:6s} kernel {m['kernel']:9.3f} ms  host {m['host']:9.3f} ms  classify {m['cls']:7.4f} ms  copy {m['copy']:7.4f} ms"
                          f"  (kind, packed, block, grid, re-runs of the warm-up align) {rec[name]['route']}", flush=True)
                h0, h1, tw = med["a16/0"]["host"], med["a16/1"]["host"], med["twin"]["host"]
                print(f"   a16/0 over a16/1: host x{h0 / h1:.2f};  a16/1 over the twin: host x{h1 / tw:.2f} ({h1 - tw:+.3f} ms)", flush=True)
                for b in held.values():
                    b.free()
                for e in engs.values():
                    e.close()


if __name__ == "__main__":
    main()
