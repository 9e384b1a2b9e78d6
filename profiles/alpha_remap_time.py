"""What "alpha_remap" costs and buys: lower-case twins of four batch shapes, each uploaded and wrapped, score-only and with
CIGAR, aligned with the tunable at 0 and at 1 in turn, beside the upper-cased twin batch (the reference: the same kernels on the same relation).

Per cell: kernel ms (mwf_gpu_get_stats: HIP events around the align kernels) and the host clock around align -> results(), one warm-up then
the median of nine; the remap kernels' own time from HIP events around them (Engine.alpha_ms: classification, copy) and the bytes per second
that is.  An uploaded batch is remapped by its first align only, so every repetition of an uploaded cell aligns a fresh upload of the batch
(the upload is outside the clock, for every variant alike); a wrapped batch is classified and copied at every align, so it is wrapped once.

    python profiles/alpha_remap_time.py [--shapes 10k,15k,50k,150bp] [--reps 9] [--modes score,cigar] [--paths uploaded,wrapped]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402  (first: its HIP runtime must be the one the process loads)

import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import PackedBatch, synth_pair  # noqa: E402

SHAPES = {"10k": (1024, 10000, 0.05), "15k": (512, 15000, 0.05), "50k": (1250, 50000, 0.03), "150bp": (40000, 150, 0.05)}
HBM_PEAK = 8.0e12  # bytes per second, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10k,15k,50k,150bp")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--modes", default="score,cigar")
    ap.add_argument("--paths", default="uploaded,wrapped")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"# alpha_remap_time: reps {a.reps} (+1 warm-up), median; libmwf_hip.so {os.path.getsize(mw.api._build.LIB)} bytes", flush=True)
    for shape in a.shapes.split(","):
        n, length, p = SHAPES[shape]
        t0 = time.perf_counter()
        upper = [synth_pair(424200 + i, length, p) for i in range(n)]
        lower = [(t.lower(), q.lower()) for t, q in upper]
        pk = {"upper": PackedBatch(upper), "lower": PackedBatch(lower)}
        nbytes = pk["lower"].bases
        print(f"\n## {n} x {length} @ {p:g}: {nbytes} bases (generated in {time.perf_counter() - t0:.1f} s)", flush=True)
        for path in a.paths.split(","):
            for mode in a.modes.split(","):
                opt = mw.opt_init(flag=mw.MWF_F_CIGAR if mode == "cigar" else 0)
                variants = (("lower/0", "lower", 0), ("lower/1", "lower", 1), ("upper", "upper", 0))
                engs = {}
                for name, _, remap in variants:
                    engs[name] = mw.Engine(0)
                    engs[name].set("alpha_remap", remap)
                held = {name: engs[name].wrap_packed(pk[which], dev) for name, which, _ in variants} if path == "wrapped" else {}
                rec = {name: {"kernel": [], "host": [], "cls": [], "copy": [], "route": None} for name, _, _ in variants}
                for rep in range(a.reps + 1):
                    for name, which, remap in variants:   # 0 and 1 in turn, the twin beside them
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
                    print(f"   {name:8s} kernel {m['kernel']:9.3f} ms  host {m['host']:9.3f} ms  classify {m['cls']:7.4f} ms  copy {m['copy']:7.4f} ms"
                          f"  (kind, packed, block, grid, re-runs of the warm-up align) {rec[name]['route']}", flush=True)
                l0, l1, up = med["lower/0"], med["lower/1"], med["upper"]
                remap_ms = l1["cls"] + l1["copy"]
                # bytes the remap kernels move: the classification reads every base, the copy reads and writes every base
                moved = nbytes * ((1 if l1["cls"] > 0 else 0) + 2)
                rate = moved / (remap_ms * 1e-3) if remap_ms > 0 else 0.0
                print(f"   0 / 1: kernel x{l0['kernel'] / l1['kernel']:.2f}, host x{l0['host'] / l1['host']:.2f};  1 against the twin: kernel {l1['kernel'] - up['kernel']:+.3f} ms,"
                      f" host {l1['host'] - up['host']:+.3f} ms, remap kernels {remap_ms:.4f} ms = {rate / 1e9:.0f} GB/s ({100 * rate / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:g} TB/s)", flush=True)
                for b in held.values():
                    b.free()
                for e in engs.values():
                    e.close()


if __name__ == "__main__":
    main()
