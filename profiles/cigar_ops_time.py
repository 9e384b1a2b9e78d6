"""Device-side summary and coordinate maps (mwf_cigar_ops.hip) against what a caller had to do before it could begin the same computation on
the host: results() + fetch_cigars() of the same aligned batch (the fixed-size records and the whole CIGAR pool to host memory).
Per shape: every round re-aligns the resident batch with CIGAR and waits for the device, then times (host clock, each ending in a device
synchronise) results() + fetch_cigars(), then summarize(), map(0) and map(1) from enqueue to synchronised; medians over the rounds after a
warm-up round.  Raw output of a run: profiles/cigar_ops/.
Usage (GPU box): python profiles/cigar_ops_time.py [--rounds 9]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from miniwfa_amd import api as mw
from miniwfa_amd.synth import PackedBatch, synth_pair

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()

SHAPES = (("1024 x 10 kb @ 5 %", lambda: [synth_pair(1000 + i, 10000, 0.05) for i in range(1024)]),
          ("40000 x 150 bp @ 5 %", lambda: [synth_pair(33000 + i, 150, 0.05) for i in range(40000)]),
          ("1 x 150 kb @ 3.5 %", lambda: [synth_pair(2001, 150000, 0.035)]))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for name, make in SHAPES:
    pairs = make()
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    b = eng.upload(pk)
    o = mw.opt_init(flag=mw.MWF_F_CIGAR)
    cols = {"fetch": [], "summarize": [], "map0": [], "map1": []}
    for rnd in range(args.rounds + 1):
        b.align(o)
        torch.cuda.synchronize()
        t_fetch = timed(lambda: (b.results(), b.fetch_cigars()))
        t_sum = timed(b.summarize)
        t_m0 = timed(lambda: b.map(0))
        t_m1 = timed(lambda: b.map(1))
        if rnd > 0:  # round 0 warms up: code objects, the library-owned buffers, the pinned staging buffer
            for k, v in zip(cols, (t_fetch, t_sum, t_m0, t_m1)):
                cols[k].append(v)
    s, it, nc = b.results()
    rec = b.summary()
    st = eng.stats()
    assert (rec["first_bad"] == -1).all() and (rec["score"] == s).all()
    ident = rec["n_eq"].sum() / (rec["n_eq"] + rec["n_x"] + rec["n_ins"] + rec["n_del"]).sum()
    med = {k: statistics.median(v) for k, v in cols.items()}
    print(f"{name}: results+fetch_cigars {med['fetch']:.3f} ms | summarize {med['summarize']:.3f} ms | map q->t {med['map0']:.3f} ms | map t->q {med['map1']:.3f} ms"
          f"   (min {min(cols['fetch']):.3f} / {min(cols['summarize']):.3f} / {min(cols['map0']):.3f} / {min(cols['map1']):.3f}; {args.rounds} rounds; "
          f"{int(nc.sum())} words, {pk.bases} bases, identity {ident:.4f}, re-runs {st.n_retries}, dev_bytes {st.dev_bytes})", flush=True)
    b.free()
    eng.close()
