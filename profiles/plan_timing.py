"""First align (plan not cached: a fresh batch every time) and repeated align of a 40 000 x 150 bp batch, host clock around align + results (ends in a stream
synchronise): host planning is on the hot path of read batches.  One JSON line; MWF_HIP_LIB=... selects another build of libmwf_hip.so (profiles/plan_refactor/:
the parent's library and this tree's, four processes each, alternating).

    python profiles/plan_timing.py LABEL"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import miniwfa_amd as mw
from miniwfa_amd.synth import PackedBatch, synth_pair

base = [synth_pair(70000 + i, 150, 0.05) for i in range(4000)]
pairs = base * 10
pb = PackedBatch(pairs)
eng = mw.Engine(0)
opt = mw.opt_init()
first, rep = [], []
for r in range(12):
    b = eng.upload(pb)
    t0 = time.perf_counter(); b.align(opt); b.results(); first.append((time.perf_counter() - t0) * 1e3)
    if r == 11:
        for k in range(60):
            t0 = time.perf_counter(); b.align(opt); b.results(); rep.append((time.perf_counter() - t0) * 1e3)
    b.free()
first = first[2:]   # (the first two: code objects, workspace)
rep = rep[10:]
out = dict(lib=sys.argv[1], n_pairs=len(pairs), first_align_ms=dict(median=float(np.median(first)), min=min(first), max=max(first), n=len(first)),
           repeated_align_ms=dict(median=float(np.median(rep)), min=min(rep), max=max(rep), n=len(rep)), n_retries=int(eng.stats().n_retries))
print(json.dumps(out))
