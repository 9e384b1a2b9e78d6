"""Per-call time of the drop-in mwf_wfa_exact (host strings in, result out: one kernel launch per call) on pairs the packed band kernel takes — where a
microsecond of host dispatch would show.  Run from the root of the tree to be measured; prints one JSON line.

  python profiles/band_units_call_latency.py [LABEL]

Per length (2 kb, 10 kb; 5 % divergence, score-only, default penalties): three warm-up calls, then 200 timed one by one; the median and the minimum in microseconds."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import synth_pair  # noqa: E402

out = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "metric": "mwf_wfa_exact per call, score-only, us"}
for tl in (2000, 10000):
    t, q = synth_pair(123, tl, 0.05)
    o = mw.opt_init()
    for _ in range(3):
        mw.wfa_exact(t, q, o)
    times = []
    for _ in range(200):
        t0 = time.perf_counter()
        mw.wfa_exact(t, q, o)
        times.append((time.perf_counter() - t0) * 1e6)
    times.sort()
    out[f"{tl}bp_median_us"] = round(times[len(times) // 2], 2)
    out[f"{tl}bp_min_us"] = round(times[0], 2)
print(json.dumps(out))
