"""Batches of mid-size pairs under gap extensions of 3 and 4 — the sets the packed band kernel is built for besides (2,1), (2,2), (1,1) — with the default set
as the yardstick in the same run: 1024 x 10 kb @ 5 % (score, CIGAR), 512 x 2 kb @ 5 %, 20 000 x 150 bp @ 5 % and, with --span, 1250 x 50 kb @ 3 % (score).
Kernel time from mwf_gpu_get_stats (device events around the call's launches), one warm-up and `--reps` timed aligns per row: min / median / max.

Two builds are compared in ONE call by alternating them, a fresh process per build and round (a process loads one library):

    python profiles/penalty_survey_band.py                                    # the in-tree library
    python profiles/penalty_survey_band.py --libs before=/path/libmwf_hip.so after=miniwfa_amd/csrc/libmwf_hip.so --rounds 2 [--span] [--set work_order=0]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEN = [("default 4,4,2,15,1", dict()), ("asm5-like 4,6,3,26,1", dict(x=4, o1=6, e1=3, o2=26, e2=1)), ("4,4,3,24,2", dict(x=4, o1=4, e1=3, o2=24, e2=2)),
       ("4,6,4,26,1", dict(x=4, o1=6, e1=4, o2=26, e2=1)), ("2,4,4,24,2", dict(x=2, o1=4, e1=4, o2=24, e2=2))]
MODES = [("score", dict(flag=0)), ("cigar", dict(flag=1))]


def rows(reps, span, only, tun):
    import torch  # noqa: F401
    from miniwfa_amd import api as mw
    from miniwfa_amd.synth import PackedBatch, synth_pair
    shapes = [("1024 x 10 kb @ 5 %", lambda: [synth_pair(50000 + i, 10000, 0.05) for i in range(1024)], MODES),
              ("512 x 2 kb @ 5 %", lambda: [synth_pair(100 + i, 2000, 0.05) for i in range(512)], MODES),
              ("20000 x 150 bp @ 5 %", lambda: [synth_pair(7000 + i, 150, 0.05) for i in range(20000)], MODES[:1])]
    if span:
        shapes.append(("1250 x 50 kb @ 3 %", lambda: [synth_pair(90000 + i, 50000, 0.03) for i in range(1250)], MODES[:1]))
    for sname, make, modes in shapes:
        if only and not any(sname.startswith(o) for o in only):
            continue
        pk = PackedBatch(make())
        for pname, kw in PEN:
            for mname, mkw in modes:
                eng = mw.Engine(0)
                for k, v in tun:
                    eng.set(k, v)
                b = eng.upload(pk)
                o = mw.opt_init(**kw, **mkw)
                ms = []
                for it in range(reps + 1):
                    b.align(o)
                    s, _, _ = b.results()
                    st = eng.stats()
                    if it:
                        ms.append(st.kernel_ms)
                print(f"{sname:22s} {pname:22s} {mname:6s} kernel ms min {min(ms):9.3f} median {statistics.median(ms):9.3f} max {max(ms):9.3f}  "
                      f"(kind {st.kernel_kind} block {st.block} packed {st.packed}, {st.n_retries} re-run, {st.n_launches} launches, sum s {int(s.sum())})", flush=True)
                b.free()
                eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="*", default=[], help="label=path of the builds to alternate (default: the in-tree library)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--span", action="store_true", help="also 1250 x 50 kb @ 3 % (the span geometry; a few hundred ms per align on a build that sends it to the generic kernel)")
    ap.add_argument("--only", nargs="*", default=[], help="shapes to run, by the start of their name (e.g. 1024)")
    ap.add_argument("--set", nargs="*", default=[], help="engine tunables name=value (e.g. work_order=0)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    tun = [(kv.split("=")[0], int(kv.split("=")[1])) for kv in a.set]
    if a.child or not a.libs:
        rows(a.reps, a.span, a.only, tun)
        return
    for r in range(a.rounds):
        for spec in a.libs:
            label, path = spec.split("=", 1)
            print(f"== {label} (round {r + 1})", flush=True)
            env = dict(os.environ, MWF_HIP_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--span"] if a.span else []) + (["--only"] + a.only if a.only else []) + (["--set"] + a.set if a.set else [])
            rc = subprocess.run(cmd, env=env, timeout=900).returncode
            if rc != 0:  # a failed step ends the survey: nothing more is started on the device
                raise SystemExit(f"{label}: exit status {rc}")


if __name__ == "__main__":
    main()
