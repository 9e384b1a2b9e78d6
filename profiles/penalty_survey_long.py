"""Long pairs under gap extensions of 3 and 4 — the sets the whole-device kernel is built for besides (2,1), (2,2), (1,1) — with the default set as the
yardstick in the same run: one 150 kb pair @ 3 % (score, CIGAR, low-memory step = 5000), 12 x 25 kb @ 3 % side by side, optionally the 5 Mb pair (default set).
Kernel time from mwf_gpu_get_stats (device events around the call's launches), one warm-up and `--reps` timed aligns per row: min / median / max.

Two builds are compared in ONE call by alternating them, a fresh process per build and round (a process loads one library):

    python profiles/penalty_survey_long.py                                    # the in-tree library
    python profiles/penalty_survey_long.py --libs before=/path/libmwf_hip.so after=miniwfa_amd/csrc/libmwf_hip.so --rounds 2 [--mhc]
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
MODES = [("score", dict(flag=0)), ("cigar", dict(flag=1)), ("lowmem 5000", dict(flag=1, step=5000))]


def rows(reps, mhc):
    import torch  # noqa: F401
    from miniwfa_amd import api as mw
    from miniwfa_amd.synth import PackedBatch, synth_pair
    shapes = [("1 x 150 kb @ 3 %", [synth_pair(4242, 150000, 0.03)], MODES), ("12 x 25 kb @ 3 %", [synth_pair(640030 + i, 25000, 0.03) for i in range(12)], MODES[:2])]
    if mhc:
        shapes.append(("1 x 5 Mb (MHC-like)", [synth_pair(2002, 5000000, 0.008, 3, 15000)], [MODES[2]]))
    for sname, pairs, modes in shapes:
        pk = PackedBatch(pairs)
        for pname, kw in (PEN[:1] if sname.startswith("1 x 5 Mb") else PEN):
            for mname, mkw in modes:
                eng = mw.Engine(0)
                b = eng.upload(pk)
                o = mw.opt_init(**kw, **mkw)
                ms, first = [], None
                for it in range(reps + 1):
                    b.align(o)
                    s, _, _ = b.results()
                    st = eng.stats()
                    if it:
                        ms.append(st.kernel_ms)
                    first = int(s[0])
                print(f"{sname:20s} {pname:22s} {mname:12s} kernel ms min {min(ms):9.3f} median {statistics.median(ms):9.3f} max {max(ms):9.3f}  "
                      f"(kind {st.kernel_kind}, two-pass {st.lowmem_two_pass}, {st.n_retries} re-run, s[0] {first})", flush=True)
                b.free()
                eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="*", default=[], help="label=path of the builds to alternate (default: the in-tree library)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mhc", action="store_true", help="also the 5 Mb pair in low-memory mode under the default set (minutes on a build that sends it to the generic kernel under other sets)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child or not a.libs:
        rows(a.reps, a.mhc)
        return
    for r in range(a.rounds):
        for spec in a.libs:
            label, path = spec.split("=", 1)
            print(f"== {label} (round {r + 1})", flush=True)
            env = dict(os.environ, MWF_HIP_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--mhc"] if a.mhc else [])
            rc = subprocess.run(cmd, env=env, timeout=900).returncode
            if rc != 0:  # a failed step ends the survey: nothing more is started on the device
                raise SystemExit(f"{label}: exit status {rc}")


if __name__ == "__main__":
    main()
