"""The gates of the 512-thread geometry's copies on biased offsets (class 14) for the sets beyond (2,1): batches whose pairs plain 16-bit offsets cannot be promised
to hold — 1024 x 10 kb @ 5 % under (2,2) and (3,2), 512 x 15 kb @ 5 % under (1,1), (3,1) and (4,1) —, score-only and with CIGAR, and the rows that must not
move: the default set on 1024 x 10 kb, (2,1) on 512 x 15 kb (the existing class 14), 20 000 x 150 bp reads.  Kernel time from mwf_gpu_get_stats, one warm-up and
`--reps` timed aligns per row: min / median / max, with what the last align launched.

Two builds are compared in ONE call by alternating them, a fresh process per build and round (a process loads one library):

    python profiles/penalty_survey_band_biased.py --libs before=/path/libmwf_hip.so after=miniwfa_amd/csrc/libmwf_hip.so --rounds 2
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A22 = ("-a 4,4,2,4,2", dict(x=4, o1=4, e1=2, o2=4, e2=2))
E32 = ("4,4,3,24,2", dict(x=4, o1=4, e1=3, o2=24, e2=2))
EDIT = ("-e 1,0,1,0,1", dict(x=1, o1=0, e1=1, o2=0, e2=1))
E31 = ("asm5-like 4,6,3,26,1", dict(x=4, o1=6, e1=3, o2=26, e2=1))
E41 = ("4,6,4,26,1", dict(x=4, o1=6, e1=4, o2=26, e2=1))
DEFAULT = ("default 4,4,2,15,1", dict())
MODES = [("score", dict(flag=0)), ("cigar", dict(flag=1))]


def rows(reps, only, pens_only=()):
    import torch  # noqa: F401
    from miniwfa_amd import api as mw
    from miniwfa_amd.synth import PackedBatch, synth_pair
    shapes = [("1024 x 10 kb @ 5 %", lambda: [synth_pair(50000 + i, 10000, 0.05) for i in range(1024)], [A22, E32, DEFAULT], MODES),
              ("512 x 15 kb @ 5 %", lambda: [synth_pair(60000 + i, 15000, 0.05) for i in range(512)], [EDIT, E31, E41, DEFAULT], MODES),
              ("20000 x 150 bp @ 5 %", lambda: [synth_pair(7000 + i, 150, 0.05) for i in range(20000)], [DEFAULT], MODES[:1])]
    for sname, make, pens, modes in shapes:
        if only and not any(sname.startswith(o) for o in only):
            continue
        pk = PackedBatch(make())
        for pname, kw in pens:
            if pens_only and not any(pname.startswith(o) for o in pens_only):
                continue
            for mname, mkw in modes:
                eng = mw.Engine(0)
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
    ap.add_argument("--only", nargs="*", default=[], help="shapes to run, by the start of their name (e.g. 1024)")
    ap.add_argument("--pens", nargs="*", default=[], help="penalty sets to run, by the start of their name (e.g. asm5)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child or not a.libs:
        rows(a.reps, a.only, a.pens)
        return
    for r in range(a.rounds):
        for spec in a.libs:
            label, path = spec.split("=", 1)
            print(f"== {label} (round {r + 1})", flush=True)
            env = dict(os.environ, MWF_HIP_LIB=os.path.abspath(path))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--only"] + a.only if a.only else []) + (["--pens"] + a.pens if a.pens else [])
            rc = subprocess.run(cmd, env=env, timeout=600).returncode
            if rc != 0:  # a failed step ends the survey: nothing more is started on the device
                raise SystemExit(f"{label}: exit status {rc}")


if __name__ == "__main__":
    main()
