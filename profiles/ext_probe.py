"""What the extension rule costs inside the ends-free kernel (mwf_ends.hip, EXT form).  Method of profiles/ends_probe.py: HIP-event time around the kernels
(GpuStats.kernel_ms), one process, warm-ups, the sides of a comparison alternating align by align, median [min, max].

  gate    align_ext(match 1, zdrop -1) against the PARENT commit's align_ends(0, free, 0, free) on a batch whose best cell is its end cell: the two kernels
          sweep the same penalties and cells, the difference is the reduction.  256 x 2 kb and 1024 x 300 bp at 5 %, score-only and with CIGAR.  A third
          side, this tree's own align_ends, shows that the unchanged kernel stays inside the parent's spread.  The parent is a built checkout of the parent
          commit, loaded beside this tree's library: --parent DIR (the directory that holds its miniwfa_amd/).  Without it the gate has two sides.
  report  a junk-tail batch, 1024 x (1 kb @ 5 % + 500 unrelated bases per sequence): align_ext(1, 100) against align_ends(0, free, 0, free) of the same
          batch; time and summed n_iter.

    python profiles/ext_probe.py [--parent DIR] [--aligns 20] [--out profiles/ext]

Writes ext_probe.json and ext_probe.txt (the tables of DESIGN.md) into --out."""
from __future__ import annotations

import argparse
import importlib.util
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
from miniwfa_amd.synth import PackedBatch, random_seq, synth_batch, synth_pair  # noqa: E402

FREE = mw.ENDS_FREE
EXTENSION = (0, FREE, 0, FREE)


def load_parent(path):
    """The parent checkout's package under another name, on its own library (which must be built: nothing is compiled here)."""
    pkg = os.path.join(path, "miniwfa_amd")
    lib = os.path.join(pkg, "csrc", "libmwf_hip.so")
    assert os.path.exists(lib), lib + " is not built"
    spec = importlib.util.spec_from_file_location("miniwfa_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["miniwfa_amd_parent"] = mod
    spec.loader.exec_module(mod)
    os.environ["MWF_HIP_LIB"] = lib
    try:
        mod.lib()
    finally:
        del os.environ["MWF_HIP_LIB"]
    return mod


def timed(side):
    """side = (label, module, engine, batch, opt, what): what is ("ends", allowances) or ("ext", (match, zdrop)) -> (ms, re-runs, sum of s, sum of n_iter)."""
    label, mod, eng, batch, opt, (kind, args) = side
    if kind == "ends":
        batch.align_ends(opt, *args)
    else:
        batch.align_ext(opt, *args)
    s, it, _ = batch.results()
    st = eng.stats()
    return float(st.kernel_ms), int(st.n_retries), int(np.asarray(s, dtype=np.int64).sum()), int(np.asarray(it, dtype=np.int64).sum())


def compare(name, sides, aligns, warmup=3):
    """Alternates the sides align by align; -> one record, ratios against the LAST side."""
    times = {s[0]: [] for s in sides}
    extra = {}
    for k in range(warmup + aligns):
        for side in sides:
            ms, retries, ssum, isum = timed(side)
            if k >= warmup:
                times[side[0]].append(ms)
            extra[side[0]] = dict(n_retries=retries, s_sum=ssum, n_iter_sum=isum)
    rec = dict(name=name, aligns=aligns, sides=[s[0] for s in sides])
    for label, v in times.items():
        rec[label] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), **extra[label])
    base = rec[sides[-1][0]]["median_ms"]
    rec["ratio"] = {s[0]: rec[s[0]]["median_ms"] / base for s in sides[:-1]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aligns", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ext"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    parent = load_parent(a.parent) if a.parent else None
    mw.lib()
    eng = mw.Engine(0)
    eng2 = mw.Engine(0)
    peng = parent.Engine(0) if parent else None
    out = dict(gate=[], report=[], parent=bool(parent))
    for n, tl in ((256, 2000), (1024, 300)):
        pairs = synth_batch(1234, n, tl, 0.05)
        pk = PackedBatch(pairs)
        bx, be = eng.upload(pk), eng2.upload(pk)
        bp = peng.upload(pk) if parent else None
        for cigar in (0, 1):
            opt = mw.opt_init(flag=cigar)
            sides = [("ext", mw, eng, bx, opt, ("ext", (1, -1))), ("ends", mw, eng2, be, opt, ("ends", EXTENSION))]
            if parent:
                sides.append(("parent_ends", parent, peng, bp, parent.opt_init(flag=cigar), ("ends", EXTENSION)))
            r = compare(f"{n} x {tl} bp @ 5 %, {'CIGAR' if cigar else 'score'}", sides, a.aligns)
            # the best cell is the end cell on (nearly) every pair: the two passes then sweep the same penalties and cells
            assert r["ext"]["n_iter_sum"] == r["ends"]["n_iter_sum"], r
            r["s_sum_ext_over_ends"] = r["ext"]["s_sum"] / r["ends"]["s_sum"]
            out["gate"].append(r)
        bx.free(), be.free()
        if bp:
            bp.free()
    n, good, junk = 1024, 1000, 500
    pairs = []
    for k in range(n):
        t, q = synth_pair(4321 + k, good, 0.05)
        pairs.append((t + random_seq(900000 + k, junk), q + random_seq(950000 + k, junk)))
    pk = PackedBatch(pairs)
    bx, be = eng.upload(pk), eng2.upload(pk)
    for cigar in (0, 1):
        opt = mw.opt_init(flag=cigar)
        sides = [("ext_z100", mw, eng, bx, opt, ("ext", (1, 100))), ("ends_extension", mw, eng2, be, opt, ("ends", EXTENSION))]
        out["report"].append(compare(f"{n} x ({good} bp @ 5 % + {junk} junk), {'CIGAR' if cigar else 'score'}", sides, a.aligns))
    bx.free(), be.free()
    lines = []
    for kind in ("gate", "report"):
        lines.append(f"{kind}: median ms [min, max] over {a.aligns} aligns, the sides alternating; ratios against the last side")
        for r in out[kind]:
            cols = [f"{k} {r[k]['median_ms']:.3f} [{r[k]['min_ms']:.3f}, {r[k]['max_ms']:.3f}] (re-runs {r[k]['n_retries']}, n_iter {r[k]['n_iter_sum']})" for k in r["sides"]]
            lines.append(f"  {r['name']:<44} " + "   ".join(cols) + "   ratio " + ", ".join(f"{k} {v:.3f}" for k, v in r["ratio"].items()))
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(a.out, "ext_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "ext_probe.txt"), "w") as f:
        f.write(text + "\n")
    for e in (eng, eng2, peng):
        if e:
            e.close()


if __name__ == "__main__":
    main()
