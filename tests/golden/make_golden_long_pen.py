#!/usr/bin/env python3
"""Generate tests/golden/long_pairs_pen.jsonl: the single long pairs of make_golden_long.py (the C4-like 150 kb pair, the
MHC-like 5 Mb pair) under penalty sets with gap extensions of 3 and 4, run through the REAL reference
(oracle/_ref/libmwf_ref.so).

Run in the build container (needs the reference's sources to compile it); minutes of one core for each 5 Mb vector:

    python tests/golden/make_golden_long_pen.py               # every vector, one process per vector
    python tests/golden/make_golden_long_pen.py c4-e31-score  # a single vector (prints its line)

A vector stores n_cigar and the SHA-256 of the CIGAR as little-endian uint32 words (len<<4|op) instead of the string.
Every `step` vector is checked to really take snapshots (s >= step).  Data only.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_long import C4, MHC, cigar_sha256  # noqa: E402

OUT = os.path.join(HERE, "long_pairs_pen.jsonl")

# tag -> x, o1, e1, o2, e2: one set per gap-extension pair (3,1), (3,2), (4,1), (4,2); e31 is minimap2's asm5-like set
PEN = {"e31": dict(x=4, o1=6, e1=3, o2=26, e2=1), "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2),
       "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1), "e42": dict(x=2, o1=4, e1=4, o2=24, e2=2)}
MODES = {"score": dict(flag=0), "cigar": dict(flag=1), "lowmem": dict(flag=1, step=5000), "lowmem1000": dict(flag=1, step=1000)}
VECTORS = {f"c4-{p}-{m}": (*C4, dict(**PEN[p], **MODES[m])) for p in PEN for m in MODES}
VECTORS["mhc-e31-score"] = (*MHC, dict(**PEN["e31"], flag=0))
VECTORS["mhc-e31-lowmem"] = (*MHC, dict(**PEN["e31"], flag=1, step=5000))
# chain mode: a 100 kb pair (miniwfa_amd.synth.synth_diverged_block: seed, flank, block_t, block_q, p) whose middle — unrelated blocks just below the
# 10 kb from which the reference bridges instead of aligning (miniwfa.c:869) — is ONE long gap fill of 9500 x 9800 bases
CHAIN = (89400, 45000, 9500, 9800, 0.02)
CHAIN_VECTORS = {"chain-e31-cigar": ("chain", dict(**PEN["e31"], flag=1)), "chain-e31-score": ("chain", dict(**PEN["e31"], flag=0)),
                 "auto-e31-cigar": ("auto", dict(**PEN["e31"], flag=1))}
CHAIN_KEYS = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter", "max_occ", "kmer", "min_len")


def one_chain(name: str) -> dict:
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_diverged_block
    entry, kw = CHAIN_VECTORS[name]
    t, q = synth_diverged_block(*CHAIN)
    o = make_opt(**kw)
    R = Reference()
    s, n_iter, cig = (R.chain if entry == "chain" else R.auto)(t, q, o)
    return {"id": name, "kind": "diverged", "args": list(CHAIN), "tl": len(t), "ql": len(q), "entry": entry,
            "opt": {k: int(getattr(o, k)) for k in CHAIN_KEYS},
            "expect": {"s": s, "n_iter": n_iter if entry == "auto" else None, "n_cigar": None if cig is None else len(cig),
                       "cigar_sha256": None if cig is None else cigar_sha256(cig)}}


def one(name: str) -> dict:
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    seed, tl, p, n_long, long_max, kw = VECTORS[name]
    t, q = synth_pair(seed, tl, p, n_long, long_max)
    o = make_opt(**kw)
    R = Reference(arena=True)
    t0 = time.perf_counter()
    s, n_iter, cig = R.align(t, q, o)
    dt = time.perf_counter() - t0
    if o.step > 0 and s < o.step:
        raise SystemExit(f"{name}: s = {s} < step = {o.step}: the vector takes no snapshot")
    return {"id": name, "kind": "synth", "seed": seed, "tl": tl, "p": p, "n_long": n_long, "long_max": long_max, "ql": len(q),
            "entry": "exact",
            "opt": {k: getattr(o, k) for k in ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter")},
            "expect": {"s": s, "n_iter": n_iter, "n_cigar": None if cig is None else len(cig),
                       "cigar_sha256": None if cig is None else cigar_sha256(cig)},
            "reference_wall_s": round(dt, 2), "reference_host": "build container, 1 thread, gcc -O3 -msse4.2, one kalloc arena"}


def main():
    if len(sys.argv) > 1:
        print(json.dumps((one_chain if sys.argv[1] in CHAIN_VECTORS else one)(sys.argv[1]), separators=(",", ":")))
        return
    rows = []
    names = sorted(list(VECTORS) + list(CHAIN_VECTORS), key=lambda n: not n.startswith("mhc"))  # the 5 Mb vectors first: they run beside everything else
    procs = {}
    for n in names:
        procs[n] = subprocess.Popen([sys.executable, os.path.abspath(__file__), n], stdout=subprocess.PIPE, text=True)
        while sum(p.poll() is None for p in procs.values()) >= 6:
            time.sleep(0.2)
    for n in list(VECTORS) + list(CHAIN_VECTORS):
        out, _ = procs[n].communicate()
        if procs[n].returncode != 0:
            raise SystemExit(f"{n} failed")
        rows.append(out.strip().splitlines()[-1])
        print(rows[-1], flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(rows) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
