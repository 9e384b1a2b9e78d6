#!/usr/bin/env python3
"""Generate tests/golden/band_biased.jsonl: pairs of the length at which the packed band kernel leaves plain 16-bit offsets — target length + worst-case
penalty from 32767 on: its five- and six-slot copies of the 512-thread geometry on biased offsets, class 14 of the host's routing — under every set those
copies are built for beyond the defaults, run through the REAL reference (oracle/_ref/libmwf_ref.so).

Run in the build container (needs the reference's sources to compile it); a minute in all:

    python tests/golden/make_golden_band_biased.py

Per set: one 12 kb pair at 5 %, score-only and with CIGAR.  For (2,2) — main.c's -a preset — also a 7 kb pair (the short end: the first lengths past plain
offsets) and a 10 kb pair (the benchmark's shape).  Inputs are generator specs (miniwfa_amd.synth.synth_pair), not sequences.  A vector stores n_cigar and
the SHA-256 of the CIGAR as little-endian uint32 words (len<<4|op) where the CIGAR has more than 64 words, else the words themselves.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_long import cigar_sha256  # noqa: E402

OUT = os.path.join(HERE, "band_biased.jsonl")
PEN = {"a22": dict(x=4, o1=4, e1=2, o2=4, e2=2), "edit": dict(x=1, o1=0, e1=1, o2=0, e2=1), "e31": dict(x=4, o1=6, e1=3, o2=26, e2=1),
       "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2), "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1)}
EXACT_KEYS = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter")
# (seed, tl, p, n_long, long_max)
PAIR_12K = (810000, 12000, 0.05, 0, 0)
PAIR_7K = (811000, 7000, 0.05, 0, 0)
PAIR_10K = (812000, 10000, 0.05, 0, 0)


def _expect(s, n_iter, cig):
    e = {"s": s, "n_iter": n_iter, "n_cigar": None if cig is None else len(cig)}
    if cig is not None:
        if len(cig) > 64:
            e["cigar_sha256"] = cigar_sha256(cig)
        else:
            e["cigar"] = [int(w) for w in cig]
    return e


def _row(vid, spec, o, expect):
    from miniwfa_amd.synth import synth_pair
    seed, tl, p, n_long, long_max = spec
    _, q = synth_pair(*spec)
    return {"id": vid, "kind": "synth", "seed": seed, "tl": tl, "p": p, "n_long": n_long, "long_max": long_max, "ql": len(q), "entry": "exact",
            "opt": {k: int(getattr(o, k)) for k in EXACT_KEYS}, "expect": expect}


def main():
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    R = Reference()
    rows = []
    for tag, pen in PEN.items():
        for size, spec in (("12k", PAIR_12K),) + ((("7k", PAIR_7K), ("10k", PAIR_10K)) if tag == "a22" else ()):
            t, q = synth_pair(*spec)
            for mode, flag in (("score", 0), ("cigar", 1)):
                o = make_opt(flag=flag, **pen)
                rows.append(_row(f"biased{size}-{tag}-{mode}", spec, o, _expect(*R.align(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
