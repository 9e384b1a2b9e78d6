#!/usr/bin/env python3
"""Generate tests/golden/lane_mid_pen.jsonl: read-sized and mid-size pairs — the lane kernel's and the mid kernel's — under every penalty set of
tests/lane_mid_matrix.py (PEN, PEN_BEYOND, EDGE_PEN), run through the REAL reference (oracle/_ref/libmwf_ref.so).  The oracle is only pinned to the reference
for the sets the golden files hold; this file adds the sets those tests run under.

Run in the build container (needs the reference's sources to compile it); seconds in all:

    python tests/golden/make_golden_lane_mid.py

Per set: a 150 bp read at 5 % (CIGAR), a 300 bp read at 3 % (score-only), a 1.2 kb pair at 6 % (CIGAR) and a 1.5 kb pair at 12 % — past the first band
shrink, under most sets past several — (CIGAR).  Inputs are generator specs (miniwfa_amd.synth.synth_pair), not sequences.  A vector stores n_cigar and the
SHA-256 of the CIGAR as little-endian uint32 words (len<<4|op) where the CIGAR has more than 64 words, else the words themselves.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_band_pen import EXACT_KEYS, _expect, _row  # noqa: E402

OUT = os.path.join(HERE, "lane_mid_pen.jsonl")
# (tag, (seed, tl, p, n_long, long_max), flag)
PAIRS = (("lane150-cigar", (720000, 150, 0.05, 0, 0), 1), ("lane300-score", (720100, 300, 0.03, 0, 0), 0),
         ("mid1200-cigar", (720200, 1200, 0.06, 0, 0), 1), ("mid1500-shrunk-cigar", (720300, 1500, 0.12, 0, 0), 1))


def main():
    import lane_mid_matrix as lm
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    R = Reference()
    rows = []
    for tag, pen in list(lm.PEN.items()) + list(lm.PEN_BEYOND.items()) + list(lm.EDGE_PEN.items()):
        for name, spec, flag in PAIRS:
            t, q = synth_pair(*spec)
            o = make_opt(flag=flag, **pen)
            rows.append(_row(f"{name}-{tag}", spec, "exact", o, EXACT_KEYS, _expect(*R.align(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
