#!/usr/bin/env python3
"""Generate tests/golden/generic_pen.jsonl: a few pairs under every penalty set and mode of tests/generic_matrix.py (the generic kernel's table), run through
the REAL reference (oracle/_ref/libmwf_ref.so).  The oracle is only pinned to the reference for the sets and modes the golden files hold; this file adds the
ones those tests run under: thirteen sets and two more beyond ring depth 256, score-only, CIGAR, max_s, max_iter and low-memory steps of 97, nH, nH - 1, 1 and 2.

Run in the build container (needs the reference's sources to compile it); seconds in all:

    python tests/golden/make_golden_generic.py

Per set and mode: a 1 kb pair at 6 %, a 1.5 kb pair at 10 % with a long indel and a 600-base pair at 35 % (nearly unrelated: shrinks); the steps of 1 and 2 run
on a 257-base pair at 8 % and a 150-base pair at 15 % instead.  Inputs are generator specs (miniwfa_amd.synth.synth_pair), not sequences.  A vector stores
n_cigar and the SHA-256 of the CIGAR as little-endian uint32 words (len<<4|op) where the CIGAR has more than 64 words, else the words themselves.  Data only.
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

OUT = os.path.join(HERE, "generic_pen.jsonl")
# (tag, (seed, tl, p, n_long, long_max))
PAIRS = (("g1024", (730100, 1024, 0.06, 0, 0)), ("g1500-indel", (730200, 1500, 0.10, 1, 200)), ("g600-far", (730400, 600, 0.35, 0, 0)))
SMALL = (("g257", (730000, 257, 0.08, 0, 0)), ("g150", (730300, 150, 0.15, 0, 0)))


def main():
    import generic_matrix as gm
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    R = Reference()
    rows = []
    for tag, pen in gm.PEN.items():
        for mname, okw, which in gm.all_modes(tag):
            for name, spec in (SMALL if which == "small" else PAIRS):
                t, q = synth_pair(*spec)
                o = make_opt(**okw, **pen)
                rows.append(_row(f"{name}-{tag}-{mname}", spec, "exact", o, EXACT_KEYS, _expect(*R.align(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
