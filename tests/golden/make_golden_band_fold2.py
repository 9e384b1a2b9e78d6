#!/usr/bin/env python3
"""Generate tests/golden/band_fold2.jsonl: pairs of 0.9 - 2.6 kb with two long indels under the penalty sets on both sides of the second fold's routing rule
(tests/band_fold2_cases.py: PENS — o2 of 3, 2, 5, 9, and o2 + e2 at the fold's bound and one above), run through the REAL reference (oracle/_ref/libmwf_ref.so).

Run in the build container (needs the reference's sources to compile it); a second in all:

    python tests/golden/make_golden_band_fold2.py

Inputs are generator specs (miniwfa_amd.synth.synth_pair), not sequences; a vector stores s, n_iter, n_cigar and the CIGAR words (or their SHA-256 beyond 64 words).  Data only.
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

from make_golden_band_pen import _expect, _row, EXACT_KEYS  # noqa: E402

OUT = os.path.join(HERE, "band_fold2.jsonl")


def main():
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    import band_fold2_cases as fc
    R = Reference()
    rows = []
    for tag, pen in fc.PENS.items():
        for i, spec in enumerate(fc.GOLDEN_SPECS):
            t, q = synth_pair(*spec)
            o = make_opt(flag=1, **pen)
            rows.append(_row(f"fold2-{tag}-{i}", spec, "exact", o, EXACT_KEYS, _expect(*R.align(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
