#!/usr/bin/env python3
"""Generate tests/golden/sys_pen.jsonl: pairs of the sizes tests/sys_matrix.py runs the whole-device kernel on, under every penalty set of that table (PEN and
PEN_BEYOND), run through the REAL reference (oracle/_ref/libmwf_ref.so).  The oracle is only pinned to the reference for the sets the golden files hold; this
file adds the sets those tests run under — rings of 256 and 257 rows, rings whose depth comes from x, opens of 0 among them.

Run in the build container (needs the reference's sources to compile it); seconds in all:

    python tests/golden/make_golden_sys.py

Per set: a 300 bp pair at 5 % (score-only), a 1.5 kb pair at 8 % — past the first band shrink under most sets — with CIGAR and in the low-memory mode
(step 97, the table's), and a 3 kb pair at 3 % with two long indels in the low-memory mode.  Inputs are generator specs (miniwfa_amd.synth.synth_pair), not
sequences.  A vector stores n_cigar and the SHA-256 of the CIGAR as little-endian uint32 words (len<<4|op) where the CIGAR has more than 64 words, else the
words themselves.  Data only.
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

OUT = os.path.join(HERE, "sys_pen.jsonl")
# (tag, (seed, tl, p, n_long, long_max), flag, step)
PAIRS = (("sys300-score", (730000, 300, 0.05, 0, 0), 0, 0), ("sys1500-cigar", (730100, 1500, 0.08, 0, 0), 1, 0),
         ("sys1500-step", (730100, 1500, 0.08, 0, 0), 1, 97), ("sys3000-indels-step", (730200, 3000, 0.03, 2, 300), 1, 97))


def main():
    import sys_matrix as sm
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    R = Reference()
    rows = []
    for tag, pen in list(sm.PEN.items()) + list(sm.PEN_BEYOND.items()):
        for name, spec, flag, step in PAIRS:
            t, q = synth_pair(*spec)
            o = make_opt(flag=flag, step=step, **pen)
            rows.append(_row(f"{name}-{tag}", spec, "exact", o, EXACT_KEYS, _expect(*R.align(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
