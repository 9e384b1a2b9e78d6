#!/usr/bin/env python3
"""Generate tests/golden/band_pen.jsonl: mid-size pairs — the packed band kernel's — under penalty sets with gap extensions of 3 and 4, run
through the REAL reference (oracle/_ref/libmwf_ref.so).

Run in the build container (needs the reference's sources to compile it); seconds in all:

    python tests/golden/make_golden_band_pen.py

Per set: one 10 kb pair at 5 % (score-only and with CIGAR) and one 3 kb pair at 3 % with two long indels.  For the asm5-like set
(4,6,3,26,1): mwf_wfa_chain and mwf_wfa_auto of six 5 kb records and one 30 kb record (a long indel or two each: gap fills between anchors).
Inputs are generator specs (miniwfa_amd.synth.synth_pair), not sequences.  A vector stores n_cigar and the SHA-256 of the CIGAR as
little-endian uint32 words (len<<4|op) where the CIGAR has more than 64 words, else the words themselves.  Data only.
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

OUT = os.path.join(HERE, "band_pen.jsonl")
# (the sets the band kernel is built for: (4,2) missed its speed gate)
PEN = {"e31": dict(x=4, o1=6, e1=3, o2=26, e2=1), "e32": dict(x=4, o1=4, e1=3, o2=24, e2=2), "e41": dict(x=4, o1=6, e1=4, o2=26, e2=1)}
EXACT_KEYS = ("flag", "x", "o1", "e1", "o2", "e2", "step", "max_s", "max_iter")
CHAIN_KEYS = EXACT_KEYS + ("max_occ", "kmer", "min_len")
# (seed, tl, p, n_long, long_max)
PAIR_10K = (710000, 10000, 0.05, 0, 0)
PAIR_3K = (711000, 3000, 0.03, 2, 300)
RECORDS = [(712000 + i, 5000, (0.01, 0.03, 0.05)[i % 3], 1 + i % 2, (150, 600, 1500)[i % 3]) for i in range(6)] + [(712100, 30000, 0.03, 2, 2000)]


def _expect(s, n_iter, cig):
    e = {"s": s, "n_iter": n_iter, "n_cigar": None if cig is None else len(cig)}
    if cig is not None:
        if len(cig) > 64:
            e["cigar_sha256"] = cigar_sha256(cig)
        else:
            e["cigar"] = [int(w) for w in cig]
    return e


def _row(vid, spec, entry, o, keys, expect):
    from miniwfa_amd.synth import synth_pair
    seed, tl, p, n_long, long_max = spec
    _, q = synth_pair(*spec)
    return {"id": vid, "kind": "synth", "seed": seed, "tl": tl, "p": p, "n_long": n_long, "long_max": long_max, "ql": len(q), "entry": entry,
            "opt": {k: int(getattr(o, k)) for k in keys}, "expect": expect}


def main():
    from oracle.pyoracle import Reference, make_opt
    from miniwfa_amd.synth import synth_pair
    R = Reference()
    rows = []
    for tag, pen in PEN.items():
        for vid, spec, flag in ((f"band10k-{tag}-score", PAIR_10K, 0), (f"band10k-{tag}-cigar", PAIR_10K, 1), (f"band3k-{tag}-cigar", PAIR_3K, 1)):
            t, q = synth_pair(*spec)
            o = make_opt(flag=flag, **pen)
            rows.append(_row(vid, spec, "exact", o, EXACT_KEYS, _expect(*R.align(t, q, o))))
    o = make_opt(flag=1, **PEN["e31"])
    for i, spec in enumerate(RECORDS):
        t, q = synth_pair(*spec)
        s, _, cig = R.chain(t, q, o)
        rows.append(_row(f"rec{i}-e31-chain", spec, "chain", o, CHAIN_KEYS, _expect(s, None, cig)))
        rows.append(_row(f"rec{i}-e31-auto", spec, "auto", o, CHAIN_KEYS, _expect(*R.auto(t, q, o))))
    with open(OUT, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(OUT, len(rows), "vectors")


if __name__ == "__main__":
    main()
