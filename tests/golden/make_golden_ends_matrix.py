#!/usr/bin/env python3
"""Generate tests/golden/ends_matrix.jsonl: the answers of the two restatements (tests/ends_ref.py wfa_ends, tests/ext_ref.py wfa_ext, with the shrink) for every
run of tests/ends_matrix.py — per form, workgroup size, penalty set and allowances or (A, Z) one line with [s, n_iter, te, qe] (EXT: and V, s_stop, why, F) of
every pair of the run's batch, and the two batches of the persistent-loop test.  Numpy only, under a minute:

    python tests/golden/make_golden_ends_matrix.py

The inputs are the table's own generators; the file holds no sequences and no answer of the library.  tests/test_ends_matrix_cpu.py recomputes every line and
checks the restatements against the oracle and the DP.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import ends_matrix as em
    rows = [dict(run=key, want=em.restated(pairs, pen, ext, cfg)) for key, pairs, pen, ext, cfg in em.fixture_runs()]
    with open(em.GOLDEN, "w") as f:
        for r in rows:
            f.write(json.dumps(r, separators=(",", ":")) + "\n")
    print(em.GOLDEN, len(rows), "runs,", sum(len(r["want"]) for r in rows), "answers")


if __name__ == "__main__":
    main()
