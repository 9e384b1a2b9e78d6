"""Device-side alignment text (mwf_cigar_text.hip) against what a caller has to do without it: results() + fetch_cigars() of the same aligned
batch, then mwf_cigar_text (the host twin) over all pairs on one host thread.
Per shape: every round re-aligns the resident batch with CIGAR and waits for the device, then times (host clock) results() + fetch_cigars(), then
per kind the host loop — mwf_gpu_batch_cigar (a memcpy out of the fetched pool) + mwf_cigar_text per pair into one preallocated buffer — and per
kind Batch.text(kind) from enqueue to device-synchronised (sizing launch, scan, the wait for the total, the writing launch).  Medians over the
rounds after a warm-up round.  The host loop is driven through ctypes: its per-pair call overhead is measured on its own (the same loop with
kind 6, which returns at once: two ctypes calls and the memcpy per pair) and printed beside it — a C caller pays about the difference.  The
texts are compared once per shape and kind after the timing (device text == host text, byte for byte).  Raw output of a run: profiles/cigar_text/.
Usage (GPU box): python profiles/cigar_text_time.py [--rounds 9]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from miniwfa_amd import api as mw
from miniwfa_amd.synth import PackedBatch, synth_pair

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()

SHAPES = (("1024 x 10 kb @ 5 %", lambda: [synth_pair(1000 + i, 10000, 0.05) for i in range(1024)]),
          ("40000 x 150 bp @ 5 %", lambda: [synth_pair(33000 + i, 150, 0.05) for i in range(40000)]),
          ("1 x 150 kb @ 3.5 %", lambda: [synth_pair(2001, 150000, 0.035)]))
KIND_NAMES = ("cigar", "sam", "cs", "md", "row_t", "row_q")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


L = mw.lib()
for name, make in SHAPES:
    pairs = make()
    pk = PackedBatch(pairs)
    eng = mw.Engine(0)
    b = eng.upload(pk)
    o = mw.opt_init(flag=mw.MWF_F_CIGAR)
    n = len(pairs)
    lens = [(len(t), len(q)) for t, q in pairs]
    cap = 3 * max(tl + ql for tl, ql in lens) + 64          # (no text is longer than three bytes per base plus the last number)
    dst = C.create_string_buffer(cap)
    nc = np.zeros(n, dtype=np.int32)
    wbuf = np.zeros(1, dtype=np.uint32)
    host_out = [None] * len(KIND_NAMES)

    def host_loop(kind, keep=False):
        """What a caller's loop does after fetch_cigars(): the words of pair i (a memcpy), their text."""
        out = []
        wp, eh, bh, text, cigar = wbuf.ctypes.data, eng.h, b.h, L.mwf_cigar_text, L.mwf_gpu_batch_cigar
        for i in range(n):
            m = int(nc[i])
            cigar(eh, bh, i, wp, m)
            r = text(kind, m, wp, lens[i][0], pairs[i][0], lens[i][1], pairs[i][1], dst, cap)
            if keep:
                out.append(dst.raw[:r])
        if keep:
            host_out[kind] = out

    cols = {"fetch": [], "overhead": []}
    cols.update({f"host_{k}": [] for k in KIND_NAMES})
    cols.update({f"dev_{k}": [] for k in KIND_NAMES})
    for rnd in range(args.rounds + 1):
        b.align(o)
        torch.cuda.synchronize()

        def fetch():
            global nc
            nc = b.results()[2]
            b.fetch_cigars()

        row = {"fetch": timed(fetch)}
        if wbuf.size < int(nc.max()):
            wbuf = np.zeros(int(nc.max()), dtype=np.uint32)
        row["overhead"] = timed(lambda: host_loop(mw.MWF_TXT_KINDS))
        for k, kn in enumerate(KIND_NAMES):
            row[f"host_{kn}"] = timed(lambda: host_loop(k))
        for k, kn in enumerate(KIND_NAMES):
            row[f"dev_{kn}"] = timed(lambda: b.text(k))
        if rnd > 0:  # round 0 warms up: code objects, the library-owned buffers, the pinned staging buffer
            for key, v in row.items():
                cols[key].append(v)
    st = eng.stats()
    total = []
    for k in range(len(KIND_NAMES)):
        host_loop(k, keep=True)
        got = b.texts(k)
        assert got == host_out[k], KIND_NAMES[k]
        total.append(sum(len(x) for x in got))
    med = {k: statistics.median(v) for k, v in cols.items()}
    print(f"{name}: results+fetch_cigars {med['fetch']:.3f} ms; host loop call overhead {med['overhead']:.3f} ms; {args.rounds} rounds; "
          f"{int(nc.sum())} words, {pk.bases} bases, dev_bytes {st.dev_bytes}", flush=True)
    for k, kn in enumerate(KIND_NAMES):
        print(f"    {kn:6s} {total[k]:>10d} bytes | host twin loop {med['host_' + kn]:9.3f} ms (min {min(cols['host_' + kn]):9.3f}) | "
              f"caller today = fetch + loop {med['fetch'] + med['host_' + kn]:9.3f} ms | device text() {med['dev_' + kn]:8.3f} ms (min {min(cols['dev_' + kn]):8.3f}) | "
              f"ratio {(med['fetch'] + med['host_' + kn]) / med['dev_' + kn]:7.1f}x, without the call overhead {(med['fetch'] + max(0.0, med['host_' + kn] - med['overhead'])) / med['dev_' + kn]:7.1f}x", flush=True)
    b.free()
    eng.close()
