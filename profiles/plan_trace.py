"""Which kernel, geometry, copy form and grid every launch of a fixed list of small batches gets, and every re-route — the plan layer's behaviour as text, to
compare two builds of the library (profiles/plan_refactor/: the trace before and after the plan refactor must be identical).

    python profiles/plan_trace.py OUT.txt            (MWF_HIP_LIB=... selects another build of libmwf_hip.so)

One process, a few seconds of GPU work.  The batches make every size class launch at least once (lane with its device-side follow-up, lane-bytes, mid, the
four packed geometries and their byte-wise twins, wide aligned three times, biased, span, both 4-bit classes, generic forced and unpackable, low-mem, the
whole-device kernel alone / side by side / in low-memory mode) and exercise the re-routes band -> wide, band -> span, ST_ALPHABET -> byte-wise on a wrapped
batch and a traceback budget small enough for fewer, larger slots; an ends-free batch (score-only, with CIGAR, and with a budget that makes it run again on
fewer slots), the whole-device kernel's arena growth and a low-memory batch under a small budget.  (The ring16 -> 32-bit re-route needs 50 kb pairs and is
left out.)  An align that fails is traced with its message.
From the library's stderr under MWF_DEBUG=1 MWF_DEBUG_REROUTE=1: the `kernel kind` line of every launch and pair / tl / ql / status / kind / round of every
`re-route` line (not the class number); from the stats of every align: n_launches, n_retries, grid, block, kernel_kind, packed, lowmem_two_pass; and a hash of
the scores and n_iter."""
from __future__ import annotations

import hashlib
import os
import re
import sys
import tempfile

os.environ["MWF_DEBUG"] = "1"
os.environ["MWF_DEBUG_REROUTE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (its HIP runtime first, like tests/conftest.py: the wrapped batch lives in torch tensors)

import miniwfa_amd as mw  # noqa: E402
from miniwfa_amd.synth import PackedBatch, mutate, random_seq, synth_pair  # noqa: E402

NO_COOP = (("coop_min_len", 1 << 40),)
BANDS_ONLY = NO_COOP + (("lane_max_len", 0), ("mid_max_pairs", 0), ("div_aware", 0))


def with_n(pairs):
    """Every pair with a base outside A/C/G/T in both sequences."""
    return [(t[:len(t) // 3] + b"N" + t[len(t) // 3 + 1:], q[:len(q) // 2] + b"N" + q[len(q) // 2 + 1:]) for t, q in pairs]


def related8(seed: int, n: int, p: float):
    """A related pair over eight letters (alphabet class 3 under "alpha16")."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTRYKM", dtype=np.uint8)
    t = letters[rng.integers(0, 8, n)]
    q = t.copy()
    hit = rng.random(n) < p
    q[hit] = letters[rng.integers(0, 8, int(hit.sum()))]
    q = np.delete(q, np.nonzero(rng.random(n) < p / 4)[0])
    t, q = t.tobytes(), q.tobytes()
    assert 5 <= len(set(t + q)) <= 16
    return t, q


def reads(seed, n, length, p):
    return [synth_pair(seed + i, length, p) for i in range(n)]


def windows(seed, n, tl, ql, p):
    """Reads of ql bases, mutated at rate p, each somewhere in a window of tl bases (tests/test_ends_gpu.py window_pairs)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(n):
        t = random_seq(seed * 1000 + k, tl)
        a = int(rng.integers(0, tl - ql + 1))
        pairs.append((t, mutate(t[a:a + ql], seed * 1000 + 500 + k, p)))
    return pairs


def cases():
    """(name, tunables, pairs, opt keywords, aligns, wrapped[, ends-free allowances])"""
    geoms = reads(100, 12, 300, 0.05) + reads(200, 10, 1500, 0.05) + reads(300, 6, 3500, 0.05) + reads(400, 4, 6000, 0.05)
    yield "lane + follow-up", NO_COOP, reads(1000, 2000, 150, 0.05), {}, 2, False
    yield "lane and lane-bytes", NO_COOP, reads(4000, 1200, 150, 0.05) + with_n(reads(6000, 1100, 150, 0.05)), {}, 1, False
    yield "mid", NO_COOP, reads(8000, 6, 1000, 0.05), dict(flag=mw.MWF_F_CIGAR), 1, False
    yield "packed geometries", BANDS_ONLY, geoms, {}, 1, False
    yield "packed geometries, CIGAR", BANDS_ONLY, geoms, dict(flag=mw.MWF_F_CIGAR), 1, False
    yield "byte-wise twins", BANDS_ONLY, with_n(geoms), {}, 1, False
    # (CIGAR mode: a small score-only batch's results lie in pinned memory and its aligns need no reset kernel — the class then never measures)
    yield "wide, three aligns", BANDS_ONLY, reads(9000, 12, 6000, 0.05), dict(flag=mw.MWF_F_CIGAR), 3, False
    yield "biased", BANDS_ONLY, reads(9100, 4, 11000, 0.03), {}, 1, False
    yield "biased, -a preset", BANDS_ONLY, reads(9150, 4, 8000, 0.03), dict(o2=4, e2=2), 1, False
    yield "span", BANDS_ONLY, reads(9200, 3, 30000, 0.02), {}, 1, False
    nib = (("alpha_remap", 1), ("alpha16", 1))
    yield "4-bit classes", BANDS_ONLY + nib, [related8(9300 + i, 3000, 0.04) for i in range(4)] + [related8(9350 + i, 12000, 0.03) for i in range(2)], {}, 2, False
    yield "generic, forced", NO_COOP + (("force_kind", 0),), reads(9400, 8, 800, 0.05), {}, 1, False
    yield "generic, unpackable", BANDS_ONLY + (("band_span", 0),), reads(9500, 2, 12000, 0.03), {}, 1, False
    yield "low-mem", NO_COOP, reads(9600, 4, 600, 0.06) + reads(9650, 2, 10, 0.1), dict(flag=mw.MWF_F_CIGAR, step=50), 1, False
    yield "whole-device, alone", (), reads(9700, 1, 12000, 0.03), {}, 1, False
    yield "whole-device, side by side", (), reads(9750, 4, 12000, 0.03), {}, 1, False
    yield "whole-device, low-memory", (), reads(9800, 1, 12000, 0.03), dict(flag=mw.MWF_F_CIGAR, step=500), 1, False
    yield "re-route: band to wide", BANDS_ONLY, reads(9900, 8, 650, 0.25), {}, 1, False
    yield "re-route: band to span", BANDS_ONLY, reads(9950, 2, 9000, 0.20), {}, 1, False
    yield "re-route: ST_ALPHABET on a wrapped batch", BANDS_ONLY, with_n(reads(10000, 4, 1500, 0.05)), {}, 1, True
    yield "re-route: fewer, larger slots", NO_COOP + (("tb_budget_mb", 8),), reads(84000, 40, 1500, 0.1), dict(flag=mw.MWF_F_CIGAR), 1, False
    free_target = (mw.ENDS_FREE, mw.ENDS_FREE, 0, 0)
    yield "ends-free", (), windows(31, 8, 500, 300, 0.05), {}, 1, False, free_target
    yield "ends-free, CIGAR", (), windows(31, 8, 500, 300, 0.05), dict(flag=mw.MWF_F_CIGAR), 1, False, free_target
    # (tests/test_ends_gpu.py test_arena_rerun: unit penalties, allowances of the window's slack — eight slots of 128 KB, then one of 1 MB)
    yield ("ends-free, re-route: fewer, larger slots", (("tb_budget_mb", 1),), windows(59, 8, 2600, 2000, 0.15),
           dict(flag=mw.MWF_F_CIGAR, x=1, o1=1, e1=1, o2=1, e2=1), 1, False, (600, 600, 0, 0))
    # (tests/test_gpu_parity.py test_whole_device_traceback_arena_grows)
    small_arena = (("force_kind", 1), ("coop_tb_cap_mb", 1))
    yield "re-route: whole-device arena grows", small_arena, [synth_pair(88100, 6000, 0.15)], dict(flag=mw.MWF_F_CIGAR), 1, False
    yield "re-route: whole-device arena grows, low-memory", small_arena, [synth_pair(88100, 6000, 0.15)], dict(flag=mw.MWF_F_CIGAR, step=400), 1, False
    # (snapshots of the generic kernel's two-pass form: six slots overflow, one slot of 2 MB holds every pair, one of 1 MB does not — the align fails)
    for mb in (2, 1):
        yield "re-route: low-mem, fewer slots, %d MB" % mb, NO_COOP + (("tb_budget_mb", mb),), reads(9660, 6, 1500, 0.1), dict(flag=mw.MWF_F_CIGAR, step=50), 1, False


class Stderr:
    """The process's stderr (file descriptor 2: the library writes with fprintf) into a file while the block runs."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


REROUTE = re.compile(r"re-route: pair (\d+) \(tl (\d+) ql (\d+)\) status (\d+) kind (\d+) class -?\d+ flags -?\d+ n_iter word -?\d+ round (\d+)")


def trace_lines(text: str):
    for ln in text.splitlines():
        if "[libmwf_hip] kernel kind" in ln:
            yield "  " + ln.split("[libmwf_hip] ", 1)[1]
        m = REROUTE.search(ln)
        if m:
            yield "  re-route: pair %s tl %s ql %s status %s kind %s round %s" % m.groups()


def main(out_path: str):
    out = []
    for name, tun, pairs, opt_kw, aligns, wrapped, *ends in cases():
        eng = mw.Engine(0)
        for k, v in tun:
            eng.set(k, v)
        pb = PackedBatch(pairs)
        if wrapped:
            b = eng.wrap_packed(pb, torch.device("cuda:0"))
        else:
            b = eng.upload(pb)
        out.append("== %s: %d pairs, %s" % (name, len(pairs), " ".join("%s=%s" % kv for kv in sorted(opt_kw.items())) or "defaults"))
        for a in range(aligns):
            failed = None
            with Stderr() as err:
                try:
                    if ends:
                        b.align_ends(mw.opt_init(**opt_kw), *ends[0])
                    else:
                        b.align(mw.opt_init(**opt_kw))
                    s, it, nc = b.results()
                except RuntimeError as e:
                    failed = str(e)
            st = eng.stats()
            out.append(" align %d" % a)
            out.extend(trace_lines(err.text))
            if failed is not None:
                out.append("  failed: %s" % failed)
                continue
            out.append("  stats: n_launches %d n_retries %d grid %d block %d kernel_kind %d packed %d lowmem_two_pass %d" %
                       (st.n_launches, st.n_retries, st.grid, st.block, st.kernel_kind, st.packed, st.lowmem_two_pass))
            out.append("  results: %s" % hashlib.sha256(s.tobytes() + it.tobytes() + nc.tobytes()).hexdigest()[:16])
        b.free()
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("%d lines -> %s" % (len(out), out_path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "plan_trace.txt")
