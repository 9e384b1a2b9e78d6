"""bench.py's N > 1 start-up on CPU: a bare `python bench.py --gpus 2` (no WORLD_SIZE) must re-execute itself under
torch.distributed.run, and the two ranks must deal the pairs, gather every record with ONE all_gather and print ONE JSON line.
MWF_BENCH_BACKEND=gloo makes that a dry run on CPU with the oracle standing in for the GPU (the partition and the gather are the
same code on RCCL); the line is marked "dry_run": true and is not a measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def _json_lines(stdout):
    return [json.loads(ln) for ln in stdout.splitlines() if ln.startswith("{")]


def test_launcher_command_line():
    import bench
    cmd = bench.launcher_argv(8, ["--gpus", "8", "--steps", "20", "--warmup", "5"], 29517)
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29517"
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]      # the ranks get the caller's arguments unchanged
    p = bench.free_port()
    assert 1024 < p < 65536


@pytest.mark.parametrize("extra", [[], ["--config", "5"]])
def test_bare_two_rank_launch_dry_run_on_gloo(extra):
    r = _run(["--gpus", "2", "--steps", "2"] + extra, {"MWF_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout                      # rank 0 prints ONE line
    d = lines[0]
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["dry_run"] is True
    assert d["gathered_records_match_oracle"] is True     # every pair's record reached rank 0, in global order
    assert d["scaling"] == ("strong" if extra else "weak")
    if extra:   # configs[4]'s shape: a fixed total dealt over the ranks
        assert d["config"]["pairs_total"] == 40 and d["config"]["pairs_this_rank"] == 20
    else:       # configs[2]'s: a fixed share per rank
        assert d["config"]["pairs_total"] == 2 * d["config"]["pairs_this_rank"]


def test_launcher_and_gpus_must_agree():
    r = _run(["--gpus", "2", "--steps", "1"], {"MWF_BENCH_BACKEND": "gloo", "WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "must agree" in (r.stderr + r.stdout)


def test_single_rank_dry_run_and_no_gpu_message():
    r = _run(["--steps", "1", "--warmup", "0"], {"MWF_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_lines(r.stdout)[0]
    assert d["n_gpus"] == 1 and d["dry_run"] is True and d["gathered_records_match_oracle"] is True
    import torch
    if not torch.cuda.is_available():   # the real path refuses to run without a GPU: no CPU fallback
        r = _run(["--steps", "1", "--warmup", "0", "--extras", "0", "--cpu-sample", "0"])
        assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)


def test_bench_reads_the_real_pairs_when_they_are_dropped_in(tmp_path):
    """bench.py --c4 A B / --mhc A B (the reference's Zenodo pairs, README.md:82-88): the FASTA / FASTQ(.gz) reader takes the first record's bytes as they are."""
    import gzip
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">one desc\nACGT\nacgtN\n>two\nTTTT\n")
    fq = tmp_path / "b.fq.gz"
    with gzip.open(fq, "wb") as f:
        f.write(b"@r1\nGATTACA\n+\nIIIIIII\n@r2\nCC\n+\nII\n")
    assert bench.read_first_fasta(str(fa)) == b"ACGTacgtN"
    assert bench.read_first_fasta(str(fq)) == b"GATTACA"
    assert bench.REAL_PAIRS["c4_like_150kb"][1] == 26917 and bench.REAL_PAIRS["mhc_like_5Mb"][1] == 229868


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_full_is_off_by_default_and_steps_must_be_positive():
    bench = _bench_module()
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dry_run_dumps_the_gathered_records(tmp_path):
    """--dump-outputs on the CPU dry run: every pair's (s, n_iter) as float64 .npy, equal to the oracle's, the same from run to run."""
    from miniwfa_amd.synth import synth_pair
    from oracle.pyoracle import Oracle, make_opt
    got = []
    for k in range(2):
        d = tmp_path / f"out{k}"
        r = _run(["--gpus", "2", "--steps", "1", "--dump-outputs", str(d)], {"MWF_BENCH_BACKEND": "gloo"})
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        assert sorted(os.listdir(d)) == ["n_iter.npy", "s.npy"]
        got.append({n: np.load(d / f"{n}.npy") for n in ("s", "n_iter")})
    s, it = got[0]["s"], got[0]["n_iter"]
    assert s.dtype == np.float64 and it.dtype == np.float64 and len(s) == len(it) == 32    # 2 ranks x 16 pairs
    orc, o = Oracle(), make_opt()
    for i in range(len(s)):
        es, eit, _ = orc.align(*synth_pair(50000 + i, 300, 0.05), o)
        assert (s[i], it[i]) == (es, eit), i
    assert all((got[1][n] == got[0][n]).all() for n in ("s", "n_iter"))


class _FakeCigarBatch:
    def __init__(self, nc):
        self.nc, self.fetched = nc, False

    def fetch_cigars(self):
        self.fetched = True

    def cigar(self, i, n):
        assert self.fetched and n == self.nc[i]
        return np.arange(n, dtype=np.uint32) + np.uint32(1000 * i)


def test_dump_outputs_cigars_and_their_cap(tmp_path, monkeypatch):
    bench = _bench_module()
    rng = np.random.default_rng(5)
    n = 200
    nc = rng.integers(0, 60, n).astype(np.int32)
    last = (rng.integers(0, 999, n).astype(np.int32), rng.integers(0, 10 ** 9, n).astype(np.int64), nc)
    ids = np.arange(n) + 400
    # everything fits: every pair's words, in pair order
    files = bench.dump_outputs(str(tmp_path / "all"), last, _FakeCigarBatch(nc), ids)
    assert files == ["cigar.npy", "cigar_pairs.npy", "n_cigar.npy", "n_iter.npy", "s.npy"]
    a = {f[:-4]: np.load(tmp_path / "all" / f) for f in files}
    assert all(v.dtype == np.float64 for v in a.values())
    assert (a["s"] == last[0]).all() and (a["n_iter"] == last[1]).all() and (a["n_cigar"] == nc).all()
    assert (a["cigar_pairs"] == ids).all()
    assert (a["cigar"] == np.concatenate([np.arange(c) + 1000 * i for i, c in enumerate(nc)])).all()
    # a cap smaller than that: a fixed sample of whole pairs, the files within the cap, the same sample every time
    cap = 8 * (5 * n + 2500)
    monkeypatch.setattr(bench, "DUMP_BYTES_CAP", cap)
    picks = []
    for k in range(2):
        d = tmp_path / f"cap{k}"
        bench.dump_outputs(str(d), last, _FakeCigarBatch(nc), ids)
        b = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= cap
        keep = b["cigar_pairs"].astype(np.int64) - 400
        assert 0 < len(keep) < n and (np.diff(keep) > 0).all()
        assert (b["cigar"] == np.concatenate([np.arange(nc[i]) + 1000 * i for i in keep])).all()
        picks.append(keep)
    assert (picks[0] == picks[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cigar", [False, True])
def test_plain_run_line_and_dumped_outputs(tmp_path, cigar):
    """A plain run prints the headline fields only (nothing that takes runs of its own), `steps` is what was asked, and --dump-outputs holds
    the last timed step's records of its batch, equal to the oracle's."""
    from miniwfa_amd.synth import synth_pair
    from oracle.pyoracle import Oracle, make_opt
    d = tmp_path / "out"
    r = _run(["--steps", "3", "--warmup", "1", "--seeds", "1", "--pairs", "24", "--len", "1500", "--dump-outputs", str(d)] + (["--cigar"] if cigar else []),
             timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    for k in ("roofline", "cpu_baseline", "kernel_gbps", "end_to_end", "long_pairs", "call_latency_us"):
        assert k not in line, k
    a = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert sorted(a) == (["cigar", "cigar_pairs", "n_cigar", "n_iter", "s"] if cigar else ["n_iter", "s"])
    orc, o = Oracle(), make_opt(flag=1 if cigar else 0)
    words = []
    for i in range(24):
        es, eit, ecig = orc.align(*synth_pair(50000 + i, 1500, 0.05), o)
        assert (a["s"][i], a["n_iter"][i]) == (es, eit), i
        if cigar:
            assert a["n_cigar"][i] == len(ecig), i
            words += ecig
    if cigar:
        assert (a["cigar_pairs"] == np.arange(24)).all() and (a["cigar"] == np.asarray(words, dtype=np.float64)).all()


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements():
    r = _run(["--full", "--extras", "0", "--cpu-sample", "0", "--steps", "4", "--warmup", "1", "--pairs", "24", "--len", "1500"], timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = _json_lines(r.stdout)[-1]
    assert line["steps"] == 4 and line["roofline"]["kernel_ms"] > 0 and line["kernel_gbps"] > 0 and line["config"]["cells_this_gpu"] > 0
