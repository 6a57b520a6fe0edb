"""bench.py's multi-rank branch end to end on CPU (no GPU): two ranks over gloo through
torch.distributed.run, with tests/bench_rehearsal.py standing in for torch.cuda and
libkmeranno.so. Checks the one JSON line rank 0 prints (contract keys, the joined ranks, the
table broadcast record) and the --verify parity checks (gathered outputs = one single-rank
call, reduced tally, identical replicas), for the strong (c4) and weak (c5) workloads, run with
--full (per-kernel times and the roofline are part of the line). A plain one-rank run prints the
headline line without them and, with --dump-outputs, writes the same arrays every time."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("workload,rows", [("c4", 300_000), ("c5", 1_500_000)])
def test_bench_multirank_branch_rehearsal(workload, rows):
    env = dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "bench_rehearsal.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--workload", workload, "--n-seq", "300", "--table-rows", str(rows),
           "--dist-backend", "gloo", "--same-device", "--verify", "--full", "--no-extras",
           "--no-cpu-baseline"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 2
    assert out["scaling"] == ("strong" if workload == "c4" else "weak")
    assert [r["rank"] for r in out["ranks"]] == [0, 1]
    assert out["rank_ms_per_step_min"] <= out["rank_ms_per_step_max"]
    assert out["table_broadcast"]["ms"] is not None and out["table_broadcast"]["bytes"] > 0
    v = out["verify"]
    assert v["ok"] and v["outputs_equal_single_rank"] and v["tally_equals_single_rank"]
    assert v["table_identical_across_ranks"] and v["called"] > 0


def test_bench_plain_run_rehearsal(tmp_path):
    """One rank, no --full: the line keeps the headline keys and carries none of the figures
    that take runs of their own; --steps sets the timed steps (the tally counts them); two runs
    with the same arguments dump identical float arrays, one value per protein / function."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    dumps = []
    for name, steps in (("a", 3), ("b", 3)):
        cmd = [sys.executable, os.path.join(ROOT, "tests", "bench_rehearsal.py"), "--gpus", "1",
               "--steps", str(steps), "--warmup", "1", "--workload", "c2", "--n-seq", "200",
               "--table-rows", "300000", "--dump-outputs", str(tmp_path / name)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=ROOT, env=env)
        assert p.returncode == 0, p.stderr[-4000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        out = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in out, key
        assert out["steps"] == steps and out["ms_per_step"] > 0
        for key in ("roofline", "phases_ms", "e2e_host_call", "cpu_baseline"):
            assert key not in out, key
        d = {f: np.load(tmp_path / name / f"{f}.npy") for f in ("fid", "count", "status", "tally")}
        assert sorted(os.listdir(tmp_path / name)) == ["count.npy", "fid.npy", "status.npy",
                                                       "tally.npy"]
        assert all(a.dtype == np.float64 for a in d.values())
        assert len(d["fid"]) == len(d["count"]) == len(d["status"]) == 200
        called = d["status"] == 1
        assert called.sum() == out["called_per_batch"] > 0
        assert d["tally"].sum() == steps * called.sum()
        dumps.append(d)
    for f in ("fid", "count", "status", "tally"):
        assert (dumps[0][f] == dumps[1][f]).all(), f
