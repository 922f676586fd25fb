"""bench.py's launch contract on CPU: `python bench.py --gpus N` with no launcher in the environment starts one rank per GPU
through torch.distributed.run as a child process and relays rank 0's single JSON line (the driver's command form).  The scan
itself needs a GPU, so these runs use --dry-run: made-up counts and records, the real launch / counts exchange / hit gather /
JSON code (gloo instead of RCCL).  The reference's model for the fan-out: hypergrep/multiscanner.py:197-214."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra: str, timeout: int = 300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", *extra], capture_output=True, text=True, timeout=timeout, env=env, check=False)
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    return proc, lines


def test_self_launch_two_ranks_prints_one_json_line():
    proc, lines = _run("--gpus", "2", "--steps", "3", "--warmup", "1", "--gib", "0.01", "--workload", "c2")
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert len(lines) == 1, proc.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["scaling"] == "weak" and out["config"]["parallelism"] == "shard2"
    assert out["config"]["hits"] == 2 * 1000  # all ranks' records of one step
    assert "0.01 GiB" in out["metric"] and "1 patterns" in out["metric"]  # the label follows --gib / --workload
    assert out["data"].startswith("dry-run")


def test_single_rank_needs_no_launcher():
    proc, lines = _run("--gpus", "1", "--steps", "2", "--warmup", "0", "--gib", "0.01")
    assert proc.returncode == 0, proc.stderr[-2000:]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 1


def test_config5_sized_gather_through_the_launcher():
    """config 5 sends ~458 MB per peer; here 2.5 M records (40 MB) per rank and step through the same code."""
    proc, lines = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--gib", "0.01", "--workload", "c5", "--dry-hits", "2500000")
    assert proc.returncode == 0, proc.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["config"]["hits"] == 5000000 and out["n_gpus"] == 2


def test_a_failing_rank_fails_the_launcher():
    proc, lines = _run("--gpus", "2", "--steps", "1", "--gib", "0.01", "--backend", "no-such-backend")  # every rank dies in init_process_group
    assert proc.returncode != 0 and not lines


def _dumped(path) -> dict:
    files = sorted(os.listdir(path))
    assert files == ["hits.npy", "hits_index.npy", "scan_counts.npy"], files
    assert sum(os.path.getsize(os.path.join(path, f)) for f in files) <= 64 * 10**6
    arrays = {f[:-4]: np.load(os.path.join(path, f)) for f in files}
    for a in arrays.values():
        assert a.dtype in (np.float32, np.float64)
    return arrays


def _same(a: dict, b: dict) -> None:
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_single_rank_repeats(tmp_path):
    """--dump-outputs writes the last timed step's counts and hit records; the same arguments give the same files."""
    runs = []
    for name in ("a", "b"):
        proc, lines = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--gib", "0.01", "--dump-outputs", str(tmp_path / name))
        assert proc.returncode == 0, proc.stderr[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        runs.append(_dumped(tmp_path / name))
        assert list(runs[-1]["scan_counts"]) == [out["config"]["lines"], out["config"]["hits"]]
        assert runs[-1]["hits"].shape == (out["config"]["hits"], 5) and not out["dump_outputs"]["sampled"]
    _same(*runs)


def test_dump_outputs_sample_a_large_gather_under_the_limit(tmp_path):
    """Rank 0's gathered records of two ranks, more than fit into 64 MB: a seeded sample of rows, in order."""
    proc, lines = _run("--gpus", "2", "--steps", "2", "--warmup", "0", "--gib", "0.01", "--dry-hits", "1500000", "--dump-outputs", str(tmp_path))
    assert proc.returncode == 0, proc.stderr[-2000:]
    out = json.loads(lines[0])
    arrays = _dumped(tmp_path)
    assert out["dump_outputs"]["sampled"] and arrays["scan_counts"][1] == out["config"]["hits"] == 3000000
    rows, hits = arrays["hits_index"], arrays["hits"]
    assert hits.shape == (rows.shape[0], 3) and np.all(np.diff(rows) > 0) and rows[-1] < 3000000
    assert np.all(np.diff(hits[:, 0]) >= 0)  # ordered by line number


@pytest.mark.gpu
def test_dump_outputs_repeat_on_the_gpu(tmp_path):
    """The real scan path: two runs with the same arguments dump identical outputs, and the counts are the JSON line's."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    runs = []
    for name in ("a", "b"):
        proc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--gib", "0.25",
                               "--no-extra", "--cpu-seconds", "0", "--dump-outputs", str(tmp_path / name)],
                              capture_output=True, text=True, timeout=600, env=env, check=False)
        assert proc.returncode == 0, proc.stderr[-2000:]
        out = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][0])
        runs.append(_dumped(tmp_path / name))
        assert list(runs[-1]["scan_counts"]) == [out["config"]["lines"], out["config"]["hits"]] and out["config"]["hits"] > 0
    _same(*runs)
