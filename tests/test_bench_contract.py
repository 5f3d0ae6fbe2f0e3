"""Driver-contract guard: `python bench.py` must emit exactly one JSON
line with the agreed fields, at CPU-debug scale."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract(tmp_path):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cpu",
         "--steps", "1", "--warmup", "0", "--gb-per-gpu", "0.005",
         "--partitions-per-executor", "16"],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    for field in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
        assert field in j, field
    assert j["n_gpus"] == 1 and j["steps"] == 1
    assert j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["data"] == "synthetic"
    assert isinstance(j["value"], (int, float)) and j["value"] > 0
    cfg = j["config"]
    for field in ("model", "global_batch", "partitions", "parallelism"):
        assert field in cfg, field


import numpy as np
import pytest


def _run_bench(*extra):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cpu",
         "--gb-per-gpu", "0.002", "--partitions-per-executor", "16", *extra],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), out.stderr


def test_bench_dump_outputs_is_the_sorted_input_and_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's output (here small
    enough to be dumped whole) as float .npy files, identical from run to
    run, and equal to the sorted seeded input."""
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        j, _ = _run_bench("--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(d))
        assert j["steps"] == 2 and j["ms_per_step"] > 0
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(p.name for p in dirs[1].iterdir())
    assert "sorted_records_sample.npy" in names
    assert all(n.endswith(".npy") for n in names)
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    n_rec = int(0.002 * (1 << 30) / 16)
    keys = np.sort(np.random.default_rng(0).integers(
        0, 2 ** 64, n_rec, dtype=np.uint64))
    kb = keys.view(np.uint8).reshape(-1, 8)
    want = np.concatenate([kb, kb], axis=1)      # payload mirrors the key
    got = np.load(dirs[0] / "sorted_records_sample.npy")
    assert np.array_equal(np.load(dirs[0] / "sorted_records_sample_index.npy"),
                          np.arange(n_rec))
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(np.load(dirs[0] / "sorted_records_bytesum.npy"),
                          want.sum(axis=0, dtype=np.float64))


def test_bench_full_keeps_the_result_line():
    """--full adds the phase breakdowns on stderr; the result line keeps
    its fields."""
    j, err = _run_bench("--steps", "1", "--warmup", "0", "--full")
    for field in ("metric", "value", "unit", "higher_is_better", "dtype",
                  "ms_per_step"):
        assert field in j, field
    assert j["metric"] == "terasort_sorted_gb_per_s" and j["steps"] == 1
    assert "[step 0]" in err


@pytest.mark.parametrize("workload", ["pagerank", "join", "reducebykey",
                                      "groupby"])
def test_bench_all_workloads_emit_json(tmp_path, workload):
    """Every BASELINE workload's bench path runs end-to-end on CPU and
    emits the JSON line (guards attr regressions like r02's seq_len)."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cpu",
         "--workload", workload, "--steps", "1", "--warmup", "0",
         "--gb-per-gpu", "0.002", "--partitions-per-executor", "16"],
        capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["value"] > 0 and j["config"]["model"] == workload
