"""bench.py without a GPU: its options and --dump-outputs' writer (the GPU runs are in test_gpu_bench.py)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_full_and_dump_outputs_and_zero_steps_is_refused():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert res.returncode == 0 and "--full" in res.stdout and "--dump-outputs" in res.stdout
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert res.returncode == 2 and "--steps" in res.stderr


def test_write_outputs_whole_arrays_under_the_limit(tmp_path):
    scores = np.arange(1000, dtype=np.float32) / 7
    ids = np.array([3, 0xFFFFFFFF, 12], dtype=np.uint32).view(np.int32)  # i32 bit patterns, as the exchange hands them back
    bench.write_outputs(str(tmp_path), {"scores": scores, "ids": ids})
    got = np.load(tmp_path / "scores.npy")
    assert got.dtype == np.float32 and np.array_equal(got, scores)
    got = np.load(tmp_path / "ids.npy")
    assert got.dtype == np.float64 and got.tolist() == [3, 0xFFFFFFFF, 12]
    assert sorted(os.listdir(tmp_path)) == ["ids.npy", "scores.npy"]


def test_write_outputs_samples_the_same_rows_beyond_the_limit(tmp_path):
    limit = 200_000
    scores = np.random.default_rng(1).random(100_000, dtype=np.float32)
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), {"scores": scores}, limit=limit)
    rows = np.load(tmp_path / "a" / "scores_rows.npy")
    got = np.load(tmp_path / "a" / "scores.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and rows.size == got.size > 0
    assert np.array_equal(got, scores[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    for f in ("scores.npy", "scores_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
