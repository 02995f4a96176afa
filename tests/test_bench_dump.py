"""bench.py --dump-outputs: what it writes, and that it stays under its size budget (host only: the image is synthetic)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_an_image_within_the_budget_is_written_whole(tmp_path):
    fb = np.random.default_rng(1).random((1080, 1920, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), fb)
    assert os.listdir(tmp_path / "out") == ["framebuffer.npy"]
    got = np.load(tmp_path / "out" / "framebuffer.npy")
    assert got.dtype == np.float32 and np.array_equal(got, fb)


def test_a_larger_image_is_a_fixed_sample_of_whole_rows(tmp_path):
    fb = np.random.default_rng(2).random((2160, 3840, 4), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), fb)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["framebuffer_row_index.npy", "framebuffer_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    rows = np.load(tmp_path / "a" / "framebuffer_rows.npy")
    index = np.load(tmp_path / "a" / "framebuffer_row_index.npy")
    assert rows.dtype == np.float32 and index.dtype == np.float64 and rows.shape == (len(index), 3840, 4)
    assert len(index) > 2160 // 3 and np.all(np.diff(index) > 0)
    assert np.array_equal(rows, fb[index.astype(np.int64)])
    for f in files:                                     # the same sample every time
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
