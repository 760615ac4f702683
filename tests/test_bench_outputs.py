"""bench.py --dump-outputs: what the timed path computed, as float32 / float64 .npy files within the dump's budget; a frame larger than
the budget keeps the same seeded sample of pixels on every run, so two builds can be compared output for output."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_keeps_the_whole_accumulator_within_the_budget(tmp_path):
    accum = np.random.default_rng(1).random((96 * 54, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path), accum, [1536, 10, 20, 30, 40, 50])
    assert sorted(os.listdir(tmp_path)) == ["accum.npy", "counters.npy"]
    got = np.load(tmp_path / "accum.npy")
    assert got.dtype == np.float32 and np.array_equal(got, accum)
    c = np.load(tmp_path / "counters.npy")
    assert c.dtype == np.float64 and c.tolist() == [1536, 10, 20, 30, 40, 50]


def test_dump_samples_a_larger_frame_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 24 * 1000)  # 1000 pixels of 16 B + their 8 B index
    accum = np.random.default_rng(2).random((5000, 4), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), accum, [1.0])
    px = np.load(tmp_path / "a" / "accum_pixels.npy")
    assert px.dtype == np.float64 and len(px) == 1000 and np.all(np.diff(px) > 0)
    assert np.array_equal(px, np.load(tmp_path / "b" / "accum_pixels.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "accum.npy"), accum[px.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 24 * 1000 + 1024


def test_the_default_bench_line_is_within_the_dump_budget():
    assert 1920 * 1080 * 16 <= bench.DUMP_BUDGET_BYTES < 64e6  # bench.py's default frame is dumped whole
