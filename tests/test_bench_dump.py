"""bench.py --dump-outputs (CPU: the writer itself): float32/float64 .npy files, at most 64 MB in
all, and a large frame sampled at the same pixels in every run."""
import os

import numpy as np

import bench


def _index_frame(pixels):
    # pixel i holds i as its four RGBA bytes (little endian), so a sample names its own pixels
    return np.arange(pixels, dtype="<u4").view(np.uint8)


def _decode(px):
    return px.astype(np.uint8).view("<u4").ravel()


def test_small_frame_dumped_whole(tmp_path):
    frame = _index_frame(256 * 256)
    bench.dump_outputs(str(tmp_path / "d"), frame, [65536, 3, 2, 1, 0, 0, 0, 0])
    px = np.load(tmp_path / "d" / "frame.npy")
    assert px.dtype == np.float32 and px.shape == (65536, 4)
    assert np.array_equal(px.astype(np.uint8).ravel(), frame)
    c = np.load(tmp_path / "d" / "counters.npy")
    assert c.dtype == np.float64 and c.tolist() == [65536, 3, 2, 1, 0, 0, 0, 0]


def test_large_frame_sample_is_fixed_and_bounded(tmp_path):
    frame = _index_frame(3840 * 2160)
    counters = [2 ** 40 + 1] * 8  # exact in float64
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), frame, counters)
    a, b = (np.load(tmp_path / n / "frame.npy") for n in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_PIXELS, 4)
    assert np.array_equal(a, b)
    idx = _decode(a).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 3840 * 2160
    # spread over the whole frame: every 64th of it holds its share of the sample, within 5 %
    hist = np.bincount(idx * 64 // (3840 * 2160), minlength=64)
    assert np.all(np.abs(hist - len(idx) / 64) < 0.05 * len(idx) / 64)
    assert np.load(tmp_path / "a" / "counters.npy").tolist() == counters
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000
