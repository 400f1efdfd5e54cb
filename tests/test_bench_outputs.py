"""bench.py --dump-outputs on the host: the frame is written whole up to 64 MB, above that as a fixed, seeded sample of its pixels."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_frame_up_to_the_cap_is_written_whole(tmp_path):
    bench = _bench()
    frame = np.random.default_rng(1).random((54, 96, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    assert os.listdir(tmp_path / "out") == ["sum_buffer.npy"]
    back = np.load(tmp_path / "out" / "sum_buffer.npy")
    assert back.dtype == np.float32 and np.array_equal(back, frame)


def test_larger_frame_is_written_as_the_same_seeded_sample(tmp_path):
    bench = _bench()
    h, w = 2000, 3000    # 72 MB: above the cap.  Each pixel holds its own index (low and high 12 bits, exact in float32)
    index = np.arange(h * w)
    frame = np.stack([index % 4096, index // 4096, np.zeros(h * w)], axis=-1).astype(np.float32).reshape(h, w, 3)
    assert frame.nbytes > bench.DUMP_MAX_BYTES
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), frame)
        assert os.listdir(tmp_path / run) == ["sum_buffer_sample.npy"]
    a = np.load(tmp_path / "a" / "sum_buffer_sample.npy")
    b = np.load(tmp_path / "b" / "sum_buffer_sample.npy")
    assert a.dtype == np.float32 and a.nbytes <= bench.DUMP_MAX_BYTES and a.shape == (bench.DUMP_MAX_BYTES // 12, 3)
    assert np.array_equal(a, b)
    # every sampled row is a pixel of the frame, each at most once
    pixel = a[:, 0].astype(np.int64) + 4096 * a[:, 1].astype(np.int64)
    assert np.array_equal(a, frame.reshape(-1, 3)[pixel]) and len(np.unique(pixel)) == len(pixel)
