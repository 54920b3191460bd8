"""CPU suite: bench.py --dump-outputs writes float32 / float64 .npy files, integer codes exactly, and keeps a fixed leading sample of
every array's clips when the outputs would pass the 64 MB cap."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_types_and_values(tmp_path):
    import bench
    codes = np.arange(2 * 9 * 5, dtype=np.int64).reshape(2, 9, 5) % 1024
    audio = np.linspace(-1, 1, 2 * 1 * 50, dtype=np.float32).reshape(2, 1, 50)
    bench.dump_outputs(str(tmp_path / "d"), {"codes": codes, "audio": audio})
    c, a = np.load(tmp_path / "d" / "codes.npy"), np.load(tmp_path / "d" / "audio.npy")
    assert c.dtype == np.float64 and np.array_equal(c, codes)
    assert a.dtype == np.float32 and np.array_equal(a, audio)


def test_dump_outputs_keeps_a_fixed_leading_sample_under_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    big = np.random.default_rng(0).standard_normal((10, 1, 200)).astype(np.float32)      # 8000 B
    small = np.arange(10 * 5, dtype=np.int64).reshape(10, 5)                              # 400 B as float64
    bench.dump_outputs(str(tmp_path), {"audio": big, "codes": small})
    a, c = np.load(tmp_path / "audio.npy"), np.load(tmp_path / "codes.npy")
    assert a.nbytes + c.nbytes <= 4000
    assert a.shape[0] == c.shape[0] == 4 and np.array_equal(a, big[:4]) and np.array_equal(c, small[:4])
