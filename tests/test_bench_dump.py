"""bench.py --dump-outputs on CPU: the writer behind it keeps float32 files under the size limit and, when it has to sample,
draws the same elements every time (two builds must be comparable output for output)."""
import os

import numpy as np

import bench


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    a = {"flow_lo": np.arange(24, dtype=np.float64).reshape(1, 2, 3, 4), "flow_up": np.ones((1, 1, 12, 16), np.float32)}
    info = bench.dump_outputs(str(tmp_path), a)
    for name, v in a.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))
        assert info[name] == {"shape": list(v.shape), "saved_elements": v.size}


def test_large_outputs_are_a_fixed_sample_under_the_limit(tmp_path):
    limit = 1 << 20
    rng = np.random.default_rng(1)
    a = {"flow_lo": rng.random((2, 2, 46, 78), np.float32), "flow_up": rng.random((2, 1, 368, 624), np.float32)}
    info = bench.dump_outputs(str(tmp_path / "x"), a, limit=limit)
    bench.dump_outputs(str(tmp_path / "y"), a, limit=limit)
    assert _size(tmp_path / "x") <= limit
    for name, v in a.items():
        x, y = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "y" / (name + ".npy"))
        assert 0 < x.size < v.size and info[name]["saved_elements"] == x.size and info[name]["shape"] == list(v.shape)
        assert np.array_equal(x, y)
        assert np.isin(x, v).all()
