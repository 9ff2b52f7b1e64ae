"""bench.py --dump-outputs: the writer's contract (host only).  Every array lands as <name>.npy in
float64, the files together stay within the byte cap, and an array over its share of the cap is cut
to the same sorted sample of its entries in every run."""
import os

import numpy as np

import bench


def test_dump_outputs_float64_files(tmp_path):
    arrays = {"loss_history": [3.0, 2.0, 1.0], "theta": np.arange(6, dtype=np.float32).reshape(2, 3)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["loss_history.npy", "theta.npy"]
    h = np.load(tmp_path / "out" / "loss_history.npy")
    t = np.load(tmp_path / "out" / "theta.npy")
    assert h.dtype == np.float64 and t.dtype == np.float64
    np.testing.assert_array_equal(h, [3.0, 2.0, 1.0])
    np.testing.assert_array_equal(t, np.arange(6.0).reshape(2, 3))


def test_dump_outputs_rank_suffix(tmp_path):
    bench.dump_outputs(str(tmp_path), {"u": np.zeros(2)}, rank=3, world=8)
    assert os.listdir(tmp_path) == ["u_rank3.npy"]


def test_dump_outputs_cap_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * (8 * 100 + 256))   # 100 doubles a share
    big = np.arange(1000, dtype=np.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": np.ones(7)})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)                      # the same sample in every run
    assert a.shape == (100,) and np.all(np.diff(a) > 0)      # sorted, distinct entries of `big`
    assert np.all(np.isin(a, big))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), np.ones(7))
    files = [tmp_path / "a" / f for f in os.listdir(tmp_path / "a")]
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_MAX_BYTES


def test_default_cap_is_64_mb():
    assert bench.DUMP_MAX_BYTES == 64_000_000
