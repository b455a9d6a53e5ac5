"""bench.py --dump-outputs (CPU only): the files two builds are compared by.

A large output is sampled at rows that depend on its row count alone, so two
dumps of the same shape hold the same rows; small arrays are written whole;
everything is float32 and the largest config's training dump stays under 64 MB."""

import numpy as np
import torch

import bench


def test_dump_outputs_samples_fixed_rows(tmp_path):
    n, f = 3 * bench.DUMP_ROWS + 7, 8
    y = torch.arange(n * f, dtype=torch.float64).reshape(n, f)
    db = torch.arange(f, dtype=torch.float32)
    bench.dump_outputs(tmp_path / "a", {"y": y, "db": db, "dW": None}, None)
    bench.dump_outputs(tmp_path / "b", {"y": y + 1.0}, 2)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["db.npy", "y.npy"]
    assert [p.name for p in (tmp_path / "b").iterdir()] == ["y_r2.npy"]
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y_r2.npy")
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (bench.DUMP_ROWS, f)
    rows = a[:, 0].astype(np.int64) // f  # y[r, 0] = r * f, exact in float32 below 2^24
    assert (np.diff(rows) > 0).all() and rows[-1] < n
    assert np.array_equal(a, y[torch.from_numpy(rows)].float().numpy())
    assert np.array_equal(b, a + 1.0)  # the same rows of another tensor of that shape
    assert np.array_equal(np.load(tmp_path / "a" / "db.npy"), db.numpy())


def test_dump_outputs_size_bound():
    f = max(max(c[3], c[4]) for c in bench.CONFIGS.values())
    # a training step's y and dx sampled, dW and db whole
    assert 4 * (2 * bench.DUMP_ROWS * f + f * f + f) <= 64_000_000
