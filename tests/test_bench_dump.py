"""bench.py --dump-outputs on the host: dtypes of the written arrays, and the seeded row sample above 64 MB."""
import numpy as np
import torch

import bench


def test_dump_writes_float32_scores_and_float64_ids(tmp_path):
    s = torch.rand((1024, 10), dtype=torch.float32)
    i = torch.randint(0, 1_000_000, (1024, 10), dtype=torch.int64)
    bench.dump_outputs(np, str(tmp_path / "d"), {"scores": s, "ids": i})
    ds, di = np.load(tmp_path / "d" / "scores.npy"), np.load(tmp_path / "d" / "ids.npy")
    assert ds.dtype == np.float32 and np.array_equal(ds, s.numpy())
    assert di.dtype == np.float64 and np.array_equal(di, i.numpy().astype(np.float64))
    assert not (tmp_path / "d" / "rows.npy").exists()


def test_dump_above_the_limit_keeps_the_same_seeded_rows_of_every_array(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100_000)
    s = torch.arange(8192 * 10, dtype=torch.float32).reshape(8192, 10)
    i = torch.arange(8192 * 10, dtype=torch.int64).reshape(8192, 10)
    for d in ("a", "b"):
        bench.dump_outputs(np, str(tmp_path / d), {"scores": s, "ids": i})
    files = ("scores.npy", "ids.npy", "rows.npy")
    total = sum((tmp_path / "a" / f).stat().st_size - 128 for f in files)      # minus the .npy headers
    assert total <= 100_000
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert rows.size > 500 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), s.numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy"), i.numpy()[rows].astype(np.float64))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
