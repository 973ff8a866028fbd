"""bench.py --dump-outputs: the writer (no GPU): float64 .npy files, a long array cut to the same seeded sample in
every call, per-rank names when there are several ranks."""
import numpy as np

import bench


def test_dump_outputs_writes_float64_and_samples_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    small = np.arange(1000, dtype=np.float32)  # at the limit: written whole
    big = np.arange(5000, dtype=np.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, {"small": small, "values": big})
    a, b = np.load(tmp_path / "a" / "values.npy"), np.load(tmp_path / "b" / "values.npy")
    assert a.dtype == np.float64 and a.shape == (1000,)
    assert a.tobytes() == b.tobytes()
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(big.tolist())  # entries of the array, in index order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    # another array of the same length is sampled at the same places
    bench.dump_outputs(str(tmp_path / "c"), 0, 1, {"values": big + 1.0})
    assert np.array_equal(np.load(tmp_path / "c" / "values.npy"), a + 1.0)


def test_dump_outputs_names_ranks(tmp_path):
    bench.dump_outputs(str(tmp_path), 1, 2, {"values": np.ones(3)})
    assert [p.name for p in tmp_path.iterdir()] == ["values_rank1.npy"]
