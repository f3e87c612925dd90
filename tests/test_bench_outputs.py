"""bench.py --dump-outputs (CPU only): every output as <name>.npy in float64, exact for the histograms' counts; an output
above its share of the size cap is written as a fixed, seeded sample with the indices beside it."""
import numpy as np

import bench


def test_dump_outputs_float64_exact(tmp_path):
    h = np.arange(3 * 12, dtype=np.uint64).reshape(3, 12) * np.uint64(2**40)
    bench.dump_outputs(str(tmp_path / "d"), {"histograms": h})
    got = np.load(tmp_path / "d" / "histograms.npy")
    assert got.dtype == np.float64 and got.shape == h.shape
    assert np.array_equal(got.astype(np.uint64), h)
    assert not (tmp_path / "d" / "histograms.sample_index.npy").exists()


def test_dump_outputs_samples_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 12)
    a = np.arange(10_000, dtype=np.uint64) * np.uint64(3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": a})
    x, i = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "x.sample_index.npy")
    assert x.dtype == np.float64 and x.nbytes + i.nbytes <= 1 << 12 and len(np.unique(i)) == len(i)
    assert np.array_equal(x, a[i.astype(np.int64)].astype(np.float64))
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))   # the same sample from run to run
