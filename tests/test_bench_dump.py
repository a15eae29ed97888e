"""bench.py --dump-outputs: float .npy files under the size cap, the same rows from run to run."""
import numpy as np

import bench


def _arrays(npix):
    rng = np.random.default_rng(7)
    return {"accum": rng.random((npix, 4), dtype=np.float32),
            "bgra": rng.integers(0, 256, (npix, 4), dtype=np.uint8),
            "rays": np.array([123456789012.0])}


def test_small_outputs_are_written_whole(tmp_path):
    arrs = _arrays(1000)
    bench.dump_outputs(str(tmp_path / "d"), arrs)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["accum", "bgra", "rays"]
    assert got["accum"].dtype == np.float32 and np.array_equal(got["accum"], arrs["accum"])
    assert got["bgra"].dtype == np.float32 and np.array_equal(got["bgra"], arrs["bgra"].astype(np.float32))
    assert got["rays"].dtype == np.float64 and got["rays"][0] == 123456789012.0


def test_large_outputs_keep_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    arrs = _arrays(10_007)                                   # 160 KB each: both past an even share
    bench.dump_outputs(str(tmp_path / "a"), arrs)
    bench.dump_outputs(str(tmp_path / "b"), arrs)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 200_000
    a, b = (np.load(tmp_path / "a" / "accum.npy"), np.load(tmp_path / "a" / "bgra.npy"))
    assert np.array_equal(a, np.load(tmp_path / "b" / "accum.npy"))
    assert a.shape == b.shape and 5000 < a.shape[0] < 10_007
    # the kept rows are rows of the input, in order, and the same rows in both arrays
    keep = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(10_007, a.shape[0], replace=False))
    assert np.array_equal(a, arrs["accum"][keep])
    assert np.array_equal(b, arrs["bgra"][keep].astype(np.float32))
    assert np.load(tmp_path / "a" / "rays.npy")[0] == 123456789012.0
