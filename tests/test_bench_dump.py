"""bench.py --dump-outputs, the writer (no GPU): float32 .npy files within the byte budget, arrays kept whole when the set fits, and a larger
set sampled at the same ascending positions in every run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole_in_float32(tmp_path):
    b = _bench()
    g = np.random.default_rng(1)
    arrays = {"edited": g.random((2, 3, 8, 8)), "grad_means": g.normal(size=(100, 3)).astype(np.float32)}
    b.write_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["edited.npy", "grad_means.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == a.shape
        assert np.array_equal(got, a.astype(np.float32))


def test_large_outputs_fit_the_budget_and_sample_the_same_positions(tmp_path):
    b = _bench()
    budget = 400_000
    arrays = {"big": np.arange(300_000, dtype=np.float64), "small": np.arange(10, dtype=np.float32)}
    b.write_outputs(str(tmp_path / "a"), arrays, budget=budget)
    b.write_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert _sizes(tmp_path / "a") <= budget
    big_a, big_b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(big_a, big_b)
    assert big_a.dtype == np.float32 and 0 < big_a.size < 300_000
    assert np.all(np.diff(big_a) > 0)                                  # ascending positions of the flat array, no repeats
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])


def test_default_budget_is_64_mb():
    assert _bench().DUMP_BYTES <= 64_000_000
