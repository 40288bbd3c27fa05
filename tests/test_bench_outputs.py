"""CPU: what ``bench.py --dump-outputs`` writes (bench.py:dump_outputs) -- float32 / float64 ``.npy`` files, large arrays as one
fixed, seeded sample of their elements, at most 64 MB in all."""
import numpy as np
import pytest
import torch

from test_bench_profiles import _bench


def test_dump_outputs_dtypes_and_names(tmp_path):
    b = _bench()
    b.dump_outputs(str(tmp_path / "out"), {"loss": torch.tensor(1.5), "correct": torch.tensor(7, dtype=torch.int32),
                                           "params": torch.arange(10, dtype=torch.float32), "norm": np.float64(2.25)})
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert sorted(got) == ["correct", "loss", "norm", "params"]
    assert got["loss"].dtype == got["correct"].dtype == got["params"].dtype == np.float32 and got["norm"].dtype == np.float64
    assert float(got["loss"]) == 1.5 and float(got["correct"]) == 7.0 and float(got["norm"]) == 2.25
    assert np.array_equal(got["params"], np.arange(10, dtype=np.float32))


def test_dump_outputs_samples_large_arrays_the_same_way_every_run(tmp_path):
    b = _bench()
    n = b.DUMP_MAX_ELEMENTS + 12345
    big = torch.arange(n, dtype=torch.float64) * 0.5
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"big": big})
    a1, a2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a1.shape == (b.DUMP_MAX_ELEMENTS,) and np.array_equal(a1, a2)
    assert np.all(np.diff(a1) > 0) and np.all(a1 * 2 == np.round(a1 * 2))  # ascending elements of the array itself


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    b = _bench()
    part = torch.zeros(b.DUMP_MAX_ELEMENTS, dtype=torch.float64)  # 32 MB each
    with pytest.raises(AssertionError):
        b.dump_outputs(str(tmp_path / "out"), {"a": part, "b": part, "c": torch.zeros(1)})
    assert not (tmp_path / "out").exists()
