"""GPU: the nine loss entry points keep the bits of tests/golden/loss_bits.npz, recorded before the loss description (CeLoss,
csrc/ce_row.h) was pulled together -- the fixture's header names the commit.  tests/golden/make_loss_golden.py holds the cases and
runs them; this test runs them again and compares.

Exact: logits, d_logits, hit counts, confusion matrices, first_seen, the label / prediction vectors, the error flag, the class
weight sums, every per-row loss and weight, and the loss and weight sums where one wave adds them (B = 1).  Where several waves
add a sum with float atomics (names ending in ``_any_order``) its order is free: the sum is held to the float64 sum of the per-row
values, which are themselves compared exactly, within (n - 1) u |sum| -- what tests/test_gpu_class_weights.py allows between two
orders of the same n terms."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import make_loss_golden as M  # noqa: E402

U = 2.0 ** -24


def test_loss_entry_points_keep_the_recorded_bits(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    header, want = M.load(os.path.join(golden_dir, "loss_bits.npz"))
    got = M.record()
    print(f"{len(want)} arrays recorded on: {header['tree']}")
    assert set(got) == set(want)
    for part in ("ce", "eval", "tail"):
        assert any(k.startswith(part + "/") for k in want)
    differ = []
    for k in sorted(want):
        if k.endswith("_any_order"):
            rows = want[k.replace("loss_sum_any_order", "loss_rows").replace("wsum_any_order", "wsum_rows")].astype(np.float64)
            ref, n = float(rows.sum()), len(rows)
            err = abs(float(got[k][0]) - ref)
            print(f"{k}: {float(got[k][0]):.9g}, float64 sum of its {n} rows {ref:.9g}, err {err:.3e}, bound {(n - 1) * U * abs(ref):.3e}")
            assert err <= (n - 1) * U * abs(ref), k
        elif got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes():
            differ.append(k)
    assert not differ, differ
