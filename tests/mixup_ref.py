"""CPU restatement of the mixup kernels (csrc/batch.hip: ss_batch_plan_mixup, ss_batch_mixup) in NumPy.

The plan is integer arithmetic on Philox4x32-10 outputs, in the scheme of tests/batch_plan_ref.py with the domain tag "mixp", so it
is bit-equal to the kernel by construction:

  counter (batch_first_row, "mixp", 0)      -> u0, u1: mixed iff augment and u0 < thr(mixup_prob); k = table[mulhi(u1, N)]
  counter (batch_first_row + b, "mixp", 1)  -> key_b; perm[b] = rank of (key_b, b) among the rows (a stable argsort)
  not mixed: perm = identity, k = 256

The blend of the ROI bytes is exact integer arithmetic too; the feature blend is restated in float64 (``blend_f64``, what the
kernel's two roundings are measured against) and, for the pass-through cases, as the copy it is.
"""
import numpy as np

from batch_plan_ref import _index_range, draw, mulhi, thr

TAG_MIXUP = 0x6D697870  # "mixp"


def batch_draw(batch_first_row, seed, augment, mixup_prob, N):
    """-> (mixed, table index) of the batch whose first row draws ``batch_first_row``."""
    u0, u1, _, _ = draw(np.uint64(int(batch_first_row) & ((1 << 64) - 1)), TAG_MIXUP, 0, seed)
    mixed = bool(augment) and int(u0) < thr(mixup_prob)
    return mixed, int(mulhi(u1, N))


def row_keys(batch_first_row, B, seed):
    return draw(_index_range(batch_first_row, B), TAG_MIXUP, 1, seed)[0]


def rank_keys(keys):
    """perm[b] = the rank of (key_b, b) among all rows: the number of rows j with key_j < key_b, or key_j == key_b and j < b (the
    kernel counts exactly these).  A stable argsort gives the row at each rank; its inverse is the rank of each row."""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")  # order[rank] = row
    perm = np.empty(len(keys), np.int64)
    perm[order] = np.arange(len(keys))
    return perm


def plan(lens, y, augment, batch_first_row, seed, mixup_prob, table):
    """ss_batch_plan_mixup -> dict(perm int32, y_b int64, lens_m int64, k int, lam float32, mixed bool)."""
    lens, y, table = np.asarray(lens, np.int64), np.asarray(y, np.int64), np.asarray(table)
    B = len(lens)
    mixed, at = batch_draw(batch_first_row, seed, augment, mixup_prob, len(table))
    perm, k = np.arange(B, dtype=np.int64), 256
    if mixed:
        k = min(int(table[at]), 256)
        perm = rank_keys(row_keys(batch_first_row, B, seed))
    return dict(perm=perm.astype(np.int32), y_b=y[perm], lens_m=np.maximum(lens, lens[perm]), k=k, lam=np.float32(k / 256.0),
                mixed=mixed)


def blend_u8(R, perm, k):
    """(k R[b] + (256 - k) R[perm[b]] + 128) >> 8 per byte: exact."""
    R = np.asarray(R)
    a, b = R.astype(np.int64), R[np.asarray(perm, np.int64)].astype(np.int64)
    return ((int(k) * a + (256 - int(k)) * b + 128) >> 8).astype(np.uint8)


def blend_f64(X, perm, k):
    """lam X[b] + (1 - lam) X[perm[b]] in float64 (lam = k / 256 and 1 - lam are exact in either precision), and the bound the
    float32 kernel holds against it: one rounding of (1 - lam) * xb and one of the fused multiply-add, half an ulp each, neither
    term larger than the operand it rounds -- 2^-23 (lam |xa| + (1 - lam) |xb|), zero where both operands are zero."""
    X = np.asarray(X, np.float64)
    lam = int(k) / 256.0
    xa, xb = X, X[np.asarray(perm, np.int64)]
    return lam * xa + (1.0 - lam) * xb, 2.0 ** -23 * (lam * np.abs(xa) + (1.0 - lam) * np.abs(xb))


def passthrough_rows(perm, k):
    """The clips the kernel copies byte for byte: every clip when k == 256, else those that are their own partner."""
    perm = np.asarray(perm, np.int64)
    return np.ones(len(perm), bool) if int(k) == 256 else perm == np.arange(len(perm))


def blend_f32(X, perm, k):
    """The kernel's float32 result up to its two roundings: the float64 blend rounded once, with the copied clips exact."""
    X = np.asarray(X, np.float32)
    out = blend_f64(X, perm, k)[0].astype(np.float32)
    keep = passthrough_rows(perm, k)
    out[keep] = X[keep]
    return out
