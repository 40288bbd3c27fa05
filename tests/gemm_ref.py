"""Host references for the f32 GEMM family (csrc/gemm.hip): no GPU, NumPy float64 only.

``reference``  what a call of ``ss_gemm_f32_batched`` leaves in C (and in a_colsum), written from the ABI text of
               include/ss_hotpath.h: layouts, leading dimensions, the storage-row remap, bias, ReLU, accumulate, batch strides,
               the summed batch.  It works on the flat buffers the pointers point into, so a wrong stride or map reads the NaN
               padding the tests put around every operand.
``route``      a restatement of the dispatcher's choice of kernel, so that a test can say which kernel it means to reach and
               notice when it reaches another.
``int_operands`` / ``assert_exact_range``  small integers whose every partial sum is an integer below 2**24: any order of float
               additions then gives the same bits, and a GEMM can be compared with ``torch.equal``.
``f32_bound``  the first-order error bound of an f32 dot product in any order, for the float cases.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

INT_MAX = 2**31 - 1
IDENT = (INT_MAX, 0, 0)

# tile geometry the routing depends on (csrc/gemm.hip)
BM, BN, BK = 128, 64, 16
WT = 192            # wide tiles are WT x WT
RING = 4            # k tiles in the DMA ring: a K slice shorter than RING * BK stays on the register-staged kernel
GROUP_MAX = 4
FLOAT_K_MAX = 360  # the float cases keep K_total under this: up to here bf16-rounded operands land well outside f32_bound

ROUTES = ("staged", "dma", "wide_kc", "summed_dma", "summed_loop", "group_dma", "group_wide", "group_fallback")


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ the call
@dataclass
class Call:
    """The arguments of ss_gemm_f32_batched with every pointer replaced by an element offset into a flat float buffer
    (``None`` = NULL).  ``ra`` / ``rb`` are (group, gstride, off) of the storage-row remap."""
    a_kc: int
    b_kc: int
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    ra: Tuple[int, int, int] = IDENT
    rb: Tuple[int, int, int] = IDENT
    flags: int = 0
    splits: int = 1
    batch: int = 1
    stride_a: int = 0
    stride_b: int = 0
    stride_c: int = 0
    stride_bias: int = 0
    stride_colsum: int = 0
    a_base: int = 0
    b_base: int = 0
    c_base: int = 0
    bias_base: Optional[int] = None
    colsum_base: Optional[int] = None


def map_rows(n: int, rmap: Sequence[int]) -> np.ndarray:
    """Storage row of the rows 0 .. n-1 of an operand: (r / group) * gstride + r % group + off."""
    G, S, off = rmap
    r = np.arange(n, dtype=np.int64)
    return (r // G) * S + r % G + off


def operand_index(kc: int, rows: int, K: int, ld: int, rmap: Sequence[int]) -> np.ndarray:
    """[rows][K] element offsets (from the operand's pointer) of op(X)[row][k].  kc = 1: X is stored [row][k], the remap applies
    to the row; kc = 0: stored [k][row], the remap applies to k -- in both cases to the index whose stride is ``ld``."""
    if kc:
        return map_rows(rows, rmap)[:, None] * ld + np.arange(K, dtype=np.int64)[None, :]
    return np.arange(rows, dtype=np.int64)[:, None] + map_rows(K, rmap)[None, :] * ld


def gather_a(c: Call, buf: np.ndarray, b: int) -> np.ndarray:
    """op(A) of batch entry b as float64 [M][K]."""
    return np.asarray(buf, dtype=np.float64)[c.a_base + b * c.stride_a + operand_index(c.a_kc, c.M, c.K, c.lda, c.ra)]


def gather_b(c: Call, buf: np.ndarray, b: int) -> np.ndarray:
    """op(B) of batch entry b as float64 [K][N]."""
    return np.asarray(buf, dtype=np.float64)[c.b_base + b * c.stride_b + operand_index(c.b_kc, c.N, c.K, c.ldb, c.rb)].T


def c_index(c: Call, b: int) -> np.ndarray:
    """[M][N] element offsets of C of batch entry b (the summed batch has one C)."""
    sc = 0 if c.flags & 16 else c.stride_c
    return c.c_base + b * sc + np.arange(c.M, dtype=np.int64)[:, None] * c.ldc + np.arange(c.N, dtype=np.int64)[None, :]


def reference(c: Call, a_buf, b_buf, c_buf, bias_buf=None, colsum_buf=None):
    """-> (C buffer afterwards, a_colsum buffer afterwards or None, mask of the C elements the call may write), float64.

    flags bit 3 (workspace mode) is not a result in C; ``reference_reduced`` covers the GEMM + reduce pair."""
    assert not c.flags & 8
    out = np.array(c_buf, dtype=np.float64)
    valid = np.zeros(out.shape, dtype=bool)
    cs = None if c.colsum_base is None else np.array(colsum_buf, dtype=np.float64)
    bias_buf = None if c.bias_base is None else np.asarray(bias_buf, dtype=np.float64)
    n = np.arange(c.N)

    def finish(prod, b, idx):
        v = prod
        if bias_buf is not None:
            v = v + bias_buf[c.bias_base + b * c.stride_bias + n][None, :]
        if c.flags & 1:
            v = v + out[idx]
        if c.flags & 2:
            v = np.maximum(v, 0.0)
        out[idx] = v
        valid[idx] = True

    if c.flags & 16:  # the batch is summed into one C; one bias
        prod = sum(gather_a(c, a_buf, b) @ gather_b(c, b_buf, b) for b in range(c.batch))
        finish(prod, 0, c_index(c, 0))
    else:
        for b in range(c.batch):
            A = gather_a(c, a_buf, b)
            finish(A @ gather_b(c, b_buf, b), b, c_index(c, b))
            if cs is not None:  # column sums of the stored [k][m] A == row sums of op(A), over the mapped k rows only
                cs[c.colsum_base + b * c.stride_colsum + np.arange(c.M)] += A.sum(1)
    return out, cs, valid


def reference_reduced(c: Call, a_buf, b_buf, c_buf):
    """C after a workspace-mode GEMM (flags 8) followed by ss_gemm_splitk_reduce: C[b] += op(A[b]) op(B[b])."""
    return reference(replace(c, flags=1), a_buf, b_buf, c_buf)


# ------------------------------------------------------------------------------------------------------ exact operands
def int_operands(shape, seed: int, lo: int = -4, hi: int = 4) -> np.ndarray:
    """Integer-valued float32 in [lo, hi], roughly a quarter of them zero."""
    rng = np.random.default_rng(seed)
    x = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    x[rng.random(size=x.shape) < 0.16] = 0.0  # on top of the 1/9 the draw gives
    return x


def exact_range(pairs, c0=None, bias=None) -> float:
    """max_ij (sum over all pairs and k of |a||b| + |C0| + |bias|): no partial sum of the case, in any order, exceeds it."""
    tot = None
    for A, B in pairs:
        t = np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(B, dtype=np.float64))
        tot = t if tot is None else tot + t
    if c0 is not None:
        tot = tot + np.abs(np.asarray(c0, dtype=np.float64))
    if bias is not None:
        tot = tot + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return float(tot.max())


def assert_exact_range(pairs, c0=None, bias=None) -> float:
    """Every operand an integer and every possible partial sum below 2**24: what makes bit equality legitimate."""
    for A, B in pairs:
        for X in (A, B):
            X = np.asarray(X, dtype=np.float64)
            assert np.isfinite(X).all() and np.array_equal(X, np.rint(X)), "operands must be integers"
    for X in (c0, bias):
        if X is not None:
            X = np.asarray(X, dtype=np.float64)
            assert np.isfinite(X).all() and np.array_equal(X, np.rint(X)), "C0 / bias must be integers"
    m = exact_range(pairs, c0, bias)
    assert m < 2**24, f"partial sums may reach {m:.0f} >= 2**24: not exact in float32"
    return m


def f32_bound(absA, absB, K_total: int, extra_terms: int = 0, c0=None, bias=None) -> np.ndarray:
    """First-order bound on |fl(sum) - sum| of a float32 dot product of K_total terms plus ``extra_terms`` further additions
    (bias, accumulate, the joins of slices or kcat pairs), in ANY order: each of the at most K_total + extra_terms roundings
    a term passes through changes it by at most 2**-24 relative, one more for the product's own rounding when it is not
    fused.  absA [M][K_total] and absB [K_total][N] are |op(A)| and |op(B)| (all pairs concatenated along K)."""
    mag = np.abs(np.asarray(absA, dtype=np.float64)) @ np.abs(np.asarray(absB, dtype=np.float64))
    if c0 is not None:
        mag = mag + np.abs(np.asarray(c0, dtype=np.float64))
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return (K_total + extra_terms + 1) * 2.0**-24 * mag


# --------------------------------------------------------------------------------------------------------------- route
def slices(K: int, splits: int) -> Tuple[int, int]:
    """-> (number of K slices, elements per slice): the slice length is K / splits rounded up to whole 16-wide k tiles."""
    per = ceil_div(ceil_div(K, splits), BK) * BK
    return ceil_div(K, per), per


class Route(NamedTuple):
    name: str
    nz: int          # K slices of the narrow form (per problem of a group: of problem 0)
    ksplit: int
    wide_nz: Optional[Tuple[int, ...]] = None  # group_wide: the wide plan's slices per problem
    workgroups: Optional[int] = None           # group_wide: GEMM workgroups of the launch


def _dma_ok(c: Call, a_align: int, b_align: int, colsum: bool) -> bool:
    _, per = slices(c.K, c.splits)
    return (not colsum and a_align % 16 == 0 and b_align % 16 == 0 and c.lda % 4 == 0 and c.ldb % 4 == 0 and
            c.stride_a % 4 == 0 and c.stride_b % 4 == 0 and (bool(c.a_kc) or (c.M >= 4 and c.M % 4 == 0)) and
            (bool(c.b_kc) or (c.N >= 4 and c.N % 4 == 0)) and per >= RING * BK)


def route(c: Call, a_align: int, b_align: int, cus: int) -> Route:
    """Which kernel ss_gemm_f32_batched launches for this call.  a_align / b_align: the operand pointers' byte address
    modulo 16; cus: the device's compute units."""
    nz, per = slices(c.K, c.splits)
    dma = _dma_ok(c, a_align, b_align, c.colsum_base is not None)
    if c.flags & 16:
        return Route("summed_dma" if dma else "summed_loop", nz, per)
    if (dma and c.a_kc and c.b_kc and not c.flags & 31 and c.splits == 1 and tuple(c.ra) == IDENT and tuple(c.rb) == IDENT
            and c.K % 4 == 0):
        tiles = ceil_div(c.M, WT) * ceil_div(c.N, WT) * c.batch
        if tiles <= cus and tiles * 10 >= cus * 8 and c.N >= 96:
            return Route("wide_kc", nz, per)
    return Route("dma" if dma else "staged", nz, per)


def wide_plan(shapes: Sequence[Tuple[int, int, int, int]], cus: int) -> Tuple[Tuple[int, ...], int]:
    """K slices per problem and workgroups in all of the 192 x 192-tile form of a group of (M, N, K, batch) problems: the slice
    length is the chip's share of the work, raised (64 times at most) until the group fits the chip in one round."""
    tiles = [ceil_div(M, WT) * ceil_div(N, WT) * batch for M, N, K, batch in shapes]
    work = sum(t * s[2] for t, s in zip(tiles, shapes))
    kt = max(work // cus, RING * BK)

    def nz_of(K, kt_):
        nz = max((K + kt_ // 2) // kt_, 1)
        ks = max(ceil_div(ceil_div(K, nz), BK) * BK, RING * BK)
        return ceil_div(K, ks)

    for _ in range(64):
        if sum(t * nz_of(s[2], kt) for t, s in zip(tiles, shapes)) <= cus:
            break
        kt += kt // 32 + 1
    nzs = tuple(nz_of(s[2], kt) for s in shapes)
    return nzs, sum(t * z for t, z in zip(tiles, nzs))


def route_group(calls: Sequence[Call], aligns: Sequence[Tuple[int, int]], flags: int, cus: int) -> Route:
    """Which form ss_gemm_f32_splitk_group takes for these problems (``aligns``: (a_align, b_align) per problem)."""
    assert 1 <= len(calls) <= GROUP_MAX
    nz, per = slices(calls[0].K, calls[0].splits)
    kmajor = all(not c.a_kc and not c.b_kc and a % 16 == 0 and b % 16 == 0 and c.lda % 4 == 0 and c.ldb % 4 == 0 and
                 c.stride_a % 4 == 0 and c.stride_b % 4 == 0 and c.M >= 4 and c.M % 4 == 0 and c.N >= 4 and c.N % 4 == 0
                 for c, (a, b) in zip(calls, aligns))
    if flags & 1 and kmajor:
        nzs, wgs = wide_plan([(c.M, c.N, c.K, c.batch) for c in calls], cus)
        return Route("group_wide", nz, per, nzs, wgs)
    grouped = all(_dma_ok(c, a, b, False) and c.a_kc == calls[0].a_kc and c.b_kc == calls[0].b_kc
                  for c, (a, b) in zip(calls, aligns))
    return Route("group_dma" if grouped else "group_fallback", nz, per)


def splitk_ws_floats(M: int, N: int, K: int, splits: int, batch: int) -> int:
    """Floats of the workspace a flags-8 GEMM leaves its slices in: one 128 x 64 tile per workgroup."""
    return batch * slices(K, splits)[0] * ceil_div(M, BM) * ceil_div(N, BN) * BM * BN
