"""Host references for the bf16 GEMM family (csrc/gemm_bf16.hip): no GPU, NumPy only.  The bf16 counterpart of tests/gemm_ref.py,
whose ``Call``, ``map_rows``, ``operand_index`` and ``reference`` it reuses unchanged.

``bf16_round`` / ``bf16_bits``  float32 -> bf16, round to nearest, ties to even, by bit arithmetic on the uint32 view.
``place_bf16``     an operand as the bf16 ABI wants it (include/ss_hotpath.h: leading dimensions zero-padded to a multiple of 8)
                   inside a buffer of bf16 NaN: the zeros are the ONLY thing a kernel may read besides the operand.
``reference_bf16`` what ss_gemm_bf16_batched leaves in C: ``gemm_ref.reference`` on the rounded (f32 source) or decoded (bf16 source)
                   operands, everything else float64.
``route_bf16``     the dispatcher's choice of kernel and the k tiles of every K slice.
``group_plan``     the stream-K plan of ss_gemm_bf16_splitk_group: ring_group_prepare and the walk of the group kernel.
``carry_free_rows``  a deliberately WRONG row map: what a k-major loader reads that steps 64 k lines with the carry-free increment
                   and never applies the carry.  The remap tests use it to show that they would notice such a kernel.
"""
from __future__ import annotations

from dataclasses import replace
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import gemm_ref as GR
from gemm_ref import Call, ceil_div

BF16_NAN = 0x7FC0
GUARD_ROWS = 8

# tile geometry (csrc/gemm_bf16.hip)
BK_F32, BK_B16 = 32, 64          # k tile of the register-staged kernel: f32 operands / bf16 operands
RBM, RBN, RBK = 256, 128, 64     # ring kernel
GROUP_MAX = 8
SLAB_FLOATS = RBM * RBN

ROUTES = ("staged_f32", "staged_b16", "ring", "ring_kcat")


def ceil8(n: int) -> int:
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------ rounding
def bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16): nearest, ties to even.  The carry of the rounding runs into the exponent, so the
    largest finite bf16 + half an ulp becomes inf; inf stays inf; NaN stays a (quiet) NaN of the same sign."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = np.isnan(x)
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def bf16_decode(bits) -> np.ndarray:
    """bf16 bit patterns -> the float32 they stand for (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    return bf16_decode(bf16_bits(x))


def tie_table() -> np.ndarray:
    """float32 values whose rounding to bf16 is a tie or next to one, and the edges of the format: the table the CPU pin of
    ``bf16_bits`` and the GPU test of ss_cvt_bf16_rows share."""
    pats = []
    for base in (1.0, 257.0, 259.0, -1.0, -257.0, -259.0):
        hi = int(np.float32(base).view(np.uint32)) >> 16
        for h in range(hi - 4, hi + 5):          # the bf16 numbers around the base: even and odd last bits
            for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):   # 0x8000: exactly half an ulp above
                pats.append((h << 16) | lo)
    pats += [0x00000000, 0x80000000]                                   # +-0
    pats += [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000]  # largest finite bf16 -+ half an ulp: the upper is inf
    pats += [0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x80008000, 0x80018000]  # denormals
    pats += [0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345]  # inf, NaN
    return np.array(pats, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------------------- placing
def place_bf16(kc: int, rows: int, K: int, ld_extra: int, rmap: Sequence[int], vals: Sequence[np.ndarray], gap: int = 0
               ) -> Tuple[np.ndarray, int, int, int]:
    """The operands ``vals`` (one float32 array per batch entry, storage shape: [rows][K] for kc = 1, [K][rows] for kc = 0; every
    value must be a bf16 number or is rounded) -> (flat uint16 buffer, element offset of the first operand, ld, stride).

    ld = the contiguous extent rounded up to 8, + ld_extra (a multiple of 8).  Storage row r of the operand lies at row
    map_rows(r) of its batch entry.  Written: the entries, and ZERO from the extent up to the extent rounded up to 8 in every
    stored row.  Everything else is bf16 NaN: the rest of the leading dimension, the rows the map skips, ``gap`` elements
    between batch entries (a multiple of 8), GUARD_ROWS rows in front and behind -- which is where k lines >= K of a k-major
    operand and rows >= M (N) of a k-contiguous one would be read from."""
    assert ld_extra % 8 == 0 and gap % 8 == 0
    R, W = (rows, K) if kc else (K, rows)
    W8 = ceil8(W)
    ld = W8 + ld_extra
    sr = GR.map_rows(R, rmap)
    per = (int(sr.max()) + 1) * ld + gap
    base = GUARD_ROWS * ld
    nb = len(vals)
    buf = np.full(base + nb * per + GUARD_ROWS * ld, BF16_NAN, dtype=np.uint16)
    idx = base + sr[:, None] * ld + np.arange(W8)[None, :]
    for b, v in enumerate(vals):
        assert v.shape == (R, W)
        row = np.zeros((R, W8), dtype=np.uint16)
        row[:, :W] = bf16_bits(v)
        buf[idx + b * per] = row
    return buf, base, ld, per


# ----------------------------------------------------------------------------------------------------------- reference
def ref_call(c: Call) -> Call:
    """The call in gemm_ref's flag convention.  bf16 ABI: bit 0 accumulate, bit 2 atomics, bit 3 operands are bf16, bit 4 the
    batch is summed into one C, bits 8 - 11 diagnostics without an effect on the result; gemm_ref: bit 0 accumulate, bit 1 ReLU,
    bit 3 workspace mode, bit 4 summed batch.  Only accumulate and the summed batch change what C holds."""
    assert not c.flags & 2, "the bf16 entry point has no ReLU bit"
    return replace(c, flags=(c.flags & 1) | (16 if c.flags & 16 else 0), colsum_base=None)


def decode_operand(buf, src16: bool) -> np.ndarray:
    """The operand buffer as the values the MFMA multiplies (float64, so that gemm_ref converts nothing per batch entry)."""
    return (bf16_decode(buf) if src16 else bf16_round(buf)).astype(np.float64)


def reference_bf16(c: Call, a_buf, b_buf, c_buf, bias_buf=None, src16: Optional[bool] = None):
    """-> (C buffer afterwards (float64), mask of the C elements the call may write)."""
    if src16 is None:
        src16 = bool(c.flags & 8)
    out, _, valid = GR.reference(ref_call(c), decode_operand(a_buf, src16), decode_operand(b_buf, src16), c_buf, bias_buf)
    return out, valid


# --------------------------------------------------------------------------------------------------------------- route
class RouteBf16(NamedTuple):
    name: str
    nkt: int                    # k tiles of the call
    splits: int                 # K slices launched (the argument clamped to nkt)
    slice_tiles: Tuple[int, ...]  # k tiles of each slice; 0: the slice is launched and has nothing to multiply


def route_bf16(c: Call) -> RouteBf16:
    """Which kernel ss_gemm_bf16_batched launches: the ring kernel iff the operands are bf16, K is whole 64-deep tiles and the
    output is worth a 256 x 128 tile (M >= 128) or the batch is K-concatenated."""
    src16 = bool(c.flags & 8)
    ring = src16 and c.K % RBK == 0 and (c.M >= 128 or bool(c.flags & 16))
    bk = BK_B16 if src16 else BK_F32
    nkt = ceil_div(c.K, bk)
    splits = min(c.splits, nkt)
    per = ceil_div(nkt, splits)
    tiles = tuple(max(0, min(nkt, (s + 1) * per) - s * per) for s in range(splits))
    name = ("ring_kcat" if c.flags & 16 else "ring") if ring else ("staged_b16" if src16 else "staged_f32")
    return RouteBf16(name, nkt, splits, tiles)


def ring_grid(c: Call) -> int:
    """Workgroups of a ring launch."""
    r = route_bf16(c)
    return ceil_div(c.N, RBN) * ceil_div(c.M, RBM) * (1 if c.flags & 16 else c.batch) * r.splits


def xcd_contiguous_id(wg: int, nwg: int) -> int:
    """The tile workgroup ``wg`` of ``nwg`` takes: XCD wg % 8 owns a contiguous range."""
    xcd, q, r = wg & 7, nwg >> 3, nwg & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (wg >> 3)


# ---------------------------------------------------------------------------------------------------------- group plan
class GroupPlan(NamedTuple):
    units: int
    U: int                       # units (k tiles) per workgroup of the stream-K form
    workgroups: int              # of the stream-K form
    maxc: int                    # slab slots per output tile
    whole: bool                  # the launch takes the one-workgroup-per-tile form instead (``tiles`` workgroups, no slabs)
    ws_floats: int
    runs: List[List[Tuple[int, int, int, int]]]  # stream-K: per workgroup its runs (problem, tile of the problem, kt0, nk)
    tiles: int
    slots: List[List[Tuple[int, int]]]           # per workgroup, per run: (tile of the group, slot) the slab goes to
    counts: List[int]                            # per tile of the group: the slabs the reduce adds (its ``cnt``)


def group_plan(problems: Sequence[Tuple[int, int, int, int]], cus: int) -> GroupPlan:
    """``problems``: (M, N, K, batch) each, K a multiple of 64."""
    n = len(problems)
    assert 1 <= n <= GROUP_MAX
    nkt = [K // RBK for _, _, K, _ in problems]
    ntile = [ceil_div(N, RBN) * ceil_div(M, RBM) * batch for M, N, _, batch in problems]
    tbase, ubase = [0], [0]
    for t, k in zip(ntile, nkt):
        tbase.append(tbase[-1] + t)
        ubase.append(ubase[-1] + t * k)
    units, tiles = ubase[n], tbase[n]
    U = ceil_div(units, min(units, cus))
    maxc = (max(nkt) - 1) // U + 2
    wgs = ceil_div(units, U)
    whole = 2 * tiles >= cus and tiles <= cus
    runs, slots = [], []
    for w in range(wgs):
        u, u1 = w * U, min(units, (w + 1) * U)
        mine, where = [], []
        while u < u1:
            j = max(q for q in range(n) if u >= ubase[q])
            local = u - ubase[j]
            tile, kt0 = divmod(local, nkt[j])
            nk = min(nkt[j] - kt0, u1 - u)
            w_lo = (ubase[j] + tile * nkt[j]) // U
            mine.append((j, tile, kt0, nk))
            where.append((tbase[j] + tile, w - w_lo))
            u += nk
        runs.append(mine)
        slots.append(where)
    counts = []
    for j in range(n):
        for tile in range(ntile[j]):
            ustart = ubase[j] + tile * nkt[j]
            counts.append((ustart + nkt[j] - 1) // U - ustart // U + 1)
    return GroupPlan(units, U, wgs, maxc, whole, tiles * maxc * SLAB_FLOATS, runs, tiles, slots, counts)


# ------------------------------------------------------------------------------------------------------ the wrong map
def carry_free_rows(K: int, rmap: Sequence[int], starts: Sequence[int] = (0,)) -> np.ndarray:
    """Storage rows of k = 0 .. K-1 as a k-major loader WITHOUT the carry walks them: exact for the first 64 k lines of a slice
    (the division is done once, in front of the k loop), then + (64 / group) * gstride + 64 % group per 64-deep tile, whether or
    not the step crossed one group boundary more.  ``starts``: the first k of every K slice, ascending."""
    G, S, off = rmap
    inc = (RBK // G) * S + RBK % G
    k = np.arange(K, dtype=np.int64)
    starts = np.asarray(sorted(starts), dtype=np.int64)
    s0 = starts[np.searchsorted(starts, k, side="right") - 1]
    first = s0 + (k - s0) % RBK
    return (first // G) * S + first % G + off + ((k - s0) // RBK) * inc


def kmajor_products(c: Call, a_vals: np.ndarray, b_vals: np.ndarray, rows_a: np.ndarray, rows_b: np.ndarray) -> np.ndarray:
    """[batch][M][N] products of a call with two k-major operands when k line k is read from storage rows rows_a[k] / rows_b[k]
    (``a_vals`` / ``b_vals``: the decoded buffers).  A row outside a buffer counts as NaN."""
    out = []
    for b in range(c.batch):
        ia = c.a_base + b * c.stride_a + rows_a[:, None] * c.lda + np.arange(c.M)[None, :]
        ib = c.b_base + b * c.stride_b + rows_b[:, None] * c.ldb + np.arange(c.N)[None, :]
        A = np.where(ia < a_vals.size, a_vals[np.minimum(ia, a_vals.size - 1)].astype(np.float64), np.nan)
        B = np.where(ib < b_vals.size, b_vals[np.minimum(ib, b_vals.size - 1)].astype(np.float64), np.nan)
        out.append(A.T @ B)
    return np.stack(out)


def carry_matters(c: Call, a_vals, b_vals, starts: Sequence[int] = (0,)) -> bool:
    """True when a kernel that drops the carry would leave another C than the true one for this call (both operands k-major)."""
    assert not c.a_kc and not c.b_kc
    true = kmajor_products(c, a_vals, b_vals, GR.map_rows(c.K, c.ra), GR.map_rows(c.K, c.rb))
    assert np.isfinite(true).all()
    wrong = kmajor_products(c, a_vals, b_vals, carry_free_rows(c.K, c.ra, starts), carry_free_rows(c.K, c.rb, starts))
    return not np.array_equal(true, wrong)
