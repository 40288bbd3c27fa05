"""Host references for the GRU recurrences (csrc/gru.hip, gru_split.h, gru_bf16.hip, gru_bf16_pers.h): no GPU, torch on the CPU.

``direction`` / ``reference``  the masked bidirectional GRU the four kernel families compute, fed with the input projection
               ``gi`` directly.  In float64 it is the yardstick of the f32 kernels; with ``bf16=True`` it is float32 with the
               roundings of the bf16 kernels: bf16 W_hh, the previous state rounded to bf16 inside the product and -- through
               autograd's own backward of that rounding -- bf16 gradients on the way one step back.  ``reference`` returns what
               the kernels leave behind: ``out``, the stash (r, z, n, q = W_hn h + b_hn) on valid frames, ``d_g`` in the kernels'
               four-block layout (d a_r, d a_z, d a_n, d a_n * r) and the four bias gradients.
``f32_dispatch`` / ``bf16_dispatch``  a restatement of what the launchers choose for (B, T, H, CU count, CU cap set): parts,
               launched grid, workgroups, workspace bytes; for bf16 the clip chunks.  Written from the comments and formulas of
               gru_split.h, gru_bf16_pers.h and granule_xchg.h, so that a test can say which route it means to reach.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import torch

SLICE = 16               # clips per (slice, direction) = MFMA N (gru.hip SLICE, gru_bf16_pers.h PSLICE)
SYNC_HDR_WORDS = 64      # granule_xchg.h: header words in front of the granule sections
SPLIT_MAX_PARTS = 12     # gru_split.h: the XCD-id rows are laid out for the widest split
XCHG_MAX_T = 1022        # granule_xchg.h: step tags are 10 bits, 0 and 1023 are taken
PUNITS = 64              # gru_bf16_pers.h: hidden units per part
SPLIT_SLACK_CUS = 16     # gru_split.h split_max_wgs(): CUs left free by the f32 multi-CU form


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def bf(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and back.  Under autograd the gradient takes the same rounding on its way back."""
    return x.to(torch.bfloat16).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------ the recurrence
def direction(gi, whh, bhh, lengths, T, H, reverse, bf16=True):
    """One direction, differentiable.  gi (B, T, 3H), gate order r | z | n.  -> out (B, T, H), stash (B, T, 4, H), both zero on
    frames past a clip's end.  ``bf16``: the kernels' roundings -- bf16 W_hh and bf16 previous state inside the matmul, the
    dtype of ``gi`` elsewhere."""
    B = gi.shape[0]
    rnd = bf if bf16 else (lambda x: x)
    h = gi.new_zeros(B, H)
    outs = [None] * T
    saves = [None] * T
    wb = rnd(whh)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        valid = (lengths > t).to(gi.dtype).unsqueeze(1)
        gh = rnd(h) @ wb.t()
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H] + bhh[:H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H] + bhh[H:2 * H])
        hpre = gh[:, 2 * H:] + bhh[2 * H:]
        n = torch.tanh(gi[:, t, 2 * H:] + r * hpre)
        hn = (1 - z) * n + z * h
        h = valid * hn  # the kernel's state past a clip's end is zero (nothing valid follows in either direction)
        outs[t] = h
        saves[t] = torch.stack([r, z, n, hpre], 1) * valid.unsqueeze(2)
    return torch.stack(outs, 1), torch.stack(saves, 1)


class GruRef(NamedTuple):
    out: torch.Tensor     # (B, T, 2H)      forward direction in [:H], reverse in [H:]
    save: torch.Tensor    # (2, B, T, 4, H) r, z, n, q; zero on invalid frames
    d_g: torch.Tensor     # (2, B, T, 4, H) d a_r, d a_z, d a_n, d a_n * r; None without d_out
    g_bih: torch.Tensor   # (2, 3H) sums of (d a_r, d a_z, d a_n) over clips and frames
    g_bhh: torch.Tensor   # (2, 3H) the same with d a_n * r in the n block
    valid: torch.Tensor   # (B, T) bool
    g_whh: Sequence[torch.Tensor] = ()  # d W_hh per direction (what the d W_hh GEMM makes of d_g and out)


def reference(gi, whh: Sequence[torch.Tensor], bhh: Sequence[torch.Tensor], lengths, d_out=None, bf16=False) -> GruRef:
    """gi (2, B, T, 3H), whh / bhh one per direction, lengths (B,), d_out (B, T, 2H) = gradient w.r.t. ``out``.
    float64 throughout, or float32 with the bf16 kernels' roundings."""
    dt = torch.float32 if bf16 else torch.float64
    _, B, T, H3 = gi.shape
    H = H3 // 3
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    gi_l = [gi[d].to(dt).clone().requires_grad_(d_out is not None) for d in range(2)]
    w = [x.to(dt).clone().requires_grad_(d_out is not None) for x in whh]
    b = [x.to(dt).clone().requires_grad_(d_out is not None) for x in bhh]
    outs, saves = zip(*[direction(gi_l[d], w[d], b[d], lengths, T, H, bool(d), bf16=bf16) for d in range(2)])
    out = torch.cat(outs, 2)
    save = torch.stack([s.detach() for s in saves])
    valid = torch.arange(T)[None] < lengths[:, None]
    if d_out is None:
        return GruRef(out.detach(), save, None, None, None, valid)
    (out * d_out.to(dt)).sum().backward()
    d_g = torch.zeros(2, B, T, 4, H, dtype=dt)
    for d in range(2):
        d_g[d, :, :, :3] = gi_l[d].grad.view(B, T, 3, H)
        d_g[d, :, :, 3] = d_g[d, :, :, 2] * save[d, :, :, 0]  # d q = d a_n * r
    g_bih = d_g[:, :, :, :3].sum((1, 2)).reshape(2, 3 * H)
    g_bhh = torch.stack([x.grad for x in b])
    return GruRef(out.detach(), save, d_g, g_bih, g_bhh, valid, [x.grad for x in w])


# ------------------------------------------------------------------------------------------------------------ f32 dispatch
def sync_bytes(xid_granules: int, fwd_granules: int, bwd_granules: int) -> int:
    """SyncSections::bytes(): the header words, then three runs of 8-byte granules."""
    return SYNC_HDR_WORDS * 4 + (xid_granules + fwd_granules + bwd_granules) * 8


def split_max_wgs(cus: int) -> int:
    return cus - SPLIT_SLACK_CUS


def split_parts(B: int, T: int, H: int, cus: int) -> int:
    """gru_split_parts: six parts at H = 192, two at H = 64, while every live workgroup fits; 0 = the one-CU form."""
    pairs = 2 * ceil_div(B, SLICE)
    if T > XCHG_MAX_T:
        return 0
    P = {192: 6, 64: 2}.get(H, 0)
    return P if P and pairs * P <= split_max_wgs(cus) else 0


def split_small_parts(B: int, P: int, cus: int) -> int:
    """gru_split_small_parts: twelve parts at H = 192 where the grid padded to a multiple of 8 pairs still fits."""
    if P != 6:
        return P
    pad = ceil_div(2 * ceil_div(B, SLICE), 8) * 8
    return 12 if pad * 12 <= split_max_wgs(cus) else P


def split_grid_pairs(B: int, P: int, cus: int) -> int:
    """gru_split_grid_pairs: the next multiple of 8 pairs when that still fits the co-residency bound."""
    pairs = 2 * ceil_div(B, SLICE)
    pad = ceil_div(pairs, 8) * 8
    return pad if pad * P <= split_max_wgs(cus) else pairs


class F32Dispatch(NamedTuple):
    parts: int          # parts per (slice, direction) the kernels run with; 0 = one workgroup per (slice, direction)
    sized_parts: int    # parts ss_gru_sync_bytes lays the workspace out for (the CU cap does not reach it)
    pairs: int          # live (slice, direction) pairs
    grid_pairs: int     # launched pairs, the pad included
    workgroups: int     # of one launch; 0 in the one-CU form
    part_major: bool    # block numbering (xchg_ids): part-major when the launched pair count is a multiple of 8
    sync_bytes: int     # ss_gru_sync_bytes


def f32_dispatch(B: int, T: int, H: int, cus: int, cap_set: bool = False, workspace: bool = True) -> F32Dispatch:
    """What ss_gru_fwd_drop / ss_gru_bwd launch (gru_split_launch) and what ss_gru_sync_bytes reports."""
    pairs = 2 * ceil_div(B, SLICE)
    base = split_parts(B, T, H, cus)
    sized = split_small_parts(B, base, cus) if base else 0
    nbytes = 0
    if sized:
        nbytes = sync_bytes(ceil_div(pairs * SPLIT_MAX_PARTS, 8) * 8, 2 * pairs * SLICE * H, 2 * pairs * sized * SLICE * H)
    P = base if workspace else 0
    if P and not cap_set:
        P = split_small_parts(B, P, cus)
    gp = split_grid_pairs(B, P, cus) if P else 0
    return F32Dispatch(P, sized, pairs, gp, gp * P, bool(P) and gp % 8 == 0, nbytes)


def f32_launch_extent(d: F32Dispatch, H: int) -> Tuple[int, int, int]:
    """Granules a launch of ``d.parts`` parts can touch in the (XCD id, forward, backward) sections: only live pairs exchange
    (workgroups of the pad leave at once), indexed [pair][part], [2][pairs][16][H], [2][pairs][P][P][16][H / P]."""
    return d.pairs * d.parts, 2 * d.pairs * SLICE * H, 2 * d.pairs * d.parts * SLICE * H


def f32_sections(d: F32Dispatch, H: int) -> Tuple[int, int, int]:
    """Granules of the three sections of the workspace as ss_gru_sync_bytes sizes it (split_sync at the sized parts)."""
    return ceil_div(d.pairs * SPLIT_MAX_PARTS, 8) * 8, 2 * d.pairs * SLICE * H, 2 * d.pairs * d.sized_parts * SLICE * H


# ------------------------------------------------------------------------------------------------------------ bf16 dispatch
def pers_supported(H: int) -> bool:
    return 128 <= H <= 512 and H % 64 == 0


def pers_chunk_clips(B: int, H: int, cus: int) -> int:
    """Clips per persistent launch: as many slices as fit the chip with both directions and all H / 64 parts resident; equal
    chunks otherwise, rounded up to 4 slices (8 groups: part-major, same-XCD exchange) where that still fits."""
    P = H // PUNITS
    slices = cus // (2 * P)
    if slices < 1:
        return 0
    need = ceil_div(B, SLICE)
    if slices >= need:
        return B
    launches = ceil_div(need, slices)
    per = ceil_div(need, launches)
    if ceil_div(per, 4) * 4 <= slices:
        per = ceil_div(per, 4) * 4
    return per * SLICE


class Bf16Dispatch(NamedTuple):
    chunk: int                        # clips per persistent launch, 0 = the step kernels run the shape
    launches: List[Tuple[int, int]]   # (c0, nc) of every persistent launch of one call
    workgroups: List[int]             # of every launch
    sync_bytes: int                   # ss_gru_bf16_sync_bytes


def bf16_dispatch(B: int, T: int, H: int, cus: int) -> Bf16Dispatch:
    chunk = pers_chunk_clips(B, H, cus) if pers_supported(H) and T <= XCHG_MAX_T else 0
    if chunk <= 0:
        return Bf16Dispatch(0, [], [], 0)
    P = H // PUNITS
    launches = [(c0, min(chunk, B - c0)) for c0 in range(0, B, chunk)]
    groups = 2 * ceil_div(chunk, SLICE)
    nbytes = sync_bytes(ceil_div(groups * P, 8) * 8, 2 * groups * SLICE * (H // 2), 2 * groups * P * P * SLICE * (PUNITS // 2))
    return Bf16Dispatch(chunk, launches, [2 * ceil_div(nc, SLICE) * P for _, nc in launches], nbytes)


# ------------------------------------------------------------------------------------------------------------ the edges
# The dispatch edges of a 256-CU part (MI355X), worked by hand from the headers; tests/test_gru_ref_cpu.py holds the
# restatement above to them and the GPU edge tests hold the library to both.
# (H, B) -> parts, sized parts, live pairs, launched pairs, workgroups, part-major, at 256 CUs and T <= 1022, cap not set
F32_EDGES_256 = {
    (192, 1): (12, 12, 2, 8, 96, True),
    (192, 15): (12, 12, 2, 8, 96, True),
    (192, 16): (12, 12, 2, 8, 96, True),
    (192, 17): (12, 12, 4, 8, 96, True),       # the partial tail slice beside a full one; 4 pairs padded to 8
    (192, 49): (12, 12, 8, 8, 96, True),
    (192, 64): (12, 12, 8, 8, 96, True),       # 8 pairs: the pad adds nothing
    (192, 65): (12, 12, 10, 16, 192, True),    # 10 pairs padded to 16: 6 idle pairs, part-major numbering
    (192, 128): (12, 12, 16, 16, 192, True),   # the last batch on twelve parts, none idle
    (192, 129): (6, 6, 18, 24, 144, True),     # the first batch on six parts, 18 pairs padded to 24
    (192, 320): (6, 6, 40, 40, 240, True),     # on the co-residency bound; 40 pairs are a multiple of 8 themselves
    (192, 321): (0, 0, 42, 0, 0, False),       # 42 * 6 = 252 > 240: the one-CU form, no workspace
    (64, 1): (2, 2, 2, 8, 16, True),
    (64, 17): (2, 2, 4, 8, 16, True),
    (64, 960): (2, 2, 120, 120, 240, True),    # 120 pairs x 2 on the bound
    (64, 961): (0, 0, 122, 0, 0, False),
}

# (H, B) -> the (c0, nc) launches at 256 CUs
BF16_EDGES_256 = {
    (128, 1): [(0, 1)],
    (128, 17): [(0, 17)],
    (128, 1024): [(0, 1024)],                   # 64 slices x 2 directions x 2 parts = 256 workgroups
    (128, 1025): [(0, 576), (576, 449)],        # 65 slices in two launches: 33 each, rounded up to 36 <= 64
    (256, 512): [(0, 512)],
    (256, 513): [(0, 320), (320, 193)],         # 33 slices: 17 per launch rounded up to 20 <= 32
    (384, 336): [(0, 336)],                     # 21 slices x 2 x 6 = 252 workgroups
    (384, 337): [(0, 192), (192, 145)],
    (384, 641): [(0, 336), (336, 305)],         # 41 slices: 21 per launch, 24 would not fit 21 -- the round-up is not taken
    (512, 256): [(0, 256)],
    (512, 257): [(0, 192), (192, 65)],          # 17 slices: 9 per launch rounded up to 12; the rest is 5 slices, the last one clip
}
