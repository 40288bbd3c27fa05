"""GPU: every route of the bf16 GEMM family (csrc/gemm_bf16.hip) at its tile, ring and unit edges, bit for bit.

The bf16 counterpart of tests/test_gpu_gemm_routes.py.  Operands are small integers -- bf16 holds them exactly and
``gemm_ref.assert_exact_range`` shows for every case that no partial sum can reach 2**24 -- so every order of f32 additions (MFMA
chains, K slices with float atomics, stream-K slabs + reduce, the K-concatenated pairs) gives the same bits and each case is
compared with ``torch.equal`` against ``gemm_bf16_ref.reference_bf16``.  bf16 operands lie in buffers of bf16 NaN built by
``place_bf16`` on the host (zeros only where the ABI asks for them: from the extent to the extent rounded up to 8), f32 operands
in buffers of f32 NaN; C lies in a buffer of a sentinel that must be the same afterwards outside the M x N elements, the stream-K
workspace is NaN between two sentinel guards.  Every case names the kernel it means to reach and asserts that
``gemm_bf16_ref.route_bf16`` agrees; the ring and group cases run twice on the same buffers.

One float case per route bounds the error by ``gemm_ref.f32_bound``: the reference multiplies the bf16-rounded operands in
float64, a bf16 x bf16 product is exact in f32, so only the f32 accumulation is left.  Largest error / bound ratios measured on
an MI355X (every route stands on the bound as ``f32_bound`` gives it, none needed the factor 2 of a truncating MFMA sum):
staged_f32 0.0040, staged_b16 0.0046 - 0.0058 (two runs: the order of the K slices' atomics), ring 0.0029, ring_kcat 0.0029, group stream-K 0.0024, group whole 0.0078.

ss_cvt_bf16_rows takes ``cols % 4 == 0`` only (include/ss_hotpath.h): the column counts 1, 7 and 9 are asserted to be refused with
the destination untouched, 4, 8, 12 and 100 are converted.
"""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

import gemm_bf16_ref as BR
import gemm_ref as GR
from gemm_bf16_ref import ceil8
from gemm_ref import IDENT, INT_MAX, Call, ceil_div
from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8
SENT = -77.0
NAN = float("nan")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]
SS_ERR_ARG, SS_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def cus(L):
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------------------ placing
@dataclass
class Spec:
    route: str
    a_kc: int
    b_kc: int
    M: int
    N: int
    K: int
    src16: int = 1
    a_ld: int = 0       # leading dimension beyond the extent rounded up to 8 (bf16: 0 / 8 / 16) or to 4 (f32: 0 / 4 / 8)
    b_ld: int = 0
    c_pad: int = 0      # ldc - N
    c_off: int = 0      # floats C's base lies off 16-byte alignment
    ra: Tuple[int, int, int] = IDENT
    rb: Tuple[int, int, int] = IDENT
    bias: bool = False
    bias_stride: Optional[int] = None   # default: N
    flags: int = 0                      # without bit 3, which follows src16
    splits: int = 1
    batch: int = 1
    share_a: bool = False               # stride_a = 0
    share_b: bool = False
    a_gap: int = 0                      # NaN elements between batch entries
    b_gap: int = 0
    c_gap: int = 0                      # stride_c = M * ldc + c_gap
    kind: str = "int"                   # "int" | "real" | "tie" (A: odd integers 257 .. 511, B: -1 / 0 / 1)


def values(nb, shape, seed, kind, hi=4):
    """nb arrays of ``shape``; entry b depends on (seed, b) alone."""
    out = []
    for b in range(nb):
        rng = np.random.default_rng(seed + 7919 * b)
        if kind == "real":
            out.append(rng.standard_normal(shape).astype(np.float32))
        elif kind == "tieA":
            out.append((257 + 2 * rng.integers(0, 128, size=shape)).astype(np.float32))
        elif kind == "tieB":
            out.append(rng.integers(-1, 2, size=shape).astype(np.float32))
        else:
            out.append(GR.int_operands(shape, seed + 7919 * b, -hi, hi))
    return out


def place_f32(kc, rows, K, extra, rmap, vals, gap=0):
    """f32 operands inside a buffer of NaN: -> (buffer, element offset of the first, ld, stride).  ld = extent + extra."""
    R, W = (rows, K) if kc else (K, rows)
    assert W % 4 == 0 and extra % 4 == 0 and gap % 4 == 0
    ld = W + extra
    sr = GR.map_rows(R, rmap)
    per = (int(sr.max()) + 1) * ld + gap
    base = GUARD_ROWS * ld
    buf = np.full(base + len(vals) * per + GUARD_ROWS * ld, NAN, dtype=np.float32)
    idx = base + sr[:, None] * ld + np.arange(W)[None, :]
    for b, v in enumerate(vals):
        buf[idx + b * per] = v
    return buf, base, ld, per


def place_out(rows, cols, pad, nb, off, gap, seed, kind, filled):
    """C: nb blocks of [rows][cols + pad] inside a buffer of the sentinel; its base lies ``off`` floats behind a multiple of 4 (the
    device allocation is 16-byte aligned).  ``filled``: the blocks hold values (a C that is accumulated into), else the sentinel."""
    ld = cols + pad
    per = rows * ld
    stride = per + gap
    base = (GUARD_ROWS * ld + 3) // 4 * 4 + off
    buf = np.full(base + (nb - 1) * stride + per + GUARD_ROWS * ld, SENT, dtype=np.float32)
    if filled:
        vals = values(nb, (rows, cols), seed, "real" if kind == "real" else "int")
        idx = base + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        for b in range(nb):
            buf[idx + b * stride] = vals[b]
    return buf, base, ld, stride


@dataclass
class Plan:
    call: Call
    a: np.ndarray       # uint16 (bf16 source) or float32
    b: np.ndarray
    c: np.ndarray
    bias: Optional[np.ndarray]
    src16: bool


def plan(s: Spec, seed: int) -> Plan:
    """Host side of a case: the buffers and the call that points into them."""
    kcat = bool(s.flags & 16)
    ka, kb = ("tieA", "tieB") if s.kind == "tie" else (s.kind, s.kind)
    a_vals = values(1 if s.share_a else s.batch, (s.M, s.K) if s.a_kc else (s.K, s.M), seed, ka)
    b_vals = values(1 if s.share_b else s.batch, (s.N, s.K) if s.b_kc else (s.K, s.N), seed + 1, kb)
    if s.src16:
        a, a_base, lda, a_per = BR.place_bf16(s.a_kc, s.M, s.K, s.a_ld, s.ra, a_vals, s.a_gap)
        b, b_base, ldb, b_per = BR.place_bf16(s.b_kc, s.N, s.K, s.b_ld, s.rb, b_vals, s.b_gap)
    else:
        a, a_base, lda, a_per = place_f32(s.a_kc, s.M, s.K, s.a_ld, s.ra, a_vals, s.a_gap)
        b, b_base, ldb, b_per = place_f32(s.b_kc, s.N, s.K, s.b_ld, s.rb, b_vals, s.b_gap)
    c, c_base, ldc, c_stride = place_out(s.M, s.N, s.c_pad, 1 if kcat else s.batch, s.c_off, s.c_gap, seed + 2, s.kind, bool(s.flags & 1))
    bias = bias_base = None
    bstride = s.bias_stride if s.bias_stride is not None else (s.N if s.batch > 1 and not kcat else 0)
    if s.bias:
        nb = 1 if bstride == 0 else s.batch
        bias = np.full(3 + (nb - 1) * bstride + s.N + 5, NAN, dtype=np.float32)
        bias_base = 3
        v = values(nb, (s.N,), seed + 3, "real" if s.kind == "real" else "int", 9)
        for k in range(nb):
            bias[3 + k * bstride: 3 + k * bstride + s.N] = v[k]
    call = Call(s.a_kc, s.b_kc, s.M, s.N, s.K, lda, ldb, ldc, ra=s.ra, rb=s.rb, flags=s.flags | (8 if s.src16 else 0), splits=s.splits,
                batch=s.batch, stride_a=0 if s.share_a else a_per, stride_b=0 if s.share_b else b_per, stride_c=c_stride,
                stride_bias=bstride if s.bias else 0, a_base=a_base, b_base=b_base, c_base=c_base, bias_base=bias_base)
    return Plan(call, a, b, c, bias, bool(s.src16))


def magnitudes(p: Plan):
    """Per C: (op(A) concatenated along K over everything summed into it, op(B) likewise, C0, bias), as the MFMA sees them."""
    c = BR.ref_call(p.call)
    av, bv = BR.decode_operand(p.a, p.src16), BR.decode_operand(p.b, p.src16)
    out = []
    groups = [list(range(c.batch))] if c.flags & 16 else [[b] for b in range(c.batch)]
    for g in groups:
        A = np.concatenate([GR.gather_a(c, av, b) for b in g], 1)
        B = np.concatenate([GR.gather_b(c, bv, b) for b in g], 0)
        c0 = p.c.astype(np.float64)[GR.c_index(c, g[0])] if c.flags & 1 else None
        bias = None if p.bias is None else p.bias.astype(np.float64)[c.bias_base + g[0] * c.stride_bias + np.arange(c.N)]
        out.append((A, B, c0, bias))
    return out


def check_exact(p: Plan):
    for A, B, c0, bias in magnitudes(p):
        GR.assert_exact_range([(A, B)], c0, bias)


def to_dev(x):
    if x is None:
        return None
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda()


def dptr(t, base):
    return None if t is None else t.data_ptr() + t.element_size() * base


def batched_args(L, c: Call, a_d, b_d, c_d, bias_d):
    return (c.a_kc, c.b_kc, c.M, c.N, c.K, dptr(a_d, c.a_base), c.lda, *c.ra, dptr(b_d, c.b_base), c.ldb, *c.rb, dptr(c_d, c.c_base), c.ldc,
            dptr(bias_d, c.bias_base or 0), c.flags, c.splits, c.batch, c.stride_a, c.stride_b, c.stride_c, c.stride_bias, L.stream())


def same_bits(name, got, want, mask):
    """torch.equal on the elements a call may write, and on everything around them."""
    got_t, want_t, m = torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(mask)
    assert torch.equal(got_t[~m], want_t[~m]), f"{name}: an element outside the M x N of C changed"
    if not torch.equal(got_t[m], want_t[m]):
        bad = np.flatnonzero(mask & ~((got == want) | (np.isnan(got) & np.isnan(want))))
        pytest.fail(f"{name}: {bad.size} of {int(mask.sum())} elements differ, first at flat {bad[0]}: got {got[bad[0]]}, "
                    f"want {want[bad[0]]}", pytrace=False)


def unchanged(t, host):
    return torch.equal(t.cpu().view(torch.int16), torch.from_numpy(host).view(torch.int16))


def run_case(L, s: Spec, seed: int, reps: Optional[int] = None):
    """ss_gemm_bf16_batched against the reference.  -> (device C as numpy, plan, reference, valid mask, route)."""
    p = plan(s, seed)
    c = p.call
    if s.kind != "real":
        check_exact(p)
    r = BR.route_bf16(c)
    assert r.name == s.route, f"meant for {s.route}, the dispatcher takes {r.name}"
    want, valid = BR.reference_bf16(c, p.a, p.b, p.c, p.bias)
    assert np.isfinite(want).all(), "the reference read padding: the case is built wrongly"
    a_d, b_d, c_d, bias_d = to_dev(p.a), to_dev(p.b), to_dev(p.c), to_dev(p.bias)
    args = batched_args(L, c, a_d, b_d, c_d, bias_d)
    assert dptr(a_d, c.a_base) % 16 == 0 and dptr(b_d, c.b_base) % 16 == 0 and dptr(c_d, c.c_base) % 16 == 4 * s.c_off
    c0 = c_d.clone()
    for rep in range(reps if reps else (2 if r.name.startswith("ring") else 1)):
        c_d.copy_(c0)
        L.call("ss_gemm_bf16_batched", *args)
        torch.cuda.synchronize()
        got = c_d.cpu().numpy()
        if s.kind != "real":
            same_bits(f"C (run {rep})", got, want.astype(np.float32), valid)
    assert unchanged(a_d, p.a) and unchanged(b_d, p.b), "the operands are inputs"
    return got, p, want, valid, r


def ids(specs):
    return [f"{i:02d}-{s.route}-{'kc' if s.a_kc else 'km'}x{'kc' if s.b_kc else 'km'}-{s.M}x{s.N}x{s.K}-f{s.flags}s{s.splits}b{s.batch}"
            for i, s in enumerate(specs)]


# ------------------------------------------------------------------------------------------------- tile edges, staged
def staged_specs():
    out = []
    Ms, Ns, Ks = [1, 4, 63, 64, 65, 124, 127], [1, 8, 127, 128, 129, 136], [1, 7, 8, 9, 63, 65, 70, 129]
    for i in range(56):   # every (M, K) pair (7 and 8 are coprime); a chunk that starts inside K and ends in the zero padding
        a_kc, b_kc = LAYOUTS[(i // 8 + i) % 4]
        out.append(Spec("staged_b16", a_kc, b_kc, Ms[i % 7], Ns[(i // 7 + i) % 6], Ks[i % 8], a_ld=[0, 8, 16][i % 3], b_ld=[0, 8, 16][(i // 3) % 3],
                        c_pad=[0, 1, 4][(i // 2) % 3], c_off=(i // 4) % 2, bias=i % 2 == 0, flags=(i // 2) % 2))
    # whole 64-deep k tiles stay here while M < 128 (test_dispatch_boundary has the ring side)
    out += [Spec("staged_b16", *LAYOUTS[i], 127, 136, K, a_ld=8, bias=True, flags=i % 2) for i, K in enumerate([64, 128, 64, 128])]
    # f32 operands, 32-deep k tiles: contiguous extents are multiples of 4
    M4, N4, Mf, Nf, K4 = [4, 60, 64, 68, 124, 128, 132], [4, 8, 124, 128, 132, 136], [1, 4, 63, 64, 65, 124, 127], [1, 8, 127, 128, 129, 136], [4, 28, 32, 36, 64, 68]
    for i in range(42):   # every (M, K) pair
        a_kc, b_kc = LAYOUTS[(i // 6 + i) % 4]
        out.append(Spec("staged_f32", a_kc, b_kc, (Mf if a_kc else M4)[i % 7], (Nf if b_kc else N4)[(i // 7 + i) % 6], K4[i % 6], src16=0,
                        a_ld=[0, 4, 8][i % 3], b_ld=[0, 4, 8][(i // 3) % 3], c_pad=[0, 1, 4][(i // 2) % 3], c_off=(i // 4) % 2, bias=i % 2 == 1,
                        flags=(i // 2) % 2))
    return out


STAGED = staged_specs()


@pytest.mark.parametrize("s", STAGED, ids=ids(STAGED))
def test_staged_tile_edges(L, s):
    run_case(L, s, 1000 + STAGED.index(s))


# --------------------------------------------------------------------------------------------------- tile edges, ring
def ring_specs():
    out = []
    Ms, Ns, Ks = [128, 129, 255, 256, 257, 260], [1, 8, 127, 128, 129, 136, 256], [64, 128, 192, 256, 320]
    for i in range(42):   # every (M, N) pair; 1 to 5 k tiles: start-up, refill and the wrap of the three stages
        a_kc, b_kc = LAYOUTS[(i // 4 + i) % 4]
        out.append(Spec("ring", a_kc, b_kc, Ms[i % 6], Ns[i % 7], Ks[(i // 6 + i) % 5], a_ld=[0, 8, 16][i % 3], b_ld=[0, 8, 16][(i // 3) % 3],
                        bias=i % 2 == 0, flags=(i // 2) % 2, c_pad=[0, 4, 1][(i // 5) % 3]))
    return out


RING = ring_specs()


@pytest.mark.parametrize("s", RING, ids=ids(RING))
def test_ring_tile_edges(L, s):
    run_case(L, s, 2000 + RING.index(s))


@pytest.mark.parametrize("wgs,M,N,batch", [(1, 128, 8, 1), (2, 128, 8, 2), (7, 128, 8, 7), (8, 257, 129, 2), (9, 128, 8, 9), (12, 257, 136, 3)])
def test_ring_grids_map_workgroups_to_tiles_one_to_one(L, wgs, M, N, batch):
    """xcd_contiguous_id over grids of 1, 2, 7, 8, 9 (and 12) workgroups: a tile done twice or not at all shows in C."""
    s = Spec("ring", 0, 1, M, N, 128, batch=batch, bias=True, c_gap=3, a_gap=8)
    assert BR.ring_grid(plan(s, 0).call) == wgs
    assert sorted(BR.xcd_contiguous_id(w, wgs) for w in range(wgs)) == list(range(wgs))
    run_case(L, s, 2100 + wgs)


@pytest.mark.parametrize("bit", [1024, 2048])
def test_ring_diagnostic_bits_give_the_same_bits(L, bit):
    """1024: both wave groups in step; 2048: tiles as dispatched."""
    s = Spec("ring", 1, 0, 257, 136, 320, batch=2, bias=True, flags=1, c_pad=4)
    plain, *_ = run_case(L, s, 2200)
    diag, *_ = run_case(L, replace(s, flags=1 | bit), 2200)
    assert torch.equal(torch.from_numpy(plain), torch.from_numpy(diag))


def test_dispatch_boundary(L):
    """Both sides of the dispatcher's thresholds, each exact against the reference: M = 127 (staged) against 128 (ring) at K = 64 and
    128, K = 127 / 129 at M = 128 (staged: no whole k tiles), f32 operands at a ring-sized shape (staged)."""
    for K in (64, 128):
        lo, p_lo, *_ = run_case(L, Spec("staged_b16", 1, 0, 127, 136, K, bias=True), 2300)
        hi, p_hi, *_ = run_case(L, Spec("ring", 1, 0, 128, 136, K, bias=True), 2300)
        assert lo[GR.c_index(p_lo.call, 0)].shape == (127, 136) and hi[GR.c_index(p_hi.call, 0)].shape == (128, 136)
    for K in (127, 129):
        run_case(L, Spec("staged_b16", 0, 0, 128, 136, K), 2310 + K)
    run_case(L, Spec("staged_f32", 0, 0, 128, 136, 128, src16=0), 2320)


# ------------------------------------------------------------------------------------------------------ ring epilogues
def epilogue_specs():
    out = []
    i = 0
    for N in (136, 256):           # 136: a full and a ragged column tile in one launch
        for c_pad in (0, 1, 4):
            for c_off in (0, 1):
                for flags in (0, 1, 5):   # store, accumulate, atomics
                    out.append(Spec("ring", *LAYOUTS[i % 4], 260, N, 128, c_pad=c_pad, c_off=c_off, flags=flags, batch=2, bias=i % 3 != 2,
                                    bias_stride=[0, None, None][i % 3], c_gap=4 * (i % 2)))
                    i += 1
    return out


EPILOGUE = epilogue_specs()


def lds_epilogue(c: Call, b: int) -> bool:
    """Whether batch entry b's full column tiles leave through the LDS image: no atomics, ldc % 4 == 0, C of the entry 16-byte aligned."""
    return not c.flags & 4 and c.splits == 1 and c.ldc % 4 == 0 and (c.c_base + b * c.stride_c) % 4 == 0


@pytest.mark.parametrize("s", EPILOGUE, ids=[f"{x}-ldc+{s.c_pad}-off{s.c_off}" for x, s in zip(ids(EPILOGUE), EPILOGUE)])
def test_ring_epilogues(L, s):
    run_case(L, s, 3000 + EPILOGUE.index(s))


def test_ring_epilogue_selection_is_covered():
    paths = {(lds_epilogue(p.call, 0), s.c_pad, s.c_off, s.flags) for s in EPILOGUE for p in [plan(s, 0)]}
    assert (True, 0, 0, 0) in paths and (True, 4, 0, 1) in paths           # the LDS image: store and accumulate
    assert {(False, 1, 0, 0), (False, 0, 1, 0), (False, 4, 1, 1), (False, 0, 0, 5)} <= paths   # ldc % 4, alignment, atomics


@pytest.mark.parametrize("flags", [0, 1])
def test_ring_epilogue_stride_c_misaligns_entry_1_only(L, flags):
    s = Spec("ring", 0, 0, 260, 256, 64, c_pad=4, c_gap=1, batch=3, flags=flags, bias=True)
    c = plan(s, 0).call
    assert [lds_epilogue(c, b) for b in range(3)] == [True, False, False]
    run_case(L, s, 3100 + flags)


# ------------------------------------------------------------------------------------------------------------ K slices
def slice_specs():
    out = []
    i = 0
    for nkt, splits in [(5, 4), (5, 5), (5, 9), (3, 2), (2, 2)]:
        for route in ("staged_f32", "staged_b16", "ring"):
            a_kc, b_kc = LAYOUTS[i % 4]
            K = {"staged_f32": 32 * nkt, "staged_b16": 64 * nkt - (0 if i % 2 else 31), "ring": 64 * nkt}[route]
            M = {"staged_f32": 132, "staged_b16": 65, "ring": 260}[route]
            if route == "staged_f32" and ((a_kc or b_kc) and K % 4):
                K -= K % 4
            out.append(Spec(route, a_kc, b_kc, M, 136, K, src16=route != "staged_f32", flags=1 if i % 3 else 5, splits=splits, batch=2, bias=True,
                            c_gap=5, c_pad=i % 2, a_gap=8 * (i % 2)))
            i += 1
    return out


SLICES = slice_specs()


@pytest.mark.parametrize("s", SLICES, ids=ids(SLICES))
def test_k_slices(L, s):
    """Atomics into a C of integers; the bias once, not once per slice; an empty last slice adds nothing."""
    _, p, _, _, r = run_case(L, s, 4000 + SLICES.index(s), reps=2)
    nkt = ceil_div(s.K, 64 if s.src16 else 32)
    assert r.nkt == nkt and r.splits == min(s.splits, nkt) and sum(r.slice_tiles) == nkt


def test_k_slices_include_an_empty_slice_on_every_kernel():
    empty = {s.route for s in SLICES if 0 in BR.route_bf16(plan(s, 0).call).slice_tiles}
    assert empty == {"staged_f32", "staged_b16", "ring"}
    assert any(BR.route_bf16(plan(s, 0).call) == BR.RouteBf16("ring", 5, 4, (2, 2, 1, 0)) for s in SLICES)
    assert any(BR.route_bf16(plan(s, 0).call).splits == 5 and s.splits == 9 for s in SLICES)


# -------------------------------------------------------------------------------------------------------------- remap
# (group, gstride, off) of A / of B; the pairs are dG[b][t] with h[b][t - 1]
MAPS = [((5, 6, 1), (5, 6, 0)), ((29, 30, 1), (29, 30, 0)), ((7, 9, 2), (7, 9, 2)), ((63, 64, 0), (63, 64, 0)), ((65, 66, 1), (65, 66, 1)),
        ((3, 4, 0), (3, 4, 0)), ((8, 9, 1), (8, 9, 1))]
DIVIDING = (8, 9, 1)


def slice_starts(c: Call):
    r = BR.route_bf16(c)
    per = ceil_div(r.nkt, r.splits)
    return tuple(64 * per * s for s in range(r.splits) if r.slice_tiles[s])


def assert_carry_sensitivity(c: Call, a, b, starts):
    """A non-dividing group: a kernel that never applies the carry would give another C.  (8, 9, 1): it would not -- the control."""
    matters = BR.carry_matters(c, BR.bf16_decode(a), BR.bf16_decode(b), starts)
    assert matters == (64 % c.ra[0] != 0), f"group {c.ra[0]}: carry matters {matters}"


@pytest.mark.parametrize("route", ["staged_b16", "ring"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("ra,rb", MAPS, ids=[f"g{a[0]}" for a, _ in MAPS])
def test_remap_carry(L, route, splits, ra, rb):
    """k-major pairs whose group does not divide 64: the incremental row walk of TileLoader16::load / ring::Operand::piece has to
    carry.  K = 64 groups (1856 for group 29: above the size cap on purpose, tiny M x N); slices start in the middle of a group; the
    rows the map skips are NaN."""
    M = 128 if route == "ring" else 8
    K = 64 * ra[0] * (2 if ra[0] < 5 else 1)   # (group 3: six k tiles, so that each of three slices still steps once)
    s = Spec(route, 0, 0, M, 8, K, ra=ra, rb=rb, flags=1 if splits > 1 else 0, splits=splits, batch=2, a_gap=8, b_ld=8, c_pad=1)
    p = plan(s, 5000)
    assert_carry_sensitivity(p.call, p.a, p.b, slice_starts(p.call))
    if splits == 3 and 64 % ra[0]:
        assert any(k % ra[0] for k in slice_starts(p.call)), "no slice starts inside a group"
    run_case(L, s, 5000)


@pytest.mark.parametrize("ra,rb", MAPS, ids=[f"g{a[0]}" for a, _ in MAPS])
def test_remap_staged_b16_ragged_k(L, ra, rb):
    """13 groups: K is no multiple of 64, the last tile is ragged as well."""
    s = Spec("staged_b16", 0, 0, 65, 8, 13 * ra[0], ra=ra, rb=rb, flags=1, splits=2, a_ld=8)
    p = plan(s, 5100)
    if s.K > 128:
        assert_carry_sensitivity(p.call, p.a, p.b, slice_starts(p.call))
    run_case(L, s, 5100)


@pytest.mark.parametrize("ra,rb", MAPS, ids=[f"g{a[0]}" for a, _ in MAPS])
def test_remap_without_a_walk(L, ra, rb):
    """The f32-source kernel maps every k line on its own, a k-contiguous operand has its rows mapped once in init."""
    run_case(L, Spec("staged_f32", 0, 0, 8, 8, 13 * ra[0], src16=0, ra=ra, rb=rb, flags=1, splits=3, a_ld=4), 5200)
    run_case(L, Spec("staged_b16", 1, 1, 37, 22, 70, ra=ra, rb=rb, a_ld=8, bias=True), 5201)
    run_case(L, Spec("ring", 1, 0, 130, 136, 128, ra=ra, flags=1, splits=2), 5202)
    run_case(L, Spec("ring", 0, 1, 130, 136, 64, rb=rb), 5203)


# ------------------------------------------------------------------------------------------------- kcat, shared operands
KCAT = [Spec("ring_kcat", *LAYOUTS[i % 4], M, 136, 128, flags=16, batch=2 + i % 2, bias=True, a_gap=16, b_gap=8, c_pad=[0, 4, 1][i % 3],
             a_ld=8 * (i % 2)) for i, M in enumerate([8, 127, 128, 300, 8, 127, 128, 300])]


@pytest.mark.parametrize("s", KCAT, ids=ids(KCAT))
def test_k_concatenation(L, s):
    """batch (A, B) pairs summed into one C by plain stores over the sentinel; one bias; NaN between the pairs."""
    got, p, want, valid, _ = run_case(L, s, 6000 + KCAT.index(s))
    assert int(valid.sum()) == s.M * s.N and (p.c == SENT).all()


SHARED = [Spec("staged_b16", 1, 0, 65, 136, 70, batch=3, share_a=True, bias=True), Spec("staged_b16", 0, 1, 65, 136, 70, batch=3, share_b=True, flags=1),
          Spec("ring", 1, 0, 130, 136, 128, batch=3, share_a=True, bias=True, b_gap=8), Spec("ring", 0, 0, 130, 136, 192, batch=3, share_b=True, flags=1, a_gap=8)]


@pytest.mark.parametrize("s", SHARED, ids=ids(SHARED))
def test_shared_operands(L, s):
    _, p, *_ = run_case(L, s, 6100 + SHARED.index(s))
    assert (p.call.stride_a == 0) == s.share_a and (p.call.stride_b == 0) == s.share_b


# -------------------------------------------------------------------------------------------------------- stream-K group
WS_GUARD = 64


def gp(M, N, K, batch, maps=None, c_pad=2, c_off=0, c_gap=6, a_ld=0, b_ld=8, kind="int"):
    ra, rb = maps if maps else (IDENT, IDENT)
    return Spec("", 0, 0, M, N, K, ra=ra, rb=rb, flags=1, batch=batch, c_pad=c_pad, c_off=c_off, c_gap=c_gap, a_ld=a_ld, b_ld=b_ld, a_gap=8, kind=kind)


def run_group(L, cus, specs, seed, whole=None, reps=2, exact=True):
    """ss_gemm_bf16_splitk_group against the reference.  -> (per problem (C, plan, reference, valid), the plan of the group)."""
    plans = [plan(s, seed + 10 * j) for j, s in enumerate(specs)]
    gpl = BR.group_plan([(s.M, s.N, s.K, s.batch) for s in specs], cus)
    if whole is not None:
        assert gpl.whole == whole, f"meant for the {'whole' if whole else 'stream-K'} form on {cus} CUs"
    devs, probs, wants = [], [], []
    for p in plans:
        if exact:
            check_exact(p)
        c = p.call
        a_d, b_d, c_d = to_dev(p.a), to_dev(p.b), to_dev(p.c)
        devs.append((a_d, b_d, c_d, c_d.clone()))
        probs.append(L.GemmProblem(0, 0, c.M, c.N, c.K, dptr(a_d, c.a_base), c.lda, *c.ra, dptr(b_d, c.b_base), c.ldb, *c.rb,
                                   dptr(c_d, c.c_base), c.ldc, 1, c.batch, c.stride_a, c.stride_b, c.stride_c))
        want, valid = BR.reference_bf16(replace(c, flags=8 | 1), p.a, p.b, p.c)
        assert np.isfinite(want).all()
        wants.append((want, valid))
    need = L.gemm_group_ws_floats(probs, bf16=True)
    assert need == gpl.ws_floats
    have = 4 if gpl.whole else need      # one workgroup per tile stores no slabs: four floats document that none is needed
    ws = torch.full((WS_GUARD + have + WS_GUARD,), NAN, device="cuda")
    ws[:WS_GUARD] = SENT
    ws[WS_GUARD + have:] = SENT
    arr, n = L.gemm_group(probs)
    for rep in range(reps):
        for _, _, c_d, c0 in devs:
            c_d.copy_(c0)
        L.call("ss_gemm_bf16_splitk_group", arr, n, ws.data_ptr() + 4 * WS_GUARD, have, L.stream())
        torch.cuda.synchronize()
        assert bool((ws[:WS_GUARD] == SENT).all()) and bool((ws[WS_GUARD + have:] == SENT).all()), "wrote outside the workspace"
        if gpl.whole:
            assert bool(torch.isnan(ws[WS_GUARD:WS_GUARD + have]).all()), "the whole form wrote a slab"
        out = []
        for j, (p, (a_d, b_d, c_d, _), (want, valid)) in enumerate(zip(plans, devs, wants)):
            got = c_d.cpu().numpy()
            if exact:
                same_bits(f"problem {j} (run {rep})", got, want.astype(np.float32), valid)
            assert unchanged(a_d, p.a) and unchanged(b_d, p.b)
            out.append((got, p, want, valid))
    return out, gpl


def need_cus(cus, n):
    """The group cases are built from the CU count; on a device too small for the structure a case is about, say so."""
    if cus < n:
        pytest.skip(f"the case needs at least {n} compute units to have the structure it is about; this device has {cus}")


def test_group_fewer_units_than_cus(L, cus):
    """(a) U = 1: every workgroup one k tile, every tile nkt slabs."""
    need_cus(cus, 11)
    specs = [gp(8, 8, 192, 1), gp(257, 129, 128, 1)]
    _, g = run_group(L, cus, specs, 7000, whole=False)
    assert g.units == 11 and g.U == 1 and g.maxc == 4 and g.workgroups == 11


def test_group_runs_cross_tiles_and_problems(L, cus):
    """(b) units just above the CU count: U = 2 against 11 k tiles -- runs end inside tiles, cross into the next tile and from
    the problem of one k tile per tile into the one of 11."""
    need_cus(cus, 64)
    nb = ceil_div(cus + 4 - 3, 11)
    specs = [gp(8, 8, 64, 3), gp(8, 8, 704, nb)]
    _, g = run_group(L, cus, specs, 7100, whole=False)
    assert cus < g.units <= cus + 14 and g.U == 2
    assert any({j for j, *_ in runs} == {0, 1} for runs in g.runs), "no run crosses from problem 0 into problem 1"
    assert any(len(runs) == 2 and runs[0][0] == runs[1][0] == 1 for runs in g.runs), "no run crosses tiles"
    assert any(kt0 > 0 for runs in g.runs for _, _, kt0, _ in runs)


def test_group_of_eight(L, cus):
    """(c) GROUP_MAX problems, ragged tiles in M and N."""
    Ms, Ns = [8, 256, 257], [8, 128, 129]
    specs = [gp(Ms[j % 3], Ns[(j // 3 + j) % 3], 64 * (1 + (3 * j) % 5), 1 + j % 2, c_pad=j % 3, c_off=j % 2) for j in range(8)]
    _, g = run_group(L, cus, specs, 7200)
    assert g.tiles == sum(ceil_div(s.M, 256) * ceil_div(s.N, 128) * s.batch for s in specs)


@pytest.mark.parametrize("which", ["half-1", "half", "cus", "cus+1"])
def test_group_whole_thresholds(L, cus, which):
    """(d) one workgroup per tile iff 2 * tiles >= cus and tiles <= cus: both sides of both thresholds, tiny problems."""
    need_cus(cus, 3)   # (one or two CUs have no half - 1)
    half = ceil_div(cus, 2)
    tiles, whole = {"half-1": (half - 1, False), "half": (half, True), "cus": (cus, True), "cus+1": (cus + 1, False)}[which]
    run_group(L, cus, [gp(8, 8, 128, tiles, c_gap=2)], 7300, whole=whole)


def test_group_whole_with_two_problems_and_ragged_tiles(L, cus):
    """The whole form selects its problem by tile: tbase, not ubase."""
    need_cus(cus, 16)
    nb = ceil_div(cus, 2) - 4
    run_group(L, cus, [gp(257, 129, 192, 1, c_off=1), gp(8, 8, 128, nb), gp(130, 136, 64, 1, c_pad=4, c_off=0)], 7400, whole=True)


def test_group_ldc_and_offset(L, cus):
    """(e) ldc > N and a C off 16-byte alignment, accumulated into integers."""
    run_group(L, cus, [gp(130, 136, 320, 2, c_pad=5, c_off=3, c_gap=7), gp(8, 129, 128, 1, c_pad=1, c_off=1)], 7500)


@pytest.mark.parametrize("form", ["stream-K", "whole"])
@pytest.mark.parametrize("ra,rb", MAPS, ids=[f"g{a[0]}" for a, _ in MAPS])
def test_group_remap_carry(L, cus, form, ra, rb):
    """The group kernel walks remapped rows through ring::Operand::piece in both its forms, every group of MAPS.  Stream-K:
    cus / 2 - 1 tiles of 64 groups each, so that runs are several k tiles long and start at kt0 > 0."""
    need_cus(cus, 16)
    tiles = cus if form == "whole" else ceil_div(cus, 2) - 1
    s = gp(8, 8, 64 * ra[0], tiles, maps=(ra, rb), c_gap=2)
    p = plan(s, 7600)
    g = BR.group_plan([(s.M, s.N, s.K, s.batch)], cus)
    c = p.call
    sens, av, bv = [], BR.bf16_decode(p.a), BR.bf16_decode(p.b)
    for t in range(0, tiles, max(1, tiles // 4)):   # M = N = 8: tile t is batch entry t
        starts = (0,) if g.whole else tuple(sorted(64 * kt0 for runs in g.runs for j, tile, kt0, nk in runs if tile == t))
        one = replace(c, batch=1, a_base=c.a_base + t * c.stride_a, b_base=c.b_base + t * c.stride_b)
        sens.append(BR.carry_matters(one, av, bv, starts))
    assert any(sens) == (64 % ra[0] != 0), f"group {ra[0]}: carry matters {sens}"
    if form == "stream-K":
        assert g.U >= 2 and any(kt0 > 0 and nk > 1 for runs in g.runs for _, _, kt0, nk in runs)
    run_group(L, cus, [s], 7600, whole=form == "whole")


# ------------------------------------------------------------------------------------------------------------ rounding
@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (0, 0), (1, 0)])
def test_rounding_is_nearest_even_and_bf16_bits_are_taken_as_given(L, a_kc, b_kc):
    """A: odd integers 257 .. 511 -- every one a tie (257 -> 256, 259 -> 260) -- B: -1 / 0 / 1.  Truncation and round-half-up both
    give other sums.  The bf16-source routes, given bf16_bits of the same values, give the same C."""
    res = {}
    for route, M, K in (("staged_f32", 128, 252), ("staged_b16", 128, 252), ("staged_f32", 128, 256), ("ring", 128, 256)):
        s = Spec(route, a_kc, b_kc, M, 16, K, src16=route != "staged_f32", kind="tie", bias=True)
        got, p, want, valid, _ = run_case(L, s, 8000)
        res[(route, K)] = got[GR.c_index(p.call, 0)]
        if route == "staged_f32":    # the case can tell the roundings apart
            A = GR.gather_a(BR.ref_call(p.call), p.a.astype(np.float64), 0)
            assert (A % 2 == 1).all() and A.min() >= 257 and A.max() <= 511
            B = GR.gather_b(BR.ref_call(p.call), p.b.astype(np.float64), 0)
            even = want[GR.c_index(p.call, 0)] - p.bias[3:3 + 16].astype(np.float64)[None, :]
            assert not np.array_equal((A - 1) @ B, even) and not np.array_equal((A + 1) @ B, even)   # truncation, half-up
    assert torch.equal(torch.from_numpy(res[("staged_f32", 252)]), torch.from_numpy(res[("staged_b16", 252)]))
    assert torch.equal(torch.from_numpy(res[("staged_f32", 256)]), torch.from_numpy(res[("ring", 256)]))


@pytest.mark.parametrize("a_kc,b_kc", [(1, 0), (0, 0)])
def test_rounding_ring_kcat_takes_bf16_bits_as_given(L, a_kc, b_kc):
    """The K-concatenated ring, given bf16_bits of the tie values of two pairs, stores the sum of what the f32-source kernel rounds
    and multiplies pair by pair (integers: the sum of the two C is exact)."""
    f32, pf, *_ = run_case(L, Spec("staged_f32", a_kc, b_kc, 128, 16, 128, src16=0, kind="tie", batch=2), 8100)
    cat, pc, *_ = run_case(L, Spec("ring_kcat", a_kc, b_kc, 128, 16, 128, kind="tie", batch=2, flags=16, a_gap=8), 8100)
    pair_sum = f32[GR.c_index(pf.call, 0)] + f32[GR.c_index(pf.call, 1)]
    assert torch.equal(torch.from_numpy(cat[GR.c_index(BR.ref_call(pc.call), 0)]), torch.from_numpy(pair_sum))


@pytest.mark.parametrize("whole", [False, True])
def test_rounding_group_takes_bf16_bits_as_given(L, cus, whole):
    """Both forms of the group kernel, given bf16_bits of the tie values, add to C what the f32-source kernel adds.  The tie problem
    comes first (same seed, same values, same C0); tiny problems behind it put the group on the wanted side of the threshold."""
    need_cus(cus, 16)
    f32, pf, *_ = run_case(L, Spec("staged_f32", 0, 0, 128, 16, 256, src16=0, kind="tie", flags=1), 8200)
    specs = [gp(128, 16, 256, 1, kind="tie")] + ([gp(8, 8, 64, ceil_div(cus, 2), c_gap=2)] if whole else [])
    out, _ = run_group(L, cus, specs, 8200, whole=whole)
    got, pg, _, _ = out[0]
    assert torch.equal(torch.from_numpy(pf.c[GR.c_index(pf.call, 0)]), torch.from_numpy(pg.c[GR.c_index(pg.call, 0)])), "C0 differs"
    assert torch.equal(torch.from_numpy(got[GR.c_index(pg.call, 0)]), torch.from_numpy(f32[GR.c_index(pf.call, 0)]))


@pytest.mark.parametrize("ld_y_extra", [0, 8])
@pytest.mark.parametrize("cols", [1, 4, 7, 8, 9, 12, 100])
def test_cvt_bf16_rows(L, cols, ld_y_extra):
    """drop_p = 0: the tie table as a (rows, cols) block.  Bits equal bf16_bits (NaN stays NaN), the padding up to ld_y is zero,
    nothing behind the last row is touched.  cols % 4 != 0 is outside the ABI: refused, y untouched."""
    t = BR.tie_table()
    rows = ceil_div(t.size, cols)
    x = np.resize(t, rows * cols).reshape(rows, cols)
    ld_x = (cols + 3) // 4 * 4 + 4
    xb = np.full((rows, ld_x), NAN, dtype=np.float32)
    xb[:, :cols] = x
    ld_y = ceil8(cols) + ld_y_extra
    y = torch.full((rows + 2, ld_y), 0x1234, dtype=torch.int16, device="cuda")
    x_d = torch.from_numpy(xb).cuda()
    st = L.load().ss_cvt_bf16_rows(x_d.data_ptr(), ld_x, y.data_ptr(), ld_y, rows, cols, 0.0, 0, 0, L.stream())
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    if cols % 4:
        assert st == SS_ERR_ARG and (got == 0x1234).all()
        return
    assert st == 0
    want = BR.bf16_bits(x)
    nan = np.isnan(x)
    assert nan.any() and np.array_equal(got[:rows, :cols][~nan], want[~nan])
    assert np.isnan(BR.bf16_decode(got[:rows, :cols][nan])).all()
    assert (got[:rows, cols:] == 0).all() and (got[rows:] == 0x1234).all()


# --------------------------------------------------------------------------------------------------------- float cases
def float_check(name, got, want, mags, c_indices, K_total, extra):
    worst = 0.0
    for (A, B, c0, bias), idx in zip(mags, c_indices):
        bound = GR.f32_bound(np.abs(A), np.abs(B), K_total, extra, c0=c0, bias=bias)
        err = np.abs(got.astype(np.float64)[idx] - want[idx])
        assert np.isfinite(err).all(), name
        worst = max(worst, float((err / bound).max()))
    print(f"{name}: largest error / bound {worst:.4f} (K_total {K_total}, {extra} further additions)")
    assert worst <= 1.0, f"{name}: error {worst:.3f} x the f32 bound"


FLOATS = {
    "staged_f32": Spec("staged_f32", 0, 1, 132, 65, 200, src16=0, flags=1, splits=3, bias=True, a_ld=4, kind="real"),
    "staged_b16": Spec("staged_b16", 1, 0, 65, 136, 200, flags=1, splits=3, bias=True, batch=2, a_ld=8, kind="real"),
    "ring": Spec("ring", 1, 0, 260, 136, 320, flags=1, splits=2, bias=True, batch=2, kind="real"),
    "ring_kcat": Spec("ring_kcat", 1, 0, 130, 136, 128, flags=16, batch=3, bias=True, a_gap=8, kind="real"),
}


@pytest.mark.parametrize("route", list(FLOATS))
def test_float_batched(L, route):
    """randn operands: |got - float64 product of the bf16-rounded operands| <= f32_bound elementwise.  Further additions: bias,
    accumulate, one per K slice (atomics) or per joined pair."""
    s = FLOATS[route]
    got, p, want, valid, r = run_case(L, s, 9000)
    c = p.call
    kcat = c.batch if c.flags & 16 else 1
    idx = [GR.c_index(BR.ref_call(c), b) for b in range(1 if c.flags & 16 else c.batch)]
    float_check(route, got, want, magnitudes(p), idx, c.K * kcat, int(s.bias) + (c.flags & 1) + r.splits + kcat - 1)
    assert np.array_equal(got[~valid], p.c[~valid])


@pytest.mark.parametrize("form", ["stream-K", "whole"])
def test_float_group(L, cus, form):
    """Slabs + reduce: one addition per slab of a tile and the one onto C; the whole form adds onto C once."""
    if form == "whole":
        specs = [gp(8, 8, 320, max(1, ceil_div(cus, 2) - 1), kind="real", c_gap=2), gp(130, 136, 192, 1, maps=MAPS[0], kind="real")]
    else:
        specs = [gp(130, 136, 320, 2, kind="real"), gp(8, 129, 192, 1, maps=MAPS[0], kind="real")]
    need_cus(cus, 16)
    out, g = run_group(L, cus, specs, 9100, whole=form == "whole", exact=False)
    for j, (got, p, want, valid) in enumerate(out):
        c = p.call
        float_check(f"group {form} problem {j}", got, want, magnitudes(p), [GR.c_index(c, b) for b in range(c.batch)], c.K,
                    1 if g.whole else max(g.counts) + 1)
        assert np.array_equal(got[~valid], p.c[~valid])


# ------------------------------------------------------------------------------------------------------------ refusals
def _refusal_buffers():
    a = torch.zeros(64 * 64 + 64, dtype=torch.int16, device="cuda")
    b = torch.zeros(64 * 64 + 64, dtype=torch.int16, device="cuda")
    c = torch.full((4096,), SENT, device="cuda")
    bias = torch.ones(64, device="cuda")
    return a, b, c, bias


def _batched(L, bufs, **kw):
    """A small valid call (bf16 operands, k-major A, [n][k] B, 8 x 8 x 64), changed by ``kw``."""
    a, b, c, bias = bufs
    d = dict(a_kc=0, b_kc=1, M=8, N=8, K=64, A=a.data_ptr(), lda=8, B=b.data_ptr(), ldb=64, C=c.data_ptr() + 4 * 1024, ldc=8, bias=None, flags=8,
             splits=1, batch=1, sa=0, sb=0, ra=IDENT, rb=IDENT)
    d.update(kw)
    return L.load().ss_gemm_bf16_batched(d["a_kc"], d["b_kc"], d["M"], d["N"], d["K"], d["A"], d["lda"], *d["ra"], d["B"], d["ldb"], *d["rb"], d["C"],
                                         d["ldc"], d["bias"], d["flags"], d["splits"], d["batch"], d["sa"], d["sb"], 0, 0, L.stream())


BATCHED_REFUSALS = {
    "unknown flag bit 1": (dict(flags=8 | 2), SS_ERR_UNSUPPORTED),
    "unknown flag bit 5": (dict(flags=8 | 32), SS_ERR_UNSUPPORTED),
    "unknown flag bit 12": (dict(flags=8 | 4096), SS_ERR_UNSUPPORTED),
    "kcat without bf16 operands": (dict(flags=16, batch=2), SS_ERR_UNSUPPORTED),
    "kcat with K % 64": (dict(flags=8 | 16, K=56, batch=2), SS_ERR_UNSUPPORTED),
    "kcat with splits": (dict(flags=8 | 16 | 1, K=128, ldb=128, splits=2, batch=2), SS_ERR_UNSUPPORTED),
    "kcat with atomics": (dict(flags=8 | 16 | 4 | 1, batch=2), SS_ERR_UNSUPPORTED),
    "splits without accumulate": (dict(K=128, ldb=128, splits=2), SS_ERR_ARG),
    "atomics without accumulate": (dict(flags=8 | 4), SS_ERR_ARG),
    "bf16 lda % 8": (dict(lda=12), SS_ERR_UNSUPPORTED),
    "bf16 ldb % 8": (dict(ldb=68), SS_ERR_UNSUPPORTED),
    "bf16 stride_a % 8": (dict(batch=2, sa=516), SS_ERR_UNSUPPORTED),
    "bf16 stride_b % 8": (dict(batch=2, sb=4), SS_ERR_UNSUPPORTED),
    "f32 lda % 4": (dict(flags=0, K=16, lda=10, ldb=16), SS_ERR_UNSUPPORTED),
    "f32 stride_b % 4": (dict(flags=0, K=16, ldb=16, batch=2, sb=2), SS_ERR_UNSUPPORTED),
    "f32 M % 4 of a k-major A": (dict(flags=0, K=16, M=6, ldb=16), SS_ERR_UNSUPPORTED),
    "f32 K % 4 of a k-contiguous B": (dict(flags=0, K=14, ldb=16), SS_ERR_UNSUPPORTED),
    "bf16 M > lda": (dict(M=9, lda=8), SS_ERR_ARG),
    "bf16 K > ldb": (dict(K=64, ldb=56), SS_ERR_ARG),
    "A 2 bytes off": (dict(a_byte=2), SS_ERR_UNSUPPORTED),
    "A 8 bytes off": (dict(a_byte=8), SS_ERR_UNSUPPORTED),
    "B 2 bytes off": (dict(b_byte=2), SS_ERR_UNSUPPORTED),
    "B 8 bytes off": (dict(b_byte=8), SS_ERR_UNSUPPORTED),
    "A null": (dict(A=None), SS_ERR_ARG), "B null": (dict(B=None), SS_ERR_ARG), "C null": (dict(C=None), SS_ERR_ARG),
    "M = 0": (dict(M=0), SS_ERR_ARG), "N = -1": (dict(N=-1), SS_ERR_ARG), "K = 0": (dict(K=0), SS_ERR_ARG), "batch = 0": (dict(batch=0), SS_ERR_ARG),
    "splits = 0": (dict(splits=0), SS_ERR_ARG), "a_group = 0": (dict(ra=(0, 0, 0)), SS_ERR_ARG), "b_group = -1": (dict(rb=(-1, 0, 0)), SS_ERR_ARG),
}


@pytest.mark.parametrize("name", list(BATCHED_REFUSALS))
def test_refusals_batched(L, name):
    """Rejected on the host before any launch: the return code, and C keeps its bits.  The same call without the fault is taken."""
    kw, code = BATCHED_REFUSALS[name]
    kw = dict(kw)
    bufs = _refusal_buffers()
    if "a_byte" in kw:
        kw["A"] = bufs[0].data_ptr() + kw.pop("a_byte")
    if "b_byte" in kw:
        kw["B"] = bufs[1].data_ptr() + kw.pop("b_byte")
    assert _batched(L, bufs, **kw) == code
    torch.cuda.synchronize()
    assert bool((bufs[2] == SENT).all())
    assert _batched(L, bufs) == 0
    torch.cuda.synchronize()
    c = bufs[2]
    assert bool((c[1024:1088] == 0).all()) and bool((c[:1024] == SENT).all()) and bool((c[1088:] == SENT).all())


GROUP_REFUSALS = ["n = 0", "n = 9", "k-contiguous A", "k-contiguous B", "K % 64", "lda % 8", "M > lda", "ldc < N", "workspace null",
                  "workspace misaligned", "workspace one float short"]


@pytest.mark.parametrize("name", GROUP_REFUSALS)
def test_refusals_group(L, cus, name):
    a, b, c, _ = _refusal_buffers()
    ws = torch.full((WS_GUARD + 4 * BR.SLAB_FLOATS,), SENT, device="cuda")

    def prob(**kw):
        d = dict(a_kc=0, b_kc=0, M=8, N=8, K=128, lda=8, ldb=8, ldc=8, batch=1)
        d.update(kw)
        return L.GemmProblem(d["a_kc"], d["b_kc"], d["M"], d["N"], d["K"], a.data_ptr(), d["lda"], INT_MAX, 0, 0, b.data_ptr(), d["ldb"], INT_MAX, 0, 0,
                             c.data_ptr() + 4 * 1024, d["ldc"], 1, d["batch"], 0, 0, 0)

    good = prob()
    plan_ = BR.group_plan([(8, 8, 128, 1)], cus)
    need = L.gemm_group_ws_floats([good], bf16=True)
    assert need == plan_.ws_floats and (not plan_.whole or cus <= 2)
    probs, n, wsp, have, code = [good], 1, ws.data_ptr(), need, SS_ERR_ARG
    if name == "n = 0":
        n = 0
    elif name == "n = 9":
        probs, n, have = [good] * 9, 9, ws.numel()
    elif name == "k-contiguous A":
        probs, code = [good, prob(a_kc=1)], SS_ERR_UNSUPPORTED
    elif name == "k-contiguous B":
        probs, code = [prob(b_kc=1)], SS_ERR_UNSUPPORTED
    elif name == "K % 64":
        probs, code = [prob(K=96)], SS_ERR_UNSUPPORTED
    elif name == "lda % 8":
        probs = [prob(lda=12)]
    elif name == "M > lda":
        probs = [prob(M=9)]
    elif name == "ldc < N":
        probs = [good, prob(ldc=7)]
    elif name == "workspace null":
        wsp = None
    elif name == "workspace misaligned":
        wsp += 4
    elif name == "workspace one float short":
        have = need - 1
    if name not in ("n = 0", "n = 9"):
        n = len(probs)
    if n > 1 and name not in ("n = 9",):
        have = ws.numel()
    arr = (L.GemmProblem * len(probs))(*probs)
    assert L.load().ss_gemm_bf16_splitk_group(arr, n, wsp, have, L.stream()) == code
    torch.cuda.synchronize()
    assert bool((c == SENT).all()) and bool((ws == SENT).all())
    if name.startswith("n =") or "k-contiguous" in name or name in ("K % 64", "lda % 8", "M > lda", "ldc < N"):   # the size query refuses the same
        import ctypes
        out = ctypes.c_long(0)
        assert L.load().ss_gemm_bf16_splitk_group_ws_floats(arr, n, ctypes.byref(out)) == code
    # the same call without the fault is taken
    arr = (L.GemmProblem * 1)(good)
    assert L.load().ss_gemm_bf16_splitk_group(arr, 1, ws.data_ptr(), need, L.stream()) == 0
    torch.cuda.synchronize()
    assert bool((c[1024:1088] == SENT).all()) and bool((c[:1024] == SENT).all())   # C += 0 A^T B of zeros: -77 + 0
