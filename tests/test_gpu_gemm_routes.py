"""GPU: every route of the f32 GEMM dispatcher (csrc/gemm.hip) at its tile and slice edges, bit for bit.

Operands are small integers (tests/gemm_ref.py asserts for every case that no partial sum can reach 2**24), so every order of
float additions -- MFMA chains, split-K atomics, slabs + reduce, the summed batch -- gives the same bits and each case is
compared with ``torch.equal`` against the float64 reference of ``gemm_ref.reference``.  Each operand lies in a larger buffer of
NaN (leading-dimension padding, the rows a row map skips, eight guard rows before and after): an element that leaks into a
result shows as NaN.  C and a_colsum lie in buffers of a sentinel integer that must be the same afterwards.

Every case names the kernel it means to reach and asserts that ``gemm_ref.route`` agrees for the device it runs on; the cases
whose route depends on the CU count are built from it.  One float case per route checks precision against the derived
``gemm_ref.f32_bound`` (integers cannot see an MFMA of lower precision) and prints its largest error / bound ratio.
Refusals are calls the dispatcher rejects on the host before any launch.

The DMA-fed kernels cannot take a_colsum, so "all five batch strides" is four on ``dma`` plus the colsum stride on ``staged``.
"""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import pytest
import torch

import gemm_ref as GR
from gemm_ref import IDENT, INT_MAX, Call, ceil_div
from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8
SENT = -77.0
NAN = float("nan")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.fixture(scope="module")
def cus(L):
    return torch.cuda.get_device_properties(0).multi_processor_count


def pad4(extent, extra=0):
    """Padding that makes extent + padding a multiple of 4, plus ``extra``."""
    return (-extent) % 4 + extra


# ------------------------------------------------------------------------------------------------------------ placing
@dataclass
class Spec:
    route: str
    a_kc: int
    b_kc: int
    M: int
    N: int
    K: int
    a_pad: int = 0      # lda = extent + a_pad
    b_pad: int = 0
    c_pad: int = 0
    a_off: int = 0      # words the operand's base is moved off its 16-byte aligned position
    b_off: int = 0
    c_off: int = 0
    ra: Tuple[int, int, int] = IDENT
    rb: Tuple[int, int, int] = IDENT
    bias: bool = False
    bias_stride: Optional[int] = None   # default: N
    flags: int = 0
    splits: int = 1
    batch: int = 1
    share_a: bool = False               # stride_a = 0
    share_b: bool = False
    c_gap: int = 0                      # stride_c = M * ldc + c_gap
    colsum: bool = False
    colsum_gap: int = 3                 # stride_colsum = M + colsum_gap
    real: bool = False                  # normal values instead of integers (the float cases)


def values(nb, shape, seed, real, hi=4):
    """nb arrays of ``shape``; entry b depends on (seed, b) alone, so that runs with different batch counts share their entries."""
    return [np.random.default_rng(seed + 7919 * b).standard_normal(shape).astype(np.float32) if real
            else GR.int_operands(shape, seed + 7919 * b, -hi, hi) for b in range(nb)]


def place_operand(kc, rows, K, pad, rmap, nb, off, seed, real):
    """-> (flat float32 buffer of NaN holding nb operands, element offset of the first, ld, stride between them)."""
    R, W = (rows, K) if kc else (K, rows)   # storage rows before the map, their width
    ld = W + pad
    sr = GR.map_rows(R, rmap)
    per = (int(sr.max()) + 1) * ld
    base = GUARD_ROWS * ld + off
    buf = np.full(base + nb * per + GUARD_ROWS * ld, NAN, dtype=np.float32)
    vals = values(nb, (R, W), seed, real)
    idx = base + sr[:, None] * ld + np.arange(W)[None, :]
    for b in range(nb):
        buf[idx + b * per] = vals[b]
    return buf, base, ld, per


def place_out(rows, cols, pad, nb, off, gap, seed, real, fill=SENT):
    """C (or, with cols = 1 ... a vector): nb blocks of [rows][cols + pad] inside a buffer of the sentinel."""
    ld = cols + pad
    per = rows * ld
    stride = per + gap
    base = GUARD_ROWS * ld + off
    buf = np.full(base + (nb - 1) * stride + per + GUARD_ROWS * ld, fill, dtype=np.float32)
    vals = values(nb, (rows, cols), seed, real)
    idx = base + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    for b in range(nb):
        buf[idx + b * stride] = vals[b]
    return buf, base, ld, stride


@dataclass
class Plan:
    call: Call
    a: np.ndarray
    b: np.ndarray
    c: np.ndarray
    bias: Optional[np.ndarray]
    cs: Optional[np.ndarray]


def plan(s: Spec, seed: int) -> Plan:
    """Host side of a case: the buffers and the call that points into them."""
    summed = bool(s.flags & 16)
    a, a_base, lda, a_per = place_operand(s.a_kc, s.M, s.K, s.a_pad, s.ra, 1 if s.share_a else s.batch, s.a_off, seed, s.real)
    b, b_base, ldb, b_per = place_operand(s.b_kc, s.N, s.K, s.b_pad, s.rb, 1 if s.share_b else s.batch, s.b_off, seed + 1, s.real)
    c, c_base, ldc, c_stride = place_out(s.M, s.N, s.c_pad, 1 if summed else s.batch, s.c_off, s.c_gap, seed + 2, s.real)
    bias = cs = None
    bias_base = cs_base = None
    bstride = s.bias_stride if s.bias_stride is not None else (s.N if s.batch > 1 and not summed else 0)
    if s.bias:
        nb = 1 if bstride == 0 else s.batch
        bias = np.full(3 + (nb - 1) * bstride + s.N + 5, NAN, dtype=np.float32)
        bias_base = 3
        v = values(nb, (s.N,), seed + 3, s.real, 9)
        for k in range(nb):
            bias[3 + k * bstride: 3 + k * bstride + s.N] = v[k]
    cstride = 0
    if s.colsum:
        cs, cs_base, _, cstride = place_out(1, s.M, 0, s.batch, 1, s.colsum_gap, seed + 4, s.real)
    call = Call(s.a_kc, s.b_kc, s.M, s.N, s.K, lda, ldb, ldc, ra=s.ra, rb=s.rb, flags=s.flags, splits=s.splits, batch=s.batch,
                stride_a=0 if s.share_a else a_per, stride_b=0 if s.share_b else b_per, stride_c=c_stride,
                stride_bias=bstride if s.bias else 0, stride_colsum=cstride, a_base=a_base, b_base=b_base, c_base=c_base,
                bias_base=bias_base, colsum_base=cs_base)
    return Plan(call, a, b, c, bias, cs)


def magnitudes(p: Plan):
    """Per C: (|A| concatenated along K over everything that is summed into it, |B| likewise, C0, bias) for the exactness
    assertion and the float bound."""
    c = p.call
    out = []
    groups = [list(range(c.batch))] if c.flags & 16 else [[b] for b in range(c.batch)]
    for g in groups:
        A = np.concatenate([GR.gather_a(c, p.a, b) for b in g], 1)
        B = np.concatenate([GR.gather_b(c, p.b, b) for b in g], 0)
        c0 = p.c.astype(np.float64)[GR.c_index(c, g[0])] if c.flags & (1 | 8) else None
        bias = None if p.bias is None else p.bias.astype(np.float64)[c.bias_base + g[0] * c.stride_bias + np.arange(c.N)]
        out.append((A, B, c0, bias))
    return out


def check_exact(p: Plan):
    for A, B, c0, bias in magnitudes(p):
        GR.assert_exact_range([(A, B)], c0, bias)


def to_dev(x):
    return None if x is None else torch.from_numpy(x).cuda()


def dptr(t, base):
    return None if t is None else t.data_ptr() + 4 * base


def batched_args(L, c: Call, a_d, b_d, c_d, bias_d, cs_d, c_ptr=None):
    return (c.a_kc, c.b_kc, c.M, c.N, c.K, dptr(a_d, c.a_base), c.lda, *c.ra, dptr(b_d, c.b_base), c.ldb, *c.rb,
            dptr(c_d, c.c_base) if c_ptr is None else c_ptr, c.ldc, dptr(bias_d, c.bias_base or 0), dptr(cs_d, c.colsum_base or 0),
            c.flags, c.splits, c.batch, c.stride_a, c.stride_b, c.stride_c, c.stride_bias, c.stride_colsum, L.stream())


def same_bits(name, got, want, mask):
    """torch.equal on the elements a call may write, and on everything around them."""
    got_t, want_t, m = torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(mask)
    assert torch.equal(got_t[~m], want_t[~m]), f"{name}: a guard element changed"
    if not torch.equal(got_t[m], want_t[m]):
        bad = np.flatnonzero(mask & ~((got == want) | (np.isnan(got) & np.isnan(want))))
        pytest.fail(f"{name}: {bad.size} of {int(mask.sum())} elements differ, first at flat {bad[0]}: got {got[bad[0]]}, "
                    f"want {want[bad[0]]}", pytrace=False)


def run_case(L, cus, s: Spec, seed: int):
    """One ss_gemm_f32_batched call against the reference.  -> (device C as numpy, the plan)."""
    p = plan(s, seed)
    c = p.call
    if not s.real:
        check_exact(p)
    a_d, b_d, c_d, bias_d, cs_d = to_dev(p.a), to_dev(p.b), to_dev(p.c), to_dev(p.bias), to_dev(p.cs)
    r = GR.route(c, dptr(a_d, c.a_base) % 16, dptr(b_d, c.b_base) % 16, cus)
    assert r.name == s.route, f"meant for {s.route}, the dispatcher takes {r.name} on {cus} CUs"
    L.call("ss_gemm_f32_batched", *batched_args(L, c, a_d, b_d, c_d, bias_d, cs_d))
    torch.cuda.synchronize()
    got = c_d.cpu().numpy()
    want, cs_want, valid = GR.reference(c, p.a, p.b, p.c, p.bias, p.cs)
    assert np.isfinite(want).all(), "the reference read padding: the case is built wrongly"
    if s.real:
        return got, p, want, valid, r
    same_bits("C", got, want.astype(np.float32), valid)
    if s.colsum:
        cmask = np.zeros(p.cs.shape, dtype=bool)
        for b in range(c.batch):
            cmask[c.colsum_base + b * c.stride_colsum + np.arange(c.M)] = True
        same_bits("a_colsum", cs_d.cpu().numpy(), cs_want.astype(np.float32), cmask)
    # the operands are inputs
    assert torch.equal(a_d.cpu().view(torch.int32), torch.from_numpy(p.a).view(torch.int32))
    assert torch.equal(b_d.cpu().view(torch.int32), torch.from_numpy(p.b).view(torch.int32))
    return got, p, want, valid, r


def ids(specs):
    return [f"{i:02d}-{'kc' if s.a_kc else 'km'}x{'kc' if s.b_kc else 'km'}-{s.M}x{s.N}x{s.K}-f{s.flags}s{s.splits}b{s.batch}"
            for i, s in enumerate(specs)]


# ------------------------------------------------------------------------------------------------------------- staged
def staged_specs():
    Ms, Ns, Ks = [1, 5, 127, 128, 129], [1, 3, 63, 64, 65], [1, 15, 16, 17, 48]
    out = []
    for i in range(25):  # a Latin square: every pair of (M, N), (M, K), (N, K) occurs
        m, n = i % 5, i // 5
        a_kc, b_kc = LAYOUTS[i % 4]
        out.append(Spec("staged", a_kc, b_kc, Ms[m], Ns[n], Ks[(m + n) % 5], a_pad=[0, 1, 3][i % 3], b_pad=[0, 1, 3][(i // 3) % 3],
                        c_pad=[0, 1, 4][(i // 2) % 3], a_off=i % 2, b_off=(i // 2) % 2, c_off=(i // 4) % 2, bias=i % 2 == 0,
                        flags=(i + i // 5) % 4))
    # split-K atomics without column sums, and the always-atomic bit as the head gradients use it
    out += [Spec("staged", 0, 0, 129, 65, 48, flags=1, splits=3, bias=True, c_pad=1),
            Spec("staged", 1, 1, 5, 3, 17, flags=1, splits=3, a_pad=1, c_off=1),
            Spec("staged", 1, 0, 127, 64, 48, flags=1, splits=3, b_pad=4),
            Spec("staged", 0, 0, 128, 65, 17, flags=5, a_pad=1, bias=True),
            Spec("staged", 0, 1, 129, 63, 48, flags=5, c_pad=4),
            Spec("staged", 1, 1, 5, 64, 16, flags=5, bias=True)]
    # column sums of a k-major A riding along
    out += [Spec("staged", 0, 0, 129, 65, 48, colsum=True, bias=True),
            Spec("staged", 0, 1, 127, 3, 17, colsum=True, flags=1, a_pad=3),
            Spec("staged", 0, 0, 129, 64, 48, colsum=True, flags=1, splits=3),
            Spec("staged", 0, 0, 132, 68, 200, colsum=True, flags=1, splits=3, a_pad=4),   # aligned: only a_colsum keeps it here
            Spec("staged", 0, 0, 5, 65, 17, colsum=True, batch=3, bias=True, c_gap=5),
            Spec("staged", 0, 1, 129, 3, 33, colsum=True, batch=3, flags=1, splits=2, share_b=True, colsum_gap=0)]
    return out


STAGED = staged_specs()


@pytest.mark.parametrize("s", STAGED, ids=ids(STAGED))
def test_staged(L, cus, s):
    run_case(L, cus, s, 1000 + STAGED.index(s))


# ---------------------------------------------------------------------------------------------------------------- dma
def dma_spec(a_kc, b_kc, M, N, K, a_extra=0, b_extra=0, **kw):
    """Leading dimensions that are multiples of 4: the extent rounded up, plus ``extra``."""
    return Spec("dma", a_kc, b_kc, M, N, K, a_pad=pad4(K if a_kc else M, a_extra), b_pad=pad4(K if b_kc else N, b_extra), **kw)


def dma_specs():
    Ms, Ns, Ks = [4, 124, 128, 132, 260], [4, 60, 64, 68, 132], [64, 65, 67, 79, 80, 81, 116]
    out = []
    for i in range(35):  # every (M, K) pair, every (M, N) pair
        a_kc, b_kc = LAYOUTS[i % 4]
        out.append(dma_spec(a_kc, b_kc, Ms[i % 5], Ns[(i // 5 + i % 5) % 5], Ks[i % 7], a_extra=4 * (i % 2), b_extra=4 * ((i // 2) % 2),
                            a_off=4 * ((i // 2) % 2), b_off=4 * ((i // 3) % 2), c_pad=[0, 1, 4][i % 3], c_off=(i // 3) % 2,
                            bias=i % 2 == 1, flags=(i // 2) % 4))
    # K slices: a last slice shorter than the ring (200 / 3: 80, 80, 40), 129 / 2: 80, 49, 161 / 2: 96, 65 (a ragged tile of one
    # element), 193 / 4: 64, 64, 64, 1 (a last slice of one element)
    for j, (K, splits) in enumerate([(200, 3), (129, 2), (161, 2), (193, 4)]):
        for a_kc, b_kc in (LAYOUTS[j % 4], LAYOUTS[(j + 3) % 4]):
            out.append(dma_spec(a_kc, b_kc, 132, 68, K, flags=1, splits=splits, bias=j % 2 == 0, c_pad=j % 2, a_extra=4))
    # a full and a partial column tile in one launch with an aligned C: the staged 16-byte store and the scalar form together
    out += [dma_spec(1, 1, 132, 68, 67, flags=0, bias=True), dma_spec(0, 0, 260, 132, 80, flags=3, bias=True, c_pad=4),
            dma_spec(1, 0, 128, 132, 65, flags=1), dma_spec(0, 1, 124, 68, 116, flags=2, c_off=1)]
    # batches
    out += [dma_spec(1, 1, 132, 68, 67, batch=3, bias=True, c_gap=4, a_extra=4), dma_spec(0, 0, 132, 68, 81, batch=3, bias=True, c_gap=1, flags=1),
            dma_spec(1, 1, 124, 60, 80, batch=2, share_a=True, bias=True), dma_spec(0, 1, 128, 64, 65, batch=2, share_a=True, bias=True, flags=3),
            dma_spec(1, 0, 132, 68, 200, batch=2, flags=1, splits=3, bias=True, share_b=True)]
    # always atomic without a K split
    out += [dma_spec(1, 1, 132, 68, 67, flags=5, bias=True), dma_spec(0, 0, 128, 64, 64, flags=5)]
    return out


DMA = dma_specs()


@pytest.mark.parametrize("s", DMA, ids=ids(DMA))
def test_dma(L, cus, s):
    run_case(L, cus, s, 2000 + DMA.index(s))


# ----------------------------------------------------------------------------------------------------------- row maps
MAPS = [(INT_MAX, 0, 3), (5, 6, 1), (8, 9, 0), (1, 2, 0)]


def rowmap_specs():
    out = []
    combo = 0
    for route in ("staged", "dma"):
        for side in ("a", "b", "ab"):
            for kc in (1, 0):
                for G, S, off in (MAPS[combo % 4], MAPS[(combo + 2) % 4]):
                    # 37 / 83 rows or k: no multiple of a group, so that 16-wide tiles straddle groups of 5 and 8
                    M, N, K = (37, 22, 37) if route == "staged" else (132, 68, 83)
                    ra = (G, S, off) if "a" in side else IDENT
                    rb = (G, S, 0 if side == "ab" else off) if "b" in side else IDENT  # "ab": A rows pair with the B rows before
                    a_kc = kc if "a" in side else 1 - kc
                    b_kc = kc if "b" in side else 1 - kc
                    mk = dma_spec if route == "dma" else (lambda *a, **k: Spec("staged", *a, a_pad=1, **k))
                    out.append(mk(a_kc, b_kc, M, N, K, ra=ra, rb=rb, bias=combo % 2 == 0, flags=combo % 4, c_pad=combo % 2))
                combo += 1
    # a K split whose later slices start inside a group, on both kernels; column sums over the mapped rows only
    out += [dma_spec(0, 0, 132, 68, 200, ra=(5, 6, 1), rb=(5, 6, 0), flags=1, splits=3),
            dma_spec(1, 1, 132, 68, 200, ra=(5, 6, 1), rb=(8, 9, 0), flags=1, splits=3, bias=True),
            dma_spec(0, 1, 132, 68, 193, ra=(8, 9, 1), flags=1, splits=4),
            Spec("staged", 0, 0, 37, 22, 48, ra=(5, 6, 1), rb=(5, 6, 0), flags=1, splits=3, colsum=True),
            Spec("staged", 0, 0, 129, 22, 37, ra=(8, 9, 0), colsum=True, b_pad=1)]
    return out


ROWMAP = rowmap_specs()


@pytest.mark.parametrize("s", ROWMAP, ids=[f"{x}-{s.route}-a{s.ra[0] % 1000}.{s.ra[2]}-b{s.rb[0] % 1000}.{s.rb[2]}" for x, s in zip(ids(ROWMAP), ROWMAP)])
def test_row_maps(L, cus, s):
    run_case(L, cus, s, 3000 + ROWMAP.index(s))


# ------------------------------------------------------------------------------------------------------------ wide_kc
def wide_batch(M, N, cus, low):
    """A batch count that puts the 192 x 192 tile count at the low (80 %) or the high (100 %) end of the wide kernel's window."""
    tpb = ceil_div(M, GR.WT) * ceil_div(N, GR.WT)
    return ceil_div(8 * cus, 10 * tpb) if low else cus // tpb


WIDE = [(i, [1, 188, 192, 196, 385][i % 5], [96, 100, 188, 192, 196][(i // 5 + i % 5) % 5], [52, 64, 68, 116][i % 4]) for i in range(20)]


@pytest.mark.parametrize("i,M,N,K", WIDE, ids=[f"{i:02d}-{M}x{N}x{K}" for i, M, N, K in WIDE])
def test_wide_kc(L, cus, i, M, N, K):
    s = Spec("wide_kc", 1, 1, M, N, K, batch=wide_batch(M, N, cus, low=i % 2 == 1), bias=i % 3 != 0, bias_stride=[None, 0, None][i % 3],
             share_a=(i // 2) % 2 == 0, c_pad=[0, 1, 4][(i // 2) % 3], a_pad=4 * (i % 2), c_gap=4 * (i % 3), a_off=4 * ((i // 4) % 2))
    run_case(L, cus, s, 4000 + i)


def test_wide_kc_window_edges_give_the_same_bits(L, cus):
    """One tile above the CU count and the largest count under 80 % are the narrow DMA kernel's; their batch entries hold the same
    bits as the wide kernel's."""
    M, N, K = 100, 100, 68
    got = {}
    for route, batch in (("wide_kc", cus), ("dma", cus + 1), ("dma", (8 * cus - 1) // 10)):
        s = Spec(route, 1, 1, M, N, K, batch=batch, bias=True, share_a=True, c_pad=4)
        g, p, _, _, _ = run_case(L, cus, s, 4100)  # one seed: entry b of every run has the same operands
        c = p.call
        got[batch] = np.stack([g[GR.c_index(c, b)] for b in range(batch)])
    wide = got[cus]
    for batch, g in got.items():
        n = min(batch, cus)
        assert torch.equal(torch.from_numpy(g[:n]), torch.from_numpy(wide[:n]))


# ------------------------------------------------------------------------------------------------------- summed batch
def summed_specs():
    out = []
    i = 0
    for route in ("summed_dma", "summed_loop"):
        for kcat in (2, 3):
            for K in (64, 67, 116):
                dma = route == "summed_dma"
                # B is [k][n] with a column offset into a wider matrix (the d layer_in GEMM reads W_hh's neighbour); an odd ldb
                # takes the one-launch-per-pair form
                out.append(Spec(route, 1, 0, 132, 68, K, a_pad=pad4(K), b_pad=4 if dma else 3, b_off=4 if dma else 3, batch=kcat,
                                flags=16 | (i % 2), bias=i % 3 != 2, c_pad=[5, 0, 4][i % 3], c_off=(i // 2) % 2))
                i += 1
    out += [Spec("summed_dma", 1, 1, 260, 64, 81, a_pad=3, b_pad=3, batch=2, flags=17, bias=True),
            Spec("summed_loop", 0, 0, 130, 68, 67, batch=3, flags=16, bias=True)]
    return out


SUMMED = summed_specs()


@pytest.mark.parametrize("s", SUMMED, ids=ids(SUMMED))
def test_summed_batch(L, cus, s):
    run_case(L, cus, s, 5000 + SUMMED.index(s))


# ----------------------------------------------------------------------------------------------------- workspace mode
def run_workspace(L, cus, s: Spec, seed):
    """flags 8 into a workspace of exactly the advertised size (NaN before, NaN guards behind) + ss_gemm_splitk_reduce."""
    p = plan(s, seed)
    c = p.call
    if not s.real:
        check_exact(p)
    a_d, b_d, c_d = to_dev(p.a), to_dev(p.b), to_dev(p.c)
    r = GR.route(c, dptr(a_d, c.a_base) % 16, dptr(b_d, c.b_base) % 16, cus)
    assert r.name == s.route, f"meant for {s.route}, the dispatcher takes {r.name}"
    need = L.gemm_splitk_ws_floats(c.M, c.N, c.K, c.splits, c.batch)
    assert need == GR.splitk_ws_floats(c.M, c.N, c.K, c.splits, c.batch)
    ws = torch.full((need + 64,), NAN, device="cuda")
    L.call("ss_gemm_f32_batched", *batched_args(L, replace(c, ldc=c.N, stride_c=0), a_d, b_d, c_d, None, None, c_ptr=ws.data_ptr()))
    L.call("ss_gemm_splitk_reduce", ws.data_ptr(), c.M, c.N, c.K, c.splits, c.batch, dptr(c_d, c.c_base), c.ldc, c.stride_c, L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[need:]).all(), "wrote past the advertised workspace"
    want, _, valid = GR.reference_reduced(c, p.a, p.b, p.c)
    assert np.isfinite(want).all()
    return c_d.cpu().numpy(), p, want, valid, r


WORKSPACE = [("dma", 0, 0, 4, 4, 64, 1, 1), ("dma", 0, 0, 128, 64, 200, 3, 2), ("dma", 1, 1, 132, 68, 161, 2, 1), ("staged", 0, 0, 5, 3, 17, 4, 2),
             ("dma", 0, 1, 132, 68, 193, 4, 2)]


@pytest.mark.parametrize("route,a_kc,b_kc,M,N,K,splits,batch", WORKSPACE)
def test_workspace_and_reduce(L, cus, route, a_kc, b_kc, M, N, K, splits, batch):
    mk = dma_spec if route == "dma" else (lambda *a, **k: Spec("staged", *a, **k))
    s = mk(a_kc, b_kc, M, N, K, flags=8, splits=splits, batch=batch, c_pad=3, c_gap=2)
    got, p, want, valid, _ = run_workspace(L, cus, s, 6000 + M + K)
    same_bits("C", got, want.astype(np.float32), valid)


# -------------------------------------------------------------------------------------------------------------- groups
def group_problem(a_kc, b_kc, M, N, K, splits, batch, maps=None, a_pad=0, real=False):
    ra, rb = maps if maps else (IDENT, IDENT)
    return Spec("", a_kc, b_kc, M, N, K, a_pad=a_pad, ra=ra, rb=rb, flags=8, splits=splits, batch=batch, c_pad=2, c_gap=6, real=real)


PAIRED = ((5, 6, 1), (5, 6, 0))   # A rows pair with the B rows before them
P_A = group_problem(0, 0, 132, 68, 200, 3, 2)            # M no multiple of 128 or 192
P_B = group_problem(0, 0, 96, 116, 360, 5, 1)
P_C = group_problem(0, 0, 128, 64, 67, 1, 2, PAIRED)
P_D = group_problem(0, 0, 196, 200, 64, 1, 3)
P_E = group_problem(0, 0, 64, 64, 360, 4, 2, PAIRED)
P_KC1 = group_problem(1, 1, 132, 68, 200, 3, 2, a_pad=4)
P_KC2 = group_problem(1, 1, 60, 132, 64, 1, 1)
P_ODD = group_problem(0, 0, 128, 64, 200, 3, 2, a_pad=1)  # an odd lda
P_MIX = group_problem(1, 0, 132, 68, 200, 3, 1, a_pad=4)  # another layout
P_K20 = group_problem(0, 0, 132, 68, 20, 1, 2)
GROUPS = {
    "dma-1": ("group_dma", 0, [P_A]), "dma-1-map": ("group_dma", 0, [P_C]), "dma-2": ("group_dma", 0, [P_B, P_E]),
    "dma-4": ("group_dma", 0, [P_A, P_B, P_C, P_D]), "dma-2-kc": ("group_dma", 0, [P_KC1, P_KC2]), "dma-kc-wideflag": ("group_dma", 1, [P_KC1, P_KC2]),
    "wide-1": ("group_wide", 1, [P_A]), "wide-1-map": ("group_wide", 1, [P_C]), "wide-2": ("group_wide", 1, [P_B, P_E]),
    "wide-4": ("group_wide", 1, [P_A, P_B, P_C, P_D]), "wide-k20": ("group_wide", 1, [P_K20]), "wide-k20-k67": ("group_wide", 1, [P_K20, P_C, P_E]),
    "fallback-odd": ("group_fallback", 0, [P_A, P_ODD]), "fallback-odd-wideflag": ("group_fallback", 1, [P_ODD, P_C, P_A]),
    "fallback-mixed": ("group_fallback", 0, [P_A, P_MIX]), "fallback-mixed-wideflag": ("group_fallback", 1, [P_MIX, P_B]),
    "fallback-k48": ("group_fallback", 0, [P_A, group_problem(0, 0, 132, 68, 48, 1, 1)]),
}


def run_group(L, cus, route, flags, specs, seed):
    """-> per problem (C as numpy, plan, reference, valid mask), the route."""
    plans = [plan(s, seed + 10 * j) for j, s in enumerate(specs)]
    devs, probs, aligns = [], [], []
    for p, s in zip(plans, specs):
        if not s.real:
            check_exact(p)
        c = p.call
        a_d, b_d, c_d = to_dev(p.a), to_dev(p.b), to_dev(p.c)
        devs.append((a_d, b_d, c_d))
        aligns.append((dptr(a_d, c.a_base) % 16, dptr(b_d, c.b_base) % 16))
        probs.append(L.GemmProblem(c.a_kc, c.b_kc, c.M, c.N, c.K, dptr(a_d, c.a_base), c.lda, *c.ra, dptr(b_d, c.b_base), c.ldb, *c.rb,
                                   dptr(c_d, c.c_base), c.ldc, c.splits, c.batch, c.stride_a, c.stride_b, c.stride_c))
    r = GR.route_group([p.call for p in plans], aligns, flags, cus)
    assert r.name == route, f"meant for {route}, the dispatcher takes {r.name} on {cus} CUs"
    need = L.gemm_group_ws_floats(probs)
    ws = torch.full((need + 64,), NAN, device="cuda")
    arr, n = L.gemm_group(probs)
    L.call("ss_gemm_f32_splitk_group", arr, n, ws.data_ptr(), need, flags, L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[need:]).all(), "wrote past the advertised workspace"
    out = []
    for p, (_, _, c_d) in zip(plans, devs):
        want, _, valid = GR.reference_reduced(p.call, p.a, p.b, p.c)
        assert np.isfinite(want).all()
        out.append((c_d.cpu().numpy(), p, want, valid))
    return out, r


@pytest.mark.parametrize("name", list(GROUPS))
def test_groups(L, cus, name):
    route, flags, specs = GROUPS[name]
    out, _ = run_group(L, cus, route, flags, specs, 7000 + 100 * list(GROUPS).index(name))
    for j, (got, p, want, valid) in enumerate(out):
        same_bits(f"problem {j}", got, want.astype(np.float32), valid)


def test_group_wide_with_more_tiles_than_cus(L, cus):
    """16 x ceil((cus + 1) / 16) tiles of 192 x 192: the plan cannot fit the chip in one round, ends with one K slice per tile and
    launches more workgroups than there are CUs."""
    M, N = 192 * 16, 192 * ceil_div(cus + 1, 16)
    out, r = run_group(L, cus, "group_wide", 1, [replace(group_problem(0, 0, M, N, 64, 1, 1), c_pad=0, c_gap=0)], 7900)
    assert r.wide_nz == (1,) and r.workgroups == 16 * ceil_div(cus + 1, 16) > cus
    got, p, want, valid = out[0]
    same_bits("C", got, want.astype(np.float32), valid)


# -------------------------------------------------------------------------------------------------------- float cases
def float_check(name, got, want, valid, plans_mags, c_indices, K_total, extra):
    worst = 0.0
    for (A, B, c0, bias), idx in zip(plans_mags, c_indices):
        bound = GR.f32_bound(np.abs(A), np.abs(B), K_total, extra, c0=c0, bias=bias)
        err = np.abs(got.astype(np.float64)[idx] - want[idx])
        assert np.isfinite(err).all(), name
        worst = max(worst, float((err / bound).max()))
    print(f"{name}: largest error / bound {worst:.4f} (K_total {K_total}, {extra} further additions)")
    assert K_total <= GR.FLOAT_K_MAX
    assert worst <= 1.0, f"{name}: error {worst:.3f} x the f32 bound"


def float_specs(cus):
    return {
        "staged": Spec("staged", 0, 1, 129, 65, 200, flags=1, splits=3, bias=True, a_pad=1, real=True),
        "dma": dma_spec(1, 0, 132, 68, 200, flags=1, splits=3, bias=True, batch=2, real=True),
        "wide_kc": Spec("wide_kc", 1, 1, 196, 100, 116, batch=wide_batch(196, 100, cus, False), bias=True, share_a=True, real=True),
        "summed_dma": Spec("summed_dma", 1, 0, 132, 68, 116, b_pad=4, b_off=4, batch=3, flags=17, bias=True, real=True),
        "summed_loop": Spec("summed_loop", 1, 0, 132, 68, 116, b_pad=3, b_off=3, batch=3, flags=17, bias=True, real=True),
    }


@pytest.mark.parametrize("route", ["staged", "dma", "wide_kc", "summed_dma", "summed_loop"])
def test_float_batched(L, cus, route):
    """Normal values: |got - float64| <= f32_bound elementwise.  Further additions: bias, accumulate, one per K slice (atomics)
    or per joined pair."""
    s = float_specs(cus)[route]
    got, p, want, valid, r = run_case(L, cus, s, 8000)
    c = p.call
    kcat = c.batch if c.flags & 16 else 1
    idx = [GR.c_index(c, 0)] if c.flags & 16 else [GR.c_index(c, b) for b in range(c.batch)]
    float_check(route, got, want, valid, magnitudes(p), idx, c.K * kcat, int(s.bias) + (c.flags & 1) + r.nz + kcat - 1)
    assert np.array_equal(got[~valid], p.c[~valid])


@pytest.mark.parametrize("route,flags,specs", [
    ("group_dma", 0, [group_problem(0, 0, 132, 68, 200, 3, 2, real=True), group_problem(0, 0, 128, 64, 67, 1, 2, PAIRED, real=True)]),
    ("group_wide", 1, [group_problem(0, 0, 132, 68, 200, 3, 2, real=True), group_problem(0, 0, 128, 64, 67, 1, 2, PAIRED, real=True)]),
    ("group_fallback", 0, [group_problem(0, 0, 132, 68, 200, 3, 2, real=True), group_problem(0, 0, 128, 64, 67, 1, 2, PAIRED, a_pad=1, real=True)])],
    ids=["group_dma", "group_wide", "group_fallback"])
def test_float_groups(L, cus, route, flags, specs):
    """Slabs + reduce: one addition per K slice and the one onto C."""
    out, r = run_group(L, cus, route, flags, specs, 8100)
    for j, (got, p, want, valid) in enumerate(out):
        c = p.call
        nz = r.wide_nz[j] if r.wide_nz else GR.slices(c.K, c.splits)[0]
        float_check(f"{route} problem {j}", got, want, valid, magnitudes(p), [GR.c_index(c, b) for b in range(c.batch)], c.K, nz + 1)
        assert np.array_equal(got[~valid], p.c[~valid])


# ----------------------------------------------------------------------------------------------------------- refusals
def _refusal_call(L, **kw):
    """A small valid call (k-major A, [n][k] B, 8 x 8 x 8, aligned), changed by ``kw``: -> (args builder, C tensor)."""
    a = torch.ones(64, device="cuda")
    b = torch.ones(64, device="cuda")
    c = torch.full((256,), SENT, device="cuda")
    bias = torch.ones(8, device="cuda")
    cs = torch.full((16,), SENT, device="cuda")
    d = dict(a_kc=0, b_kc=1, M=8, N=8, K=8, bias=False, colsum=False, flags=0, splits=1, batch=1, c_off=64)
    d.update(kw)
    args = (d["a_kc"], d["b_kc"], d["M"], d["N"], d["K"], a.data_ptr(), 8, INT_MAX, 0, 0, b.data_ptr(), 8, INT_MAX, 0, 0,
            c.data_ptr() + 4 * d["c_off"], 8, bias.data_ptr() if d["bias"] else None, cs.data_ptr() if d["colsum"] else None,
            d["flags"], d["splits"], d["batch"], 0, 0, 0, 0, 0, L.stream())
    return args, (a, b, c, bias, cs)


REFUSALS = {
    "colsum with a_kcontig": dict(a_kc=1, colsum=True),
    "splits 2 flags 0": dict(splits=2, flags=0),
    "splits 2 flags 3": dict(splits=2, flags=3),
    "always-atomic without accumulate": dict(flags=4),
    "workspace with bias": dict(flags=8, bias=True),
    "workspace misaligned": dict(flags=8, c_off=65),
    "flags 24": dict(flags=24, batch=2),
    "summed batch with colsum": dict(flags=16, colsum=True, batch=2),
    "grid z over 65535": dict(M=1, N=1, K=1, batch=65536),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(L, name):
    """Rejected on the host, before any launch (gemm_prepare and the head of ss_gemm_f32_batched): C and a_colsum keep their bits."""
    args, keep = _refusal_call(L, **REFUSALS[name])
    with pytest.raises(RuntimeError):
        L.call("ss_gemm_f32_batched", *args)
    torch.cuda.synchronize()
    assert torch.all(keep[2] == SENT) and torch.all(keep[4] == SENT)
    # the same call without the fault is taken (the refusal is about the fault, not about the helper)
    ok, keep = _refusal_call(L)
    L.call("ss_gemm_f32_batched", *ok)
    torch.cuda.synchronize()
    assert torch.all(keep[2][64:128] == 8.0) and torch.all(keep[2][:64] == SENT) and torch.all(keep[2][128:] == SENT)


@pytest.mark.parametrize("name", ["n = 0", "n = 5", "ldc < N", "reduce misaligned workspace"])
def test_refusals_group_and_reduce(L, name):
    a = torch.ones(64 * 8, device="cuda")
    b = torch.ones(64 * 8, device="cuda")
    c = torch.full((256,), SENT, device="cuda")
    ws = torch.zeros(1 << 17, device="cuda")
    good = L.GemmProblem(0, 0, 8, 8, 64, a.data_ptr(), 8, INT_MAX, 0, 0, b.data_ptr(), 8, INT_MAX, 0, 0, c.data_ptr() + 256, 8, 1, 1, 0, 0, 0)
    bad = L.GemmProblem(0, 0, 8, 8, 64, a.data_ptr(), 8, INT_MAX, 0, 0, b.data_ptr(), 8, INT_MAX, 0, 0, c.data_ptr() + 256, 7, 1, 1, 0, 0, 0)
    if name == "reduce misaligned workspace":
        with pytest.raises(RuntimeError):
            L.call("ss_gemm_splitk_reduce", ws.data_ptr() + 4, 8, 8, 64, 1, 1, c.data_ptr() + 256, 8, 0, L.stream())
    else:
        probs = {"n = 0": [good], "n = 5": [good] * 5, "ldc < N": [good, bad]}[name]
        arr = (L.GemmProblem * len(probs))(*probs)
        n = 0 if name == "n = 0" else len(probs)
        for wide in (0, 1):  # both forms of the launch
            with pytest.raises(RuntimeError):
                L.call("ss_gemm_f32_splitk_group", arr, n, ws.data_ptr(), ws.numel(), wide, L.stream())
    torch.cuda.synchronize()
    assert torch.all(c == SENT)
