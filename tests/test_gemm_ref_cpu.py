"""The host references of tests/gemm_ref.py, pinned without a GPU: ``reference`` against torch float64 einsum and an explicit
loop, ``route`` against what the comments of csrc/gemm.hip state for a 256-CU part, the exactness condition, and the float
bound against float32 sums in three orders (inside) and bf16-rounded operands (outside)."""
import numpy as np
import pytest
import torch

import gemm_ref as GR
from gemm_ref import IDENT, INT_MAX, Call

NAN = float("nan")


def stored(X, kc, pad, rng):
    """Logical op(X) [rows][K] -> (flat NaN-padded storage, ld) in the layout ``kc`` asks for."""
    st = X if kc else X.T
    ld = st.shape[1] + pad
    buf = np.full((st.shape[0], ld), NAN)
    buf[:, : st.shape[1]] = st
    return buf.reshape(-1), ld


@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("flags,use_bias", [(0, True), (1, False), (2, True), (3, True)])
def test_reference_matches_einsum_unmapped(a_kc, b_kc, flags, use_bias):
    rng = np.random.default_rng(a_kc * 2 + b_kc + 10 * flags)
    batch, M, N, K = 3, 7, 5, 11
    A = rng.standard_normal((batch, M, K))
    B = rng.standard_normal((batch, K, N))
    bias = rng.standard_normal((batch, N))
    C0 = rng.standard_normal((batch, M, N + 2))
    a_parts = [stored(A[b], a_kc, 3, rng) for b in range(batch)]
    b_parts = [stored(B[b].T, b_kc, 1, rng) for b in range(batch)]
    a_buf = np.concatenate([np.full(4, NAN)] + [p[0] for p in a_parts])
    b_buf = np.concatenate([np.full(2, NAN)] + [p[0] for p in b_parts])
    c = Call(a_kc, b_kc, M, N, K, a_parts[0][1], b_parts[0][1], N + 2, flags=flags, batch=batch,
             stride_a=a_parts[0][0].size, stride_b=b_parts[0][0].size, stride_c=M * (N + 2), stride_bias=N,
             a_base=4, b_base=2, c_base=0, bias_base=0 if use_bias else None)
    out, cs, valid = GR.reference(c, a_buf, b_buf, C0.reshape(-1), bias.reshape(-1))
    want = torch.einsum("bmk,bkn->bmn", torch.from_numpy(A), torch.from_numpy(B)).numpy()
    if use_bias:
        want = want + bias[:, None, :]
    if flags & 1:
        want = want + C0[:, :, :N]
    if flags & 2:
        want = np.maximum(want, 0)
    out = out.reshape(batch, M, N + 2)
    np.testing.assert_allclose(out[:, :, :N], want, rtol=0, atol=1e-12)
    assert np.array_equal(out[:, :, N:], C0[:, :, N:]) and cs is None
    assert np.array_equal(valid.reshape(batch, M, N + 2), np.broadcast_to(np.arange(N + 2) < N, (batch, M, N + 2)))


def test_reference_summed_batch_and_colsum():
    rng = np.random.default_rng(3)
    batch, M, N, K = 3, 6, 4, 9
    A = rng.standard_normal((batch, K, M))  # k-major
    B = rng.standard_normal((batch, K, N))
    bias = rng.standard_normal(N)
    c = Call(0, 0, M, N, K, M, N, N, flags=16, batch=batch, stride_a=K * M, stride_b=K * N, stride_c=12345, bias_base=0)
    out, _, valid = GR.reference(c, A.reshape(-1), B.reshape(-1), np.full(M * N, 7.0), bias)
    np.testing.assert_allclose(out.reshape(M, N), np.einsum("bkm,bkn->mn", A, B) + bias, rtol=0, atol=1e-12)
    assert valid.all()
    cs0 = rng.standard_normal((batch, M + 1))
    c = Call(0, 0, M, N, K, M, N, N, batch=batch, stride_a=K * M, stride_b=K * N, stride_c=M * N, stride_colsum=M + 1, colsum_base=0)
    out, cs, _ = GR.reference(c, A.reshape(-1), B.reshape(-1), np.zeros(batch * M * N), None, cs0.reshape(-1))
    want = cs0.copy()
    want[:, :M] += A.sum(1)
    np.testing.assert_allclose(cs.reshape(batch, M + 1), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (0, 0), (1, 0)])
def test_reference_mapped_against_explicit_loop(a_kc, b_kc):
    """G = 5, S = 6, off = 1 on both operands: element by element, the header's formula spelled out."""
    G, S, off = 5, 6, 1
    M, N, K, lda, ldb, ldc = 7, 6, 12, 14, 13, 8
    rng = np.random.default_rng(7)
    a_buf = rng.integers(-3, 4, size=400).astype(np.float64)
    b_buf = rng.integers(-3, 4, size=400).astype(np.float64)
    c_buf = rng.integers(-3, 4, size=M * ldc + 5).astype(np.float64)
    c = Call(a_kc, b_kc, M, N, K, lda, ldb, ldc, ra=(G, S, off), rb=(G, S, off), flags=1, a_base=3, b_base=2, c_base=5)
    out, _, _ = GR.reference(c, a_buf, b_buf, c_buf)
    rm = lambda r: (r // G) * S + r % G + off
    want = c_buf.copy()
    for m in range(M):
        for n in range(N):
            s = 0.0
            for k in range(K):
                a = a_buf[3 + rm(m) * lda + k] if a_kc else a_buf[3 + rm(k) * lda + m]
                b = b_buf[2 + rm(n) * ldb + k] if b_kc else b_buf[2 + rm(k) * ldb + n]
                s += a * b
            want[5 + m * ldc + n] += s
    assert np.array_equal(out, want)


def test_reference_reduced_adds_the_product():
    rng = np.random.default_rng(1)
    A, B, C0 = rng.standard_normal((5, 3)), rng.standard_normal((5, 4)), rng.standard_normal((3, 4))
    c = Call(0, 0, 3, 4, 5, 3, 4, 4, flags=8, splits=2)
    out, _, _ = GR.reference_reduced(c, A.reshape(-1), B.reshape(-1), C0.reshape(-1))
    np.testing.assert_allclose(out.reshape(3, 4), C0 + A.T @ B, rtol=0, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------- route
def proj(M, N, K, batch, **kw):
    """The GRU input projection's call: both operands [row][k], A shared by the batch."""
    return Call(1, 1, M, N, K, kw.pop("lda", K), K, N, batch=batch, stride_b=N * K, stride_c=M * N, stride_bias=N, bias_base=0, **kw)


def test_route_facts_of_the_source_comments_at_256_cus():
    assert GR.route(proj(7680, 576, 384, 2), 0, 0, 256).name == "wide_kc"   # config 2: 40 x 3 x 2 = 240 tiles
    assert GR.route(proj(7680, 576, 116, 2), 0, 0, 256).name == "wide_kc"
    assert GR.route(proj(23040, 576, 180, 2), 0, 0, 256).name == "dma"      # shipped: 720 tiles, several rounds
    assert GR.route(proj(7680, 576, 384, 2), 0, 0, 304).name == "dma"       # 240 tiles are under 80 % of 304 CUs
    assert GR.route(proj(7680, 576, 385, 2, lda=385), 0, 0, 256).name == "staged"  # odd lda
    assert GR.route(Call(1, 1, 256, 128, 48, 48, 48, 128), 0, 0, 256).name == "staged"  # one slice of 48 < 64
    assert GR.route(Call(1, 1, 256, 128, 52, 52, 52, 128), 0, 0, 256).name == "dma"     # 52 rounds up to four k tiles
    assert GR.route(Call(0, 1, 130, 128, 64, 132, 64, 128), 0, 0, 256).name == "staged"  # k-major A, M % 4 != 0
    assert GR.route(Call(0, 1, 132, 128, 64, 132, 64, 128), 0, 0, 256).name == "dma"
    assert GR.route(Call(0, 1, 132, 128, 64, 132, 64, 128), 4, 0, 256).name == "staged"  # A 4 bytes off
    assert GR.route(Call(0, 1, 132, 128, 64, 132, 64, 128, colsum_base=0), 0, 0, 256).name == "staged"
    assert GR.route(Call(1, 1, 7680, 576, 384, 384, 384, 576, batch=2, stride_b=576 * 384, flags=1), 0, 0, 256).name == "dma"
    assert GR.route(Call(1, 1, 7680, 576, 384, 384, 384, 576, batch=2, ra=(INT_MAX, 0, 4)), 0, 0, 256).name == "dma"
    assert GR.route(Call(1, 0, 300, 32, 200, 200, 116, 37, batch=2, flags=16, stride_a=60000, stride_b=23200), 0, 0, 256).name == "summed_dma"
    assert GR.route(Call(1, 0, 130, 70, 50, 50, 73, 75, batch=2, flags=16, stride_a=6500, stride_b=3650), 0, 0, 256).name == "summed_loop"


def test_route_group():
    p = [Call(0, 0, 96, 116, 360, 96, 116, 118, splits=5, batch=2, stride_a=34560, stride_b=41760),
         Call(0, 0, 128, 64, 320, 128, 64, 66, splits=4, batch=2, stride_a=46080, stride_b=23040, ra=(8, 9, 1), rb=(8, 9, 0))]
    al = [(0, 0), (0, 0)]
    assert GR.route_group(p, al, 0, 256).name == "group_dma"
    r = GR.route_group(p, al, 1, 256)
    assert r.name == "group_wide" and r.workgroups <= 256
    odd = [p[0], Call(0, 0, 128, 64, 320, 129, 64, 66, splits=4, batch=2)]
    assert GR.route_group(odd, al, 0, 256).name == "group_fallback"
    assert GR.route_group(odd, al, 1, 256).name == "group_fallback"
    mixed = [p[0], Call(1, 0, 128, 64, 320, 320, 64, 66, splits=4)]
    assert GR.route_group(mixed, al, 0, 256).name == "group_fallback"
    # more 192 x 192 tiles than CUs: the plan ends with one slice per tile and a launch larger than the chip
    big = [Call(0, 0, 192 * 16, 192 * 17, 64, 192 * 16, 192 * 17, 192 * 17)]
    r = GR.route_group(big, [(0, 0)], 1, 256)
    assert r.name == "group_wide" and r.wide_nz == (1,) and r.workgroups == 272
    # config 2, layer 0: 18 tiles of K = 7680 fill 256 CUs with 14 slices each (the comment above the wide kernels)
    l0 = [Call(0, 0, 576, 116, 7680, 576, 116, 116, batch=2, stride_a=4, stride_b=4),
          Call(0, 0, 576, 192, 7680, 576, 192, 192, batch=2, stride_a=4, stride_b=4)]
    assert GR.route_group(l0, al, 1, 256).workgroups <= 256


def test_slices():
    assert GR.slices(200, 3) == (3, 80)
    assert GR.slices(65, 1) == (1, 80)
    assert GR.slices(129, 2) == (2, 80)
    assert GR.slices(161, 2) == (2, 96)
    assert GR.slices(193, 4) == (4, 64)   # the last slice is one element
    assert GR.slices(17, 4) == (2, 16)
    assert GR.splitk_ws_floats(132, 68, 161, 2, 1) == 2 * 2 * 2 * 128 * 64


# --------------------------------------------------------------------------------------------------------- exact range
def test_int_operands_and_exact_range():
    x = GR.int_operands((200, 300), 5)
    assert x.dtype == np.float32 and np.array_equal(x, np.rint(x)) and x.min() == -4 and x.max() == 4
    assert 0.2 < float((x == 0).mean()) < 0.3
    y = GR.int_operands((300, 100), 6)
    assert GR.assert_exact_range([(x, y)]) <= 300 * 16
    big = np.full((2, 1 << 12), 64.0)
    with pytest.raises(AssertionError):
        GR.assert_exact_range([(big, big.T)])             # 4096 * 64 * 64 = 2**24
    GR.assert_exact_range([(big[:, :-1], big.T[:-1])])   # one term fewer fits
    with pytest.raises(AssertionError):
        GR.assert_exact_range([(big[:, :-1], big.T[:-1])], c0=np.full((2, 2), 4096.0))
    with pytest.raises(AssertionError):
        GR.assert_exact_range([(big[:, :2048], big.T[:2048]), (big[:, :2048], big.T[:2048])])  # kcat pairs add up
    with pytest.raises(AssertionError):
        GR.assert_exact_range([(x + 0.5, y)])


# ---------------------------------------------------------------------------------------------------------- float bound
def _pairwise(p):
    while p.shape[1] > 1:
        if p.shape[1] & 1:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], 1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def _rows(K, seed=0, rows=1000):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, K)).astype(np.float32), rng.standard_normal((rows, K)).astype(np.float32)


def _row_bound(a, b):
    # f32_bound takes matrices; one row against one column is its diagonal, which is what the per-row sum computes
    K = a.shape[1]
    return (K + 1) * 2.0**-24 * (np.abs(a).astype(np.float64) * np.abs(b)).sum(1)


def test_f32_bound_matches_its_formula():
    a, b = _rows(37, rows=6)
    got = GR.f32_bound(np.abs(a), np.abs(b).T, 37, 2, c0=np.ones((6, 6)), bias=np.arange(6.0))
    want = 40 * 2.0**-24 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T + 1 + np.arange(6.0)[None, :])
    assert np.array_equal(got, want)
    assert np.allclose(np.diag(GR.f32_bound(np.abs(a), np.abs(b).T, 37, 0)), _row_bound(a, b), rtol=1e-15)


def test_f32_bound_holds_float32_sums_in_any_order():
    a, b = _rows(1920)
    ref = (a.astype(np.float64) * b.astype(np.float64)).sum(1)
    bound = _row_bound(a, b)
    p = a * b
    fwd = np.zeros(1000, np.float32)
    rev = np.zeros(1000, np.float32)
    for k in range(1920):
        fwd = fwd + p[:, k]
        rev = rev + p[:, 1919 - k]
    for name, got in (("forward", fwd), ("reverse", rev), ("pairwise", _pairwise(p))):
        r = float((np.abs(got.astype(np.float64) - ref) / bound).max())
        print(f"{name}: largest error / bound {r:.4f}")
        assert r <= 1.0, name


def test_f32_bound_excludes_bf16_operands():
    """What the float cases of test_gpu_gemm_routes.py rely on: operands rounded to bf16 land outside the bound.

    The bound grows like K**2 (K roundings of a sum of K terms), bf16's rounding noise like sqrt(K), so their ratio falls like
    K**-1.5.  Measured on 1 000 rows of normal values, error / bound over the rows (median, largest; rows outside):
    K = 64: 75, 435, 99 %;  K = 360: 5.8, 31, 91 %;  K = 1920: 0.50, 2.5, 19 %.  At K = 1920 the rows as a set fall outside
    (the largest does) but most single rows do not; up to FLOAT_K_MAX = 360, which the GPU float cases stay under, the
    median row does, nearly six times over."""
    bf = lambda x: torch.from_numpy(x).bfloat16().float().numpy().astype(np.float64)
    stats = {}
    for K in (64, 360, 1920):
        a, b = _rows(K)
        ref = (a.astype(np.float64) * b.astype(np.float64)).sum(1)
        r = np.abs((bf(a) * bf(b)).sum(1) - ref) / _row_bound(a, b)
        stats[K] = (float(np.median(r)), float(r.max()), float((r > 1).mean()))
        print(f"K = {K}: bf16 error / bound median {stats[K][0]:.3f} max {stats[K][1]:.2f}, {100 * stats[K][2]:.1f} % of rows outside")
    assert stats[1920][1] > 1.0
    assert stats[64][0] > 1.0 and stats[360][0] > 1.0
    assert GR.FLOAT_K_MAX == 360
