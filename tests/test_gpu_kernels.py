"""GPU: every HIP kernel, called through the C ABI (ctypes), against the CPU oracle / fp64 math.

Run on the MI355X box with ``python -m pytest tests -m gpu``.  Tolerances are written next to each
check; integer outputs (crop boxes, pool argmaxes, masks) are compared exactly.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_support import L  # noqa: E402, F401
from oracle import features_ref as FR  # noqa: E402
from oracle import model_ref as MR  # noqa: E402

INT_MAX = 2**31 - 1


_KEEP = []


def dev(t):
    """Host -> device copy that stays alive until the next sync(): a bare ``dev(x).data_ptr()`` would free the
    temporary at once and let the caching allocator hand its memory to the next ``dev()`` call."""
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


def sync():
    torch.cuda.synchronize()
    _KEEP.clear()


def report(name, got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    idx = int(err.argmax())
    return f"{name}: max abs err {float(err.max()):.3e} at flat {idx} (got {float(got.reshape(-1)[idx]):.6g}, ref {float(ref.reshape(-1)[idx]):.6g}), ref scale {float(ref.abs().max()):.3e}"


def assert_close(name, got, ref, atol, rtol=0.0):
    g = got.detach().double().cpu()
    r = ref.detach().double().cpu()
    assert g.shape == r.shape, (name, g.shape, r.shape)
    assert torch.isfinite(g).all(), name + " has non-finite values"
    bad = (g - r).abs() > atol + rtol * r.abs()
    if bad.any():
        pytest.fail(report(name, got, ref) + f"; {int(bad.sum())}/{bad.numel()} outside atol={atol} rtol={rtol}", pytrace=False)


# ------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("a_kc,b_kc", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("M,N,K,pad", [(70, 50, 37, 3), (256, 576, 116, 0), (130, 64, 16, 4), (5, 128, 256, 0)])
def test_gemm_layouts(L, a_kc, b_kc, M, N, K, pad):
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    A = torch.randn(M, K, generator=g)
    Bm = torch.randn(K, N, generator=g)
    bias = torch.randn(N, generator=g)
    ref = (A.double() @ Bm.double() + bias.double()).float()
    # storage with a padded leading dimension
    a_st = (A if a_kc else A.t()).contiguous()
    b_st = (Bm.t() if b_kc else Bm).contiguous()
    lda, ldb, ldc = a_st.shape[1] + pad, b_st.shape[1] + pad, N + pad
    a_buf = torch.zeros(a_st.shape[0], lda); a_buf[:, : a_st.shape[1]] = a_st
    b_buf = torch.zeros(b_st.shape[0], ldb); b_buf[:, : b_st.shape[1]] = b_st
    a_d, b_d, bias_d = dev(a_buf), dev(b_buf), dev(bias)
    c_d = torch.full((M, ldc), 7.0, device="cuda")
    L.call("ss_gemm_f32", a_kc, b_kc, M, N, K, a_d.data_ptr(), lda, INT_MAX, 0, 0, b_d.data_ptr(), ldb, INT_MAX, 0, 0,
           c_d.data_ptr(), ldc, bias_d.data_ptr(), None, 0, 1, L.stream())
    sync()
    assert_close("gemm", c_d[:, :N], ref, atol=2e-5 * K ** 0.5, rtol=1e-5)
    if pad:
        assert torch.all(c_d[:, N:] == 7.0), "wrote outside the N columns"


@pytest.mark.parametrize("M,N,K,batch,ldc_pad", [(7680, 576, 384, 2, 0), (7680, 576, 116, 2, 0), (1000, 200, 116, 20, 0),
                                                 (1000, 200, 40, 20, 3), (23040, 576, 180, 2, 0)])
def test_gemm_input_projection_wide_tiles(L, M, N, K, batch, ldc_pad):
    """The GRU input projections (C = A B^T + bias, both operands [row][k], a batch of two directions sharing A) on the 192 x 192
    wide-tile kernel: config 2's shapes, ragged K (116 = 7 x 16 + 4, 40), rows / columns past the last tile, an output whose
    leading dimension rules out 16-byte stores, the shipped shape (T = 90, D = 180)."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    Bm = torch.randn(batch, N, K, generator=g)
    bias = torch.randn(batch, N, generator=g)
    ldc = N + ldc_pad
    a_d, b_d, bias_d = dev(A), dev(Bm), dev(bias)
    c_d = torch.full((batch, M, ldc), 7.0, device="cuda")
    L.call("ss_gemm_f32_batched", 1, 1, M, N, K, a_d.data_ptr(), K, INT_MAX, 0, 0, b_d.data_ptr(), K, INT_MAX, 0, 0, c_d.data_ptr(),
           ldc, bias_d.data_ptr(), None, 0, 1, batch, 0, N * K, M * ldc, N, 0, L.stream())
    sync()
    for b in sorted({0, batch - 1, batch // 2}):
        ref = (A.double() @ Bm[b].double().t() + bias[b].double()).float()
        assert_close(f"input projection, batch entry {b}", c_d[b, :, :N], ref, atol=2e-5 * K ** 0.5, rtol=1e-5)
    if ldc_pad:
        assert torch.all(c_d[:, :, N:] == 7.0), "wrote outside the N columns"


def test_gemm_accumulate_relu_splitk_rowmap(L):
    g = torch.Generator().manual_seed(5)
    # accumulate + relu
    M, N, K = 96, 80, 64
    A, Bm, C0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(M, N, generator=g)
    a_d, b_d, c_d = dev(A), dev(Bm), dev(C0)
    L.call("ss_gemm_f32", 1, 1, M, N, K, a_d.data_ptr(), K, INT_MAX, 0, 0, b_d.data_ptr(), K, INT_MAX, 0, 0,
           c_d.data_ptr(), N, None, None, 3, 1, L.stream())
    sync()
    assert_close("acc+relu", c_d, F.relu(C0.double() + A.double() @ Bm.double().t()).float(), atol=2e-4)
    # split-K with atomics, [K][M] x [K][N] operands and the (b,t)->(b,t-1) row pairing
    Bc, T, Mm, Nn = 6, 9, 48, 40
    dG = torch.randn(Bc * T, Mm, generator=g)
    Hh = torch.randn(Bc * T, Nn, generator=g)
    ref = torch.zeros(Mm, Nn, dtype=torch.float64)
    for b in range(Bc):
        for t in range(1, T):
            ref += torch.outer(dG[b * T + t].double(), Hh[b * T + t - 1].double())
    dg_d, h_d = dev(dG), dev(Hh)
    c_d = torch.zeros(Mm, Nn, device="cuda")
    cs_d = torch.zeros(Mm, device="cuda")
    L.call("ss_gemm_f32", 0, 0, Mm, Nn, Bc * (T - 1), dg_d.data_ptr(), Mm, T - 1, T, 1, h_d.data_ptr(), Nn, T - 1, T, 0,
           c_d.data_ptr(), Nn, None, cs_d.data_ptr(), 1, 3, L.stream())
    sync()
    assert_close("splitk+rowmap", c_d, ref.float(), atol=3e-4)
    cs_ref = dG.view(Bc, T, Mm)[:, 1:].double().sum((0, 1)).float()
    assert_close("a_colsum", cs_d, cs_ref, atol=1e-4)


@pytest.mark.parametrize("M,N,K,splits,batch", [(576, 116, 1920, 7, 2), (200, 70, 333, 4, 1), (48, 40, 64, 5, 3)])
def test_gemm_splitk_workspace(L, M, N, K, splits, batch):
    """K slices left in a scratch buffer + the reduce pass == accumulate with one GEMM (the weight-gradient path)."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(batch, K, M, generator=g)
    Bm = torch.randn(batch, K, N, generator=g)
    C0 = torch.randn(batch, M, N + 3, generator=g)
    ref = C0.clone()
    ref[:, :, :N] += torch.einsum("bkm,bkn->bmn", A.double(), Bm.double()).float()
    a_d, b_d, c_d = dev(A), dev(Bm), dev(C0)
    need = L.gemm_splitk_ws_floats(M, N, K, splits, batch)
    ws = torch.full((need + 8,), float("nan"), device="cuda")
    L.call("ss_gemm_f32_batched", 0, 0, M, N, K, a_d.data_ptr(), M, INT_MAX, 0, 0, b_d.data_ptr(), N, INT_MAX, 0, 0,
           ws.data_ptr(), N, None, None, 8, splits, batch, K * M, K * N, 0, 0, 0, L.stream())
    L.call("ss_gemm_splitk_reduce", ws.data_ptr(), M, N, K, splits, batch, c_d.data_ptr(), N + 3, M * (N + 3), L.stream())
    sync()
    assert_close("splitk workspace", c_d, ref, atol=2e-5 * K ** 0.5, rtol=1e-5)
    assert torch.isnan(ws[need:]).all(), "wrote past the advertised workspace size"


@pytest.mark.parametrize("rows,cols,lda", [(300000, 8, 8), (131072, 16, 16), (70001, 24, 24), (50000, 24, 40), (777, 384, 1152)])
def test_colsum(L, rows, cols, lda):
    """out[c] += sum_r A[r][c]: the tall-and-narrow packed form (flat stream, the per-pixel gradients of the layer-by-layer CNN)
    and the general strided one."""
    g = torch.Generator().manual_seed(rows + cols)
    A = torch.randn(rows, lda, generator=g)
    out0 = torch.randn(cols, generator=g)
    a_d, o_d = dev(A), dev(out0)
    L.call("ss_colsum_f32", a_d.data_ptr(), rows, cols, lda, o_d.data_ptr(), L.stream())
    sync()
    ref = (out0.double() + A[:, :cols].double().sum(0)).float()
    assert_close("colsum", o_d, ref, atol=2e-5 * rows ** 0.5, rtol=1e-5)


@pytest.mark.parametrize("aligned,wide", [(True, 0), (False, 0), (True, 1), (False, 1)])
def test_gemm_splitk_group(L, aligned, wide):
    """Three split-K problems of different shapes, K and row maps in one grouped launch == each alone (fp64 reference).
    ``aligned=False`` gives one problem an odd leading dimension: the whole group then takes the problem-by-problem fallback.
    ``wide=1``: flags bit 0, the 192 x 192-tile form for launches that have the chip to themselves (ragged last k tile, rows past
    M / N clamped, both row maps)."""
    g = torch.Generator().manual_seed(11)
    Bc, T = 40, 9  # K slices of >= 64 rows, or the DMA-fed kernel (and with it the grouped launch) is not taken
    Nrows = Bc * T
    specs = [(96, 116, Nrows, 5, None), (128, 64, Bc * (T - 1), 4, (T - 1, T)), (64, 64, Bc * (T - 1), 3, (T - 1, T))]
    probs, refs, outs, keep = [], [], [], []
    for j, (M, N, K, splits, rmap) in enumerate(specs):
        lda = M + (0 if (aligned or j != 1) else 1)
        A = torch.randn(2, Nrows, lda, generator=g)
        Bm = torch.randn(2, Nrows, N, generator=g)
        C0 = torch.randn(2, M, N + 2, generator=g)
        ref = C0.clone().double()
        for b in range(2):
            if rmap is None:
                ref[b, :, :N] += A[b, :, :M].double().t() @ Bm[b].double()
            else:  # rows (clip, t>=1) of A pair with rows (clip, t-1) of B
                a = A[b, :, :M].view(Bc, T, M)[:, 1:].reshape(-1, M).double()
                bb = Bm[b].view(Bc, T, N)[:, :-1].reshape(-1, N).double()
                ref[b, :, :N] += a.t() @ bb
        a_d, b_d, c_d = dev(A), dev(Bm), dev(C0)
        keep += [a_d, b_d]
        am = (INT_MAX, 0, 0) if rmap is None else (rmap[0], rmap[1], 1)
        bm = (INT_MAX, 0, 0) if rmap is None else (rmap[0], rmap[1], 0)
        probs.append(L.GemmProblem(0, 0, M, N, K, a_d.data_ptr(), lda, am[0], am[1], am[2], b_d.data_ptr(), N, bm[0], bm[1], bm[2],
                                   c_d.data_ptr(), N + 2, splits, 2, Nrows * lda, Nrows * N, M * (N + 2)))
        refs.append(ref.float())
        outs.append(c_d)
    need = L.gemm_group_ws_floats(probs)
    ws = torch.full((need + 8,), float("nan"), device="cuda")
    arr, n = L.gemm_group(probs)
    L.call("ss_gemm_f32_splitk_group", arr, n, ws.data_ptr(), ws.numel(), wide, L.stream())
    sync()
    for j in range(3):
        assert_close(f"group problem {j}", outs[j], refs[j], atol=3e-4, rtol=1e-5)
    assert torch.isnan(ws[need:]).all(), "wrote past the advertised workspace size"
    # a scratch buffer that is too short is refused, not overrun
    with pytest.raises(RuntimeError):
        L.call("ss_gemm_f32_splitk_group", arr, n, ws.data_ptr(), need - 1, wide, L.stream())


@pytest.mark.parametrize("M,N,K,ldb_extra", [(7680, 384, 576, 0), (300, 32, 200, 84), (130, 70, 50, 3)])
def test_gemm_summed_batch(L, M, N, K, ldb_extra):
    """flags bit4: C = bias + A0 B0 + A1 B1 in one launch (the d layer_in GEMM of both GRU directions); the last case is
    unaligned and takes the one-launch-per-pair fallback."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(2, M, K, generator=g)                 # [row][k]
    Bm = torch.randn(2, K, N + ldb_extra, generator=g)    # [k][n], only the last N columns are used
    bias = torch.randn(N, generator=g)
    ref = (torch.einsum("bmk,bkn->mn", A.double(), Bm[:, :, ldb_extra:].double()) + bias.double()).float()
    a_d, b_d, bias_d = dev(A), dev(Bm), dev(bias)
    c_d = torch.full((M, N + 5), 7.0, device="cuda")
    L.call("ss_gemm_f32_batched", 1, 0, M, N, K, a_d.data_ptr(), K, INT_MAX, 0, 0, b_d.data_ptr() + 4 * ldb_extra,
           N + ldb_extra, INT_MAX, 0, 0, c_d.data_ptr(), N + 5, bias_d.data_ptr(), None, 16, 1, 2, M * K, K * (N + ldb_extra), 0,
           0, 0, L.stream())
    sync()
    assert_close("summed batch", c_d[:, :N], ref, atol=2e-5 * (2 * K) ** 0.5, rtol=1e-5)
    assert torch.all(c_d[:, N:] == 7.0)


# ------------------------------------------------------------------------------------- GRU
def _gru_case(H, In, B, T, seed, lengths=None):
    g = torch.Generator().manual_seed(seed)
    a = 1.5 / H ** 0.5
    mk = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * a
    sd = {}
    for suf in ("", "_reverse"):
        sd[f"gru.weight_ih_l0{suf}"] = mk(3 * H, In)
        sd[f"gru.weight_hh_l0{suf}"] = mk(3 * H, H)
        sd[f"gru.bias_ih_l0{suf}"] = mk(3 * H)
        sd[f"gru.bias_hh_l0{suf}"] = mk(3 * H)
    x = torch.randn(B, T, In, generator=g)
    if lengths is None:
        lengths = torch.randint(1, T + 1, (B,), generator=g)
        lengths[0] = T
        if B > 2:
            lengths[2] = 1
    return sd, x, torch.as_tensor(lengths, dtype=torch.int64)


@pytest.mark.parametrize("split", [False, True], ids=["one_cu", "multi_cu"])
@pytest.mark.parametrize("H,B,T", [(192, 5, 7), (192, 37, 12), (64, 3, 20), (192, 16, 1), (192, 130, 30), (64, 250, 9)])
def test_gru_fwd_bwd(L, H, B, T, split):
    """split=True hands the kernels a sync workspace: the (slice, direction) recurrences then run on several CUs each
    and exchange their state through `out` / `d_g`; three launches share the workspace (generation counter)."""
    _check_gru_fwd_bwd(L, H, B, T, split)


def _check_gru_fwd_bwd(L, H, B, T, split, lengths=None, gen0=0):
    """Body of test_gru_fwd_bwd.  ``lengths`` replaces the random ones of _gru_case; ``gen0`` is the launch generation the sync
    header holds before the first launch (int32 bits).  Returns the kernels' outputs and the sync workspace."""
    In = 20
    sync_ws = None
    if split:
        nb = L.gru_sync_bytes(B, T, H)
        if nb == 0:
            pytest.skip("shape always takes the one-CU-per-slice kernels")
        sync_ws = torch.zeros(nb // 4, device="cuda", dtype=torch.int32)
        sync_ws[0] = gen0
    sw = L.ptr(sync_ws)
    sd, x, lengths = _gru_case(H, In, B, T, seed=H + B + T, lengths=lengths)
    N = B * T
    # reference: explicit masked GRU on CPU with autograd
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xg = x.clone().requires_grad_(True)
    gi_ref = [F.linear(xg, leaves["gru.weight_ih_l0" + s], leaves["gru.bias_ih_l0" + s]) for s in ("", "_reverse")]
    for t_ in gi_ref:
        t_.retain_grad()

    def direction(gi_all, suf, reverse):
        h = x.new_zeros(B, H)
        outs = [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            valid = (lengths > t).float().unsqueeze(1)
            hn = MR.gru_cell(gi_all[:, t], h, leaves["gru.weight_hh_l0" + suf], leaves["gru.bias_hh_l0" + suf])
            h = valid * hn + (1 - valid) * h
            outs[t] = valid * h
        return torch.stack(outs, 1)

    out_ref = torch.cat([direction(gi_ref[0], "", False), direction(gi_ref[1], "_reverse", True)], 2)
    wgt = torch.randn(B, T, 2 * H, generator=torch.Generator().manual_seed(1))
    (out_ref * wgt).sum().backward()

    gi_d = dev(torch.stack([gi_ref[0].detach().reshape(N, 3 * H), gi_ref[1].detach().reshape(N, 3 * H)]))
    P = {k: dev(v) for k, v in sd.items()}
    len_d = dev(lengths.to(torch.int32))
    out_d = torch.full((N, 2 * H), 9.0, device="cuda")
    save_d = torch.zeros(2, N, 4, H, device="cuda")
    L.call("ss_gru_fwd", gi_d.data_ptr(), P["gru.weight_hh_l0"].data_ptr(), P["gru.weight_hh_l0_reverse"].data_ptr(),
           P["gru.bias_hh_l0"].data_ptr(), P["gru.bias_hh_l0_reverse"].data_ptr(), len_d.data_ptr(), B, T, H,
           out_d.data_ptr(), save_d.data_ptr(), sw, L.stream())
    sync()
    assert_close("gru out", out_d.view(B, T, 2 * H), out_ref, atol=2e-5)
    # inference form (no stash) gives the same bits
    out2 = torch.empty_like(out_d)
    L.call("ss_gru_fwd", gi_d.data_ptr(), P["gru.weight_hh_l0"].data_ptr(), P["gru.weight_hh_l0_reverse"].data_ptr(),
           P["gru.bias_hh_l0"].data_ptr(), P["gru.bias_hh_l0_reverse"].data_ptr(), len_d.data_ptr(), B, T, H,
           out2.data_ptr(), None, sw, L.stream())
    sync()
    assert torch.equal(out2, out_d)
    # nn.GRU's inter-layer dropout as a by-product of the multi-CU kernel: the same bits as ss_dropout on the finished output;
    # the one-CU form refuses (the caller then runs ss_dropout)
    out3, od3 = torch.empty_like(out_d), torch.full_like(out_d, 7.0)
    args = (gi_d.data_ptr(), P["gru.weight_hh_l0"].data_ptr(), P["gru.weight_hh_l0_reverse"].data_ptr(), P["gru.bias_hh_l0"].data_ptr(),
            P["gru.bias_hh_l0_reverse"].data_ptr(), len_d.data_ptr(), B, T, H, out3.data_ptr(), None, od3.data_ptr(), 0.2, 1234, 5 << 40, sw,
            L.stream())
    if sw is None:
        with pytest.raises(RuntimeError):
            L.call("ss_gru_fwd_drop", *args)
    else:
        L.call("ss_gru_fwd_drop", *args)
        od_ref = torch.empty_like(out_d)
        L.call("ss_dropout", out_d.data_ptr(), od_ref.data_ptr(), N * 2 * H, 0.2, 1234, 5 << 40, None, L.stream())
        sync()
        assert torch.equal(out3, out_d) and torch.equal(od3, od_ref)

    dout_d = dev(wgt.reshape(N, 2 * H))
    dg_d = torch.full((2, N, 4, H), 5.0, device="cuda")
    gb_d = torch.full((4, 3 * H), 0.5, device="cuda")  # bias gradients ride on the BPTT: (ih_f, hh_f, ih_r, hh_r), accumulated
    L.call("ss_gru_bwd", dout_d.data_ptr(), out_d.data_ptr(), save_d.data_ptr(), P["gru.weight_hh_l0"].data_ptr(),
           P["gru.weight_hh_l0_reverse"].data_ptr(), len_d.data_ptr(), B, T, H, dg_d.data_ptr(), 0.0, 0, 0,
           gb_d[0].data_ptr(), gb_d[1].data_ptr(), gb_d[2].data_ptr(), gb_d[3].data_ptr(), sw, L.stream())
    sync()
    for d in range(2):
        colsum = dg_d[d].double().sum(0)  # (4, H)
        assert_close(f"fused d b_ih dir{d}", gb_d[2 * d], (colsum[:3].reshape(-1) + 0.5).float(), atol=2e-4, rtol=1e-4)
        assert_close(f"fused d b_hh dir{d}", gb_d[2 * d + 1],
                     (torch.cat([colsum[0], colsum[1], colsum[3]]) + 0.5).float(), atol=2e-4, rtol=1e-4)
    if split:
        assert int(sync_ws[2]) == 0, "a wait on a partner workgroup timed out"
        # four launches (three forward, one backward), each closed its generation
        assert (int(sync_ws[0]) - gen0) % 2**32 == 4 and int(sync_ws[1]) == 0
    # inter-layer dropout fused into the read of d_out == ss_dropout on d_out first, bit for bit
    p_drop, seed, off = 0.25, 1234567, 3 << 40
    dmask = torch.empty_like(dout_d)
    L.call("ss_dropout", dout_d.data_ptr(), dmask.data_ptr(), N * 2 * H, p_drop, seed, off, None, L.stream())
    dg_a, dg_b = torch.zeros_like(dg_d), torch.zeros_like(dg_d)
    for src, dst, pp in ((dmask, dg_a, 0.0), (dout_d, dg_b, p_drop)):
        L.call("ss_gru_bwd", src.data_ptr(), out_d.data_ptr(), save_d.data_ptr(), P["gru.weight_hh_l0"].data_ptr(),
               P["gru.weight_hh_l0_reverse"].data_ptr(), len_d.data_ptr(), B, T, H, dst.data_ptr(), pp, seed, off, None, None, None, None,
               sw, L.stream())
    sync()
    assert float((dmask == 0).float().mean()) > 0.15
    if split:
        assert_close("fused dropout", dg_b, dg_a, atol=1e-6, rtol=1e-5)  # reduce-scatter order is timing dependent? no: fixed
    else:
        assert torch.equal(dg_a, dg_b)
    for d in range(2):
        dgi_ref = gi_ref[d].grad.reshape(N, 3 * H)
        assert_close(f"d gi dir{d}", dg_d[d, :, :3].reshape(N, 3 * H), dgi_ref, atol=3e-5, rtol=1e-4)
        suf = "" if d == 0 else "_reverse"
        # 4th block = d(W_hn h + b_hn): its column sum is the n-part of d b_hh
        db_hh = leaves["gru.bias_hh_l0" + suf].grad
        assert_close(f"d b_hh n dir{d}", dg_d[d, :, 3].sum(0), db_hh[2 * H:], atol=2e-4, rtol=1e-4)
        assert_close(f"d b_hh rz dir{d}", dg_d[d, :, :2].reshape(N, 2 * H).sum(0), db_hh[: 2 * H], atol=2e-4, rtol=1e-4)
    if split:
        assert int(sync_ws[2]) == 0 and (int(sync_ws[0]) - gen0) % 2**32 == 6  # and the two backward launches with dropout
    return dict(out=out_d, out2=out2, out3=out3, od3=od3, dg=dg_d, gb=gb_d, dg_a=dg_a, dg_b=dg_b), sync_ws


# Batches padded past their longest clip, as the reference trains (MAX_T = 90, train_model_official.py:93-117): the first
# T - max(len) steps of the reverse recurrence run with no valid clip in the batch -- in the multi-CU form whole sweeps that
# publish zero state -- and the last T - max(len) forward steps emit nothing.
GRU_PADDED = [
    (192, 5, 7, [3, 1, 6, 2, 5]),
    (192, 16, 6, [1] * 16),                                              # every clip one frame long
    (192, 37, 12, [1 + (5 * b) % 9 for b in range(37)]),                 # max 9 of 12, three slices
    (64, 250, 9, [1 + (3 * b) % 7 for b in range(250)]),
    (192, 16, 90, [53, 17, 1, 34] + [2 + (11 * b) % 87 for b in range(12)]),   # the shipped MAX_T, max(len) = 88
    (192, 130, 90, [1 + (7 * b) % 80 for b in range(130)]),
]


@pytest.mark.parametrize("split", [False, True], ids=["one_cu", "multi_cu"])
@pytest.mark.parametrize("H,B,T,lengths", GRU_PADDED, ids=[f"H{h}-B{b}-T{t}-max{max(n)}" for h, b, t, n in GRU_PADDED])
def test_gru_fwd_bwd_padded_past_the_longest_clip(L, H, B, T, lengths, split):
    assert max(lengths) < T and len(lengths) == B
    _check_gru_fwd_bwd(L, H, B, T, split, lengths=lengths)


@pytest.mark.parametrize("T", [1022, 1023])
def test_gru_fwd_bwd_at_the_step_tag_limit(L, T):
    """Step tags are 10 bits (granule_xchg.h, XCHG_MAX_T = 1022): T = 1022 is the longest clip the multi-CU recurrence takes, at
    T = 1023 gru_sync_bytes says 0 and the one-CU kernels run.  Both sides against the reference, ragged, max(len) < T on one side."""
    H, B = 192, 3
    nb = L.gru_sync_bytes(B, T, H)
    assert (nb > 0) == (T <= 1022), nb
    lengths = [T, 1, 700] if T == 1022 else [1022, 5, 700]
    _check_gru_fwd_bwd(L, H, B, T, nb > 0, lengths=lengths)


@pytest.mark.parametrize("gen0", [2**22 - 2, -2], ids=["gen_2^22-2", "gen_2^32-2"])
def test_gru_split_generation_wrap(L, gen0):
    """The launch generation is masked to 22 bits in the step tags ((gen & 0x3FFFFF) << 10, xchg_tag_base in granule_xchg.h) and is a 32-bit
    counter in the header: a graph replayed for every served window reaches both wraps.  The six launches of test_gru_fwd_bwd
    across each wrap give the bits a fresh workspace gives, and no bounded wait gives up (a wrong tag shows as NaN plus a
    time-out count in sync[2], not as a hang)."""
    H, B, T = 192, 37, 12
    lengths = [T] + [1 + (5 * b) % 9 for b in range(B - 1)]
    fresh, ws0 = _check_gru_fwd_bwd(L, H, B, T, True, lengths=lengths)
    wrapped, ws1 = _check_gru_fwd_bwd(L, H, B, T, True, lengths=lengths, gen0=gen0)
    assert int(ws0[0]) == 6 and int(ws1[0]) == gen0 + 6  # (int32: -2 + 6 launches = 4 past the 32-bit wrap)
    assert int(ws1[2]) == 0 and int(ws1[1]) == 0
    for k, v in fresh.items():
        if k == "gb":  # the bias-gradient column sums are float atomics over the 16-clip slices: their order is the scheduler's
            assert float((wrapped[k] - v).abs().max()) <= 1e-6 * max(1.0, float(v.abs().max())), k
        else:
            assert torch.equal(wrapped[k], v), k


# ------------------------------------------------------------------------------------- AttnPool / LayerNorm / CE
def test_attn_pool(L):
    _check_attn_pool(L, 7, 11, [11, 1, 5, 11, 2, 7, 3])


# every column >= max(len) is masked for every clip: the softmax of each row runs over its clip alone
ATTN_PADDED = [(7, 11, [4, 1, 5, 9, 2, 7, 3]), (5, 90, [1] * 5), (16, 90, [53, 17, 1, 34] + [2 + (11 * b) % 87 for b in range(12)])]


@pytest.mark.parametrize("B,T,lengths", ATTN_PADDED, ids=[f"B{b}-T{t}-max{max(n)}" for b, t, n in ATTN_PADDED])
def test_attn_pool_padded_past_the_longest_clip(L, B, T, lengths):
    assert max(lengths) < T
    _check_attn_pool(L, B, T, lengths)


def _check_attn_pool(L, B, T, lengths):
    D = 384
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, T, D, generator=g)
    lengths = torch.tensor(lengths)
    for b in range(B):
        h[b, lengths[b]:] = 0
    sd = {"pool.score.weight": torch.randn(1, D, generator=g) * 0.2, "pool.score.bias": torch.randn(1, generator=g)}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    hg = h.clone().requires_grad_(True)
    pooled_ref = MR.attn_pool(hg, lengths, leaves)
    dp = torch.randn(B, D, generator=g)
    (pooled_ref * dp).sum().backward()
    h_d, len_d, w_d, b_d = dev(h), dev(lengths.to(torch.int32)), dev(sd["pool.score.weight"]), dev(sd["pool.score.bias"])
    attn = torch.empty(B, T, device="cuda")
    pooled = torch.empty(B, D, device="cuda")
    L.call("ss_attn_pool_fwd", h_d.data_ptr(), len_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), B, T, D,
           attn.data_ptr(), pooled.data_ptr(), L.stream())
    sync()
    assert_close("pooled", pooled, pooled_ref, atol=2e-6, rtol=1e-5)
    assert_close("attn rows sum to 1", attn.sum(1), torch.ones(B), atol=1e-6)
    dh = torch.full((B, T, D), 3.0, device="cuda")
    gw, gb = torch.zeros(D, device="cuda"), torch.zeros(1, device="cuda")
    L.call("ss_attn_pool_bwd", h_d.data_ptr(), len_d.data_ptr(), w_d.data_ptr(), attn.data_ptr(), dev(dp).data_ptr(), B, T,
           D, dh.data_ptr(), gw.data_ptr(), gb.data_ptr(), L.stream())
    sync()
    mask = (torch.arange(T).unsqueeze(0) < lengths.unsqueeze(1)).unsqueeze(-1)
    assert_close("d h", dh, hg.grad * mask, atol=3e-6, rtol=1e-5)
    gw_ref = leaves["pool.score.weight"].grad.reshape(-1)
    assert_close("d w_score", gw, gw_ref, atol=2e-6 * float(gw_ref.abs().max()), rtol=1e-5)
    assert abs(float(gb)) < 1e-5


def test_layernorm(L):
    B, D = 9, 384
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, D, generator=g) * 3 + 1
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    xg, gg, bg = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = F.layer_norm(xg, (D,), gg, bg, 1e-5)
    dy = torch.randn(B, D, generator=g)
    (y_ref * dy).sum().backward()
    y, xhat, rstd = (torch.empty(B, D, device="cuda"), torch.empty(B, D, device="cuda"), torch.empty(B, device="cuda"))
    x_d, g_d, b_d = dev(x), dev(gamma), dev(beta)
    L.call("ss_layernorm_fwd", x_d.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), B, D, 1e-5, y.data_ptr(), xhat.data_ptr(),
           rstd.data_ptr(), L.stream())
    dx, ggam, gbet = torch.empty(B, D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    L.call("ss_layernorm_bwd", dev(dy).data_ptr(), xhat.data_ptr(), rstd.data_ptr(), g_d.data_ptr(), B, D, dx.data_ptr(),
           ggam.data_ptr(), gbet.data_ptr(), L.stream())
    sync()
    assert_close("ln y", y, y_ref, atol=3e-6, rtol=1e-5)
    assert_close("ln dx", dx, xg.grad, atol=3e-6, rtol=1e-5)
    assert_close("ln dgamma", ggam, gg.grad, atol=1e-5, rtol=1e-5)
    assert_close("ln dbeta", gbet, bg.grad, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("B,T,C,Hd", [(7, 11, 5, 192), (33, 30, 10, 192), (2, 90, 100, 192), (5, 30, 100, 512), (3, 9, 7, 250)])
def test_fused_tail_fwd_bwd(L, B, T, C, Hd):
    """ss_tail_fwd / ss_tail_bwd (AttnPool + head + CE in one launch per direction) against the oracle's autograd.
    Hd = 512 is config 5's width (2H = 1024: the columns beyond the forward kernel's register prefetch), 250 a width that is
    no multiple of the 64-lane column groups."""
    _check_fused_tail(L, B, T, C, Hd)


TAIL_PADDED = [(7, 11, 5, 192, [4, 1, 5, 9, 2, 7, 3]), (4, 90, 10, 192, [53, 17, 1, 34]), (3, 9, 7, 250, [1, 1, 1]),
               (5, 90, 100, 512, [89, 1, 40, 7, 66])]


@pytest.mark.parametrize("B,T,C,Hd,lengths", TAIL_PADDED, ids=[f"B{b}-T{t}-C{c}-Hd{h}-max{max(n)}" for b, t, c, h, n in TAIL_PADDED])
def test_fused_tail_fwd_bwd_padded_past_the_longest_clip(L, B, T, C, Hd, lengths):
    assert max(lengths) < T
    _check_fused_tail(L, B, T, C, Hd, lengths)


def _check_fused_tail(L, B, T, C, Hd, lengths=None):
    D, MID = 2 * Hd, 128
    import weights as W

    g = torch.Generator().manual_seed(B * 7 + T)
    sd = {k: v for k, v in W.make_state_dict(31 + B, 84, C, False, hidden=Hd).items() if k.startswith(("pool.", "head."))}
    h = torch.randn(B, T, D, generator=g)
    drawn = torch.randint(1, T + 1, (B,), generator=g)
    if lengths is None:
        lengths = drawn
        lengths[0] = T
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    for b in range(B):
        h[b, lengths[b]:] = 0
    y = torch.randint(0, C, (B,), generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    hg = h.clone().requires_grad_(True)
    pooled = MR.attn_pool(hg, lengths, leaves)
    logits_ref = MR.head(pooled, leaves)
    loss_ref = MR.ce_label_smoothing(logits_ref, y)
    loss_ref.backward()

    P = {k: dev(v) for k, v in sd.items()}
    h_d, len_d, y_d = dev(h), dev(lengths.to(torch.int32)), dev(y)
    f = lambda *s: torch.empty(*s, device="cuda")
    attn, xhat, rstd, ln, mid, mid_d = f(B, T), f(B, D), f(B), f(B, D), f(B, MID), f(B, MID)
    logits, d_logits = f(B, C), f(B, C)
    loss = torch.zeros(1, device="cuda")
    correct = torch.zeros(1, device="cuda", dtype=torch.int32)
    L.call("ss_tail_fwd", h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["pool.score.bias"].data_ptr(),
           P["head.0.weight"].data_ptr(), P["head.0.bias"].data_ptr(), P["head.1.weight"].data_ptr(),
           P["head.1.bias"].data_ptr(), P["head.4.weight"].data_ptr(), P["head.4.bias"].data_ptr(), y_d.data_ptr(), B, T, D,
           MID, C, 1e-5, 0.0, 0, 0, 0.05, float(B), attn.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), ln.data_ptr(),
           mid.data_ptr(), mid_d.data_ptr(), logits.data_ptr(), d_logits.data_ptr(), loss.data_ptr(), correct.data_ptr(),
           L.stream())
    sync()
    assert_close("tail logits", logits, logits_ref, atol=3e-6 if Hd == 192 else 1e-5, rtol=1e-5)
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 3e-6 * max(1.0, abs(float(loss_ref.detach())))
    assert int(correct) == int((logits_ref.argmax(1) == y).sum())
    assert torch.equal(mid, mid_d)  # p = 0
    # inference form: no stash, no loss, same logits
    logits2 = f(B, C)
    L.call("ss_tail_fwd", h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["pool.score.bias"].data_ptr(),
           P["head.0.weight"].data_ptr(), P["head.0.bias"].data_ptr(), P["head.1.weight"].data_ptr(),
           P["head.1.bias"].data_ptr(), P["head.4.weight"].data_ptr(), P["head.4.bias"].data_ptr(), None, B, T, D, MID, C,
           1e-5, 0.0, 0, 0, 0.0, 1.0, None, None, None, None, None, None, logits2.data_ptr(), None, None, None, L.stream())
    sync()
    assert torch.equal(logits2, logits)

    d_mid, d_h = f(B, MID), torch.full((B, T, D), 3.0, device="cuda")
    gg, gb, gw, gs = (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"),
                      torch.zeros(1, device="cuda"))
    L.call("ss_tail_bwd", h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["head.0.weight"].data_ptr(),
           P["head.1.weight"].data_ptr(), P["head.4.weight"].data_ptr(), attn.data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
           mid.data_ptr(), d_logits.data_ptr(), B, T, D, MID, C, 0.0, 0, 0, d_mid.data_ptr(), d_h.data_ptr(), gg.data_ptr(),
           gb.data_ptr(), gw.data_ptr(), gs.data_ptr(), None, L.stream())
    # the same with the per-clip scratch rows + column sums instead of float atomics on the three D-vectors
    part = torch.full((B, 3, D), 9.0, device="cuda")
    g3 = torch.zeros(3, D, device="cuda")
    gs2, d_h2, d_mid2 = torch.zeros(1, device="cuda"), torch.empty(B, T, D, device="cuda"), f(B, MID)
    L.call("ss_tail_bwd", h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["head.0.weight"].data_ptr(),
           P["head.1.weight"].data_ptr(), P["head.4.weight"].data_ptr(), attn.data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
           mid.data_ptr(), d_logits.data_ptr(), B, T, D, MID, C, 0.0, 0, 0, d_mid2.data_ptr(), d_h2.data_ptr(), g3[0].data_ptr(),
           g3[1].data_ptr(), g3[2].data_ptr(), gs2.data_ptr(), part.data_ptr(), L.stream())
    for k in range(3):
        L.call("ss_colsum_f32", part.data_ptr() + 4 * k * D, B, D, 3 * D, g3[k].data_ptr(), L.stream())
    sync()
    assert torch.equal(d_h2, d_h) and torch.equal(d_mid2, d_mid)
    for k, ref_t in enumerate((gg, gb, gw)):
        assert_close(f"col_part {k}", g3[k], ref_t, atol=2e-5 * float(ref_t.abs().max()) + 1e-8, rtol=1e-4)
    assert_close("col_part b_score", gs2, gs, atol=1e-6, rtol=1e-5)
    mask = (torch.arange(T).unsqueeze(0) < lengths.unsqueeze(1)).unsqueeze(-1)
    scale = float(hg.grad.abs().max())
    assert_close("tail d_h", d_h, hg.grad * mask, atol=2e-5 * scale, rtol=1e-4)
    for name, got, key in (("d gamma", gg, "head.0.weight"), ("d beta", gb, "head.0.bias"), ("d w_score", gw, "pool.score.weight")):
        ref = leaves[key].grad.reshape(-1)
        assert_close(name, got, ref, atol=2e-5 * float(ref.abs().max()) + 1e-8, rtol=1e-4)
    # the two Linear weight gradients are GEMMs over what the kernels stashed
    dW1 = d_mid.t() @ ln
    dW4 = d_logits.t() @ mid_d
    assert_close("dW1 via stash", dW1, leaves["head.1.weight"].grad, atol=2e-5 * float(leaves["head.1.weight"].grad.abs().max()), rtol=1e-4)
    assert_close("dW4 via stash", dW4, leaves["head.4.weight"].grad, atol=2e-5 * float(leaves["head.4.weight"].grad.abs().max()), rtol=1e-4)
    # dropout in the fused tail draws the ss_dropout stream
    if B == 7:
        L.call("ss_tail_fwd", h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["pool.score.bias"].data_ptr(),
               P["head.0.weight"].data_ptr(), P["head.0.bias"].data_ptr(), P["head.1.weight"].data_ptr(),
               P["head.1.bias"].data_ptr(), P["head.4.weight"].data_ptr(), P["head.4.bias"].data_ptr(), None, B, T, D, MID,
               C, 1e-5, 0.2, 5, 7 << 40, 0.0, 1.0, attn.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), ln.data_ptr(),
               mid.data_ptr(), mid_d.data_ptr(), logits2.data_ptr(), None, None, None, L.stream())
        ref_d = torch.empty_like(mid)
        L.call("ss_dropout", mid.data_ptr(), ref_d.data_ptr(), B * MID, 0.2, 5, 7 << 40, None, L.stream())
        sync()
        assert torch.equal(ref_d, mid_d) and not torch.equal(mid, mid_d)


@pytest.mark.parametrize("B,C", [(8, 5), (300, 10), (3, 100)])
def test_ce_label_smoothing(L, B, C):
    g = torch.Generator().manual_seed(B + C)
    logits = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    lg = logits.clone().requires_grad_(True)
    loss_ref = F.cross_entropy(lg, y, label_smoothing=0.05)
    loss_ref.backward()
    d = torch.empty(B, C, device="cuda")
    loss = torch.zeros(1, device="cuda")
    correct = torch.zeros(1, device="cuda", dtype=torch.int32)
    L.call("ss_ce_ls_fwd_bwd", dev(logits).data_ptr(), dev(y).data_ptr(), B, C, 0.05, float(B), d.data_ptr(),
           loss.data_ptr(), correct.data_ptr(), L.stream())
    sync()
    assert abs(float(loss) - float(loss_ref)) < 2e-6 * max(1.0, abs(float(loss_ref)))
    assert_close("d logits", d, lg.grad, atol=1e-7, rtol=1e-5)
    assert int(correct) == int((logits.argmax(1) == y).sum())


def test_sumsq_adam_clip(L):
    n = 100003
    g = torch.Generator().manual_seed(8)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    m, v = torch.zeros(n), torch.zeros(n)
    p_d, g_d, m_d, v_d = dev(p), dev(gr), dev(m), dev(v)
    ss = torch.zeros(1, device="cuda")
    pr = p.clone()
    for step in (1, 2, 3):
        ss.zero_()
        L.call("ss_sumsq_f32", g_d.data_ptr(), n, ss.data_ptr(), L.stream())
        L.call("ss_adam_clip", p_d.data_ptr(), g_d.data_ptr(), m_d.data_ptr(), v_d.data_ptr(), n, ss.data_ptr(), 1.0, 1.0,
               3e-4, 0.9, 0.999, 1e-8, step, L.stream())
        sync()
        total = float(gr.double().norm())
        assert abs(float(ss.sqrt()) - total) < 1e-5 * total
        MR.adam_step(pr, gr * MR.clip_coef(total, 1.0), m, v, step)
        assert_close(f"adam p step {step}", p_d, pr, atol=2e-7, rtol=1e-6)
    # grad_scale (mean over ranks after a summing all-reduce)
    p2, m2, v2 = dev(p), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    g4 = dev(gr * 4)
    ss.zero_()
    L.call("ss_sumsq_f32", g4.data_ptr(), n, ss.data_ptr(), L.stream())
    L.call("ss_adam_clip", p2.data_ptr(), g4.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, ss.data_ptr(), 0.25, 1.0, 3e-4,
           0.9, 0.999, 1e-8, 1, L.stream())
    p3, m3, v3 = dev(p), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ss.zero_()
    L.call("ss_sumsq_f32", g_d.data_ptr(), n, ss.data_ptr(), L.stream())
    L.call("ss_adam_clip", p3.data_ptr(), g_d.data_ptr(), m3.data_ptr(), v3.data_ptr(), n, ss.data_ptr(), 1.0, 1.0, 3e-4,
           0.9, 0.999, 1e-8, 1, L.stream())
    sync()
    assert_close("grad_scale", p2, p3, atol=1e-7, rtol=1e-6)


def test_dropout_mask_is_reproducible_and_unbiased(L):
    n = 1 << 20
    x = torch.ones(n, device="cuda")
    y1, y2, y3 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    L.call("ss_dropout", x.data_ptr(), y1.data_ptr(), n, 0.2, 11, 5 << 40, None, L.stream())
    L.call("ss_dropout", x.data_ptr(), y2.data_ptr(), n, 0.2, 11, 5 << 40, None, L.stream())
    L.call("ss_dropout", x.data_ptr(), y3.data_ptr(), n, 0.2, 12, 5 << 40, None, L.stream())
    sync()
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    keep = float((y1 > 0).float().mean())
    assert abs(keep - 0.8) < 3e-3
    assert abs(float(y1.mean()) - 1.0) < 5e-3
    assert set(torch.unique(y1).tolist()) == {0.0, 1.25}
    # ... and it is the stream of an independent Philox4x32-10 (tests/flat_ref.py): every fused consumer above is compared
    # with ss_dropout, this ties ss_dropout to the published generator
    import flat_ref as FR

    keep, want, bound = FR.dropout_expected(np.ones(n, np.float32), n, 0.2, 11, 5 << 40)
    assert np.array_equal(y1.cpu().numpy() != 0, keep) and (np.abs(y1.cpu().numpy().astype(np.float64) - want) <= bound).all()


# ------------------------------------------------------------------------------------- ROI CNN
def _cnn_sd(seed):
    import weights as W

    sd = W.make_state_dict(seed, 84, 5, True)
    return {k: v for k, v in sd.items() if k.startswith("roi_cnn.")}


CNN_KEYS = ("roi_cnn.net.0.weight", "roi_cnn.net.0.bias", "roi_cnn.net.3.weight", "roi_cnn.net.3.bias",
            "roi_cnn.net.6.weight", "roi_cnn.net.6.bias", "roi_cnn.fc.weight", "roi_cnn.fc.bias")


def _cnn_frames(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    R = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8)
    ramp = (torch.arange(W).view(1, 1, W) * 255 // (W - 1)).to(torch.int32)
    R = ((R.to(torch.int32) + ramp) // 2).to(torch.uint8)
    R[0] = 0
    # a constant non-zero frame normalises to exactly 0 here; torch's float mean of 1024 equal values is one ulp off and
    # the 1e-6 clamp turns that ulp into 0.06, so that frame is only compared at the sizes where torch is exact too
    if N > 1 and H * W != 1024:
        R[1] = 200
    if N > 2:
        R[2] = 17
        R[2, 3, 5] = 18
    return R


@pytest.mark.parametrize("H,W", [(64, 64), (48, 96), (32, 32)])
@pytest.mark.parametrize("standardize", [1, 0])
def test_roi_cnn_fwd(L, H, W, standardize):
    N = 300 if (H, W) == (64, 64) else 19  # 300 > 256 workgroups: exercises the persistent frame walk
    sd = _cnn_sd(21)
    R = _cnn_frames(N, H, W, 2)
    ref = MR.roi_cnn(MR.roi_normalise(R.unsqueeze(0), bool(standardize)), sd)[0]
    P = [dev(sd[k]) for k in CNN_KEYS]
    ld = 40
    out = torch.full((N, ld), -3.0, device="cuda")
    L.call("ss_roi_cnn_fwd", dev(R).data_ptr(), N, H, W, standardize, *[p.data_ptr() for p in P], 32,
           out.data_ptr() + 8 * 4, ld, L.stream())
    sync()
    assert_close("roi_e", out[:, 8:], ref, atol=2e-5, rtol=1e-4)
    assert torch.all(out[:, :8] == -3.0)


@pytest.mark.parametrize("B,T", [(7, 12), (300, 5), (1, 1), (4096, 3)])
def test_active_frames_list_and_cleared_rows(L, B, T):
    """ss_roi_active_frames: rows b*T + t with t < min(max(len, 0), T), ascending, their count in front; the embedding columns of
    every other row cleared, nothing else touched (reference: pack_padded_sequence drops those rows, train_model_official.py:300)."""
    g = torch.Generator().manual_seed(B * 31 + T)
    lengths = torch.randint(-1, T + 3, (B,), generator=g, dtype=torch.int32)  # incl. 0, negative and longer than T
    lengths[0] = T
    _check_active_frames(L, B, T, lengths)


# the trailing T - max(len) time columns are dropped for every clip
FRAMES_PADDED = [(7, 12, [4, 1, 5, 9, 2, 7, 11]), (300, 5, [1] * 300), (4, 90, [53, 17, 1, 34]),
                 (256, 90, [1 + (7 * b) % 89 for b in range(256)])]


@pytest.mark.parametrize("B,T,lengths", FRAMES_PADDED, ids=[f"B{b}-T{t}-max{max(n)}" for b, t, n in FRAMES_PADDED])
def test_active_frames_padded_past_the_longest_clip(L, B, T, lengths):
    assert max(lengths) < T
    _check_active_frames(L, B, T, torch.tensor(lengths, dtype=torch.int32))


def _check_active_frames(L, B, T, lengths):
    want = [b * T + t for b in range(B) for t in range(min(max(int(lengths[b]), 0), T))]
    ld, x_dim, E = 13, 5, 6
    Z = torch.full((B * T, ld), 7.0, device="cuda")
    frames = torch.full((1 + B * T,), -5, device="cuda", dtype=torch.int32)
    L.call("ss_roi_active_frames", dev(lengths).data_ptr(), B, T, frames.data_ptr(), Z.data_ptr() + 4 * x_dim, ld, E, L.stream())
    sync()
    got = frames.cpu().tolist()
    assert got[0] == len(want) and got[1:1 + len(want)] == want
    assert all(v == -5 for v in got[1 + len(want):]), "entries behind the list are not the kernel's to write"
    keep = torch.zeros(B * T, dtype=torch.bool)
    keep[torch.tensor(want, dtype=torch.long)] = True
    Zc = Z.cpu()
    assert torch.all(Zc[keep] == 7.0)
    assert torch.all(Zc[~keep][:, x_dim:x_dim + E] == 0.0)
    assert torch.all(Zc[~keep][:, :x_dim] == 7.0) and torch.all(Zc[~keep][:, x_dim + E:] == 7.0)
    # the list alone (no embedding matrix to clear)
    frames2 = torch.zeros_like(frames)
    L.call("ss_roi_active_frames", dev(lengths).data_ptr(), B, T, frames2.data_ptr(), None, 0, 0, L.stream())
    sync()
    assert frames2.cpu().tolist()[:1 + len(want)] == got[:1 + len(want)]


@pytest.mark.parametrize("H,W", [(64, 64), (48, 96), (32, 32)])
def test_roi_cnn_listed_frames_equal_the_full_walk(L, H, W):
    """ss_roi_cnn_fwd_frames / _bwd_frames on a list of frames: the listed rows of `out` are bit-equal to the full walk's, the
    others untouched; the gradients are those of the full walk with d_out == 0 on the frames left out (what the padding rows of
    a batch carry); an empty list adds nothing; a capped grid (several frames per workgroup: the prefetch pipeline) agrees."""
    N = 90 if (H, W) == (64, 64) else 23
    sd = _cnn_sd(5)
    R_d = dev(_cnn_frames(N, H, W, 8))
    P = [dev(sd[k]) for k in CNN_KEYS]
    sizes = L.cnn_stash_sizes(H, W)
    n_a1, n_a2, n_i1, n_i2, n_m3, n_feat = sizes
    g = torch.Generator().manual_seed(77)
    pick = torch.rand(N, generator=g) < 0.6
    pick[0], pick[N - 1] = True, False
    listed = torch.nonzero(pick).flatten().to(torch.int32)
    frames = dev(torch.cat([torch.tensor([len(listed)], dtype=torch.int32), listed,
                            torch.full((N - len(listed),), 10 ** 6, dtype=torch.int32)]))  # the tail must not be read
    d_out = torch.randn(N, 32, generator=g)
    d_masked = dev(d_out * pick[:, None])

    def stash():
        return [torch.zeros(N, n_a1, device="cuda"), torch.zeros(N, n_i1, device="cuda", dtype=torch.uint8),
                torch.zeros(N, n_a2, device="cuda"), torch.zeros(N, n_i2, device="cuda", dtype=torch.uint8),
                torch.zeros(N, n_m3, device="cuda", dtype=torch.uint8), torch.zeros(N, n_feat, device="cuda")]

    def run(fr, d, cap=0):
        out = torch.full((N, 32), -3.0, device="cuda")
        st = stash()
        G = [torch.zeros_like(p) for p in P]
        L.call("ss_roi_cnn_set_max_workgroups", cap)
        try:
            L.call("ss_roi_cnn_fwd_frames", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, out.data_ptr(), 32,
                   *[s.data_ptr() for s in st], sizes.ptr, L.ptr(fr), L.stream())
            L.call("ss_roi_cnn_bwd_frames", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, *[s.data_ptr() for s in st],
                   sizes.ptr, d.data_ptr(), 32, *[gg.data_ptr() for gg in G], L.ptr(fr), L.stream())
        finally:
            L.call("ss_roi_cnn_set_max_workgroups", 0)
        sync()
        return out, G

    out_full, G_full = run(None, d_masked)
    for cap in (0, 3):
        out_l, G_l = run(frames, dev(d_out), cap)  # d_out of the frames left out is never read
        assert torch.equal(out_l[pick.cuda()], out_full[pick.cuda()])
        assert torch.all(out_l[~pick.cuda()] == -3.0)
        for k, a, b in zip(CNN_KEYS, G_l, G_full):
            scale = max(float(b.abs().max()), 1e-6)
            assert float((a - b).abs().max()) < 2e-5 * scale, (k, cap, float((a - b).abs().max()), scale)
    empty = dev(torch.zeros(1 + N, dtype=torch.int32))
    out_e, G_e = run(empty, dev(d_out))
    assert torch.all(out_e == -3.0) and all(float(gg.abs().max()) == 0.0 for gg in G_e)


@pytest.mark.parametrize("H,W", [(64, 64), (48, 96), (32, 32)])
def test_roi_cnn_stash_and_bwd(L, H, W):
    N = 270 if (H, W) == (64, 64) else 11
    sd = _cnn_sd(22)
    R = _cnn_frames(N, H, W, 3)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x = MR.roi_normalise(R.unsqueeze(0), True)[0]  # (N,1,H,W)
    c1 = F.relu(F.conv2d(x, leaves[CNN_KEYS[0]], leaves[CNN_KEYS[1]], padding=1))
    a1, i1 = F.max_pool2d(c1, 2, return_indices=True)
    c2 = F.relu(F.conv2d(a1, leaves[CNN_KEYS[2]], leaves[CNN_KEYS[3]], padding=1))
    a2, i2 = F.max_pool2d(c2, 2, return_indices=True)
    c3 = F.relu(F.conv2d(a2, leaves[CNN_KEYS[4]], leaves[CNN_KEYS[5]], padding=1))
    feat = c3.mean((2, 3))
    out_ref = F.linear(feat, leaves[CNN_KEYS[6]], leaves[CNN_KEYS[7]])
    d_out = torch.randn(N, 32, generator=torch.Generator().manual_seed(9))
    (out_ref * d_out).sum().backward()

    P = [dev(sd[k]) for k in CNN_KEYS]
    R_d = dev(R)
    out = torch.empty(N, 32, device="cuda")
    H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
    sizes = L.cnn_stash_sizes(H, W)
    n_a1, n_a2, n_i1, n_i2, n_m3, n_feat = sizes
    assert (n_i2, n_m3) == (H4 * W4 * 16, H4 * W4 * 32) and n_feat >= 50

    def wrong(k, delta):  # the same six sizes with one of them off: what a stale object / a mis-sized caller would hand in
        v = list(sizes)
        v[k] += delta
        return L.StashSizes(v)

    st_a1 = torch.empty(N, n_a1, device="cuda")
    st_i1 = torch.empty(N, n_i1, device="cuda", dtype=torch.uint8)
    st_a2 = torch.empty(N, n_a2, device="cuda")
    st_i2 = torch.empty(N, H4, W4, 16, device="cuda", dtype=torch.uint8)  # pixel-major
    st_m3 = torch.empty(N, H4 * W4, 32, device="cuda", dtype=torch.uint8)  # pixel-major, 24 of 32 channel slots used
    st_feat = torch.empty(N, n_feat, device="cuda")  # 24 features, 24 positive-output counts, frame mean / std, pad
    st = [st_a1, st_i1, st_a2, st_i2, st_m3, st_feat]
    L.call("ss_roi_cnn_fwd_stash", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, out.data_ptr(), 32,
           *[s.data_ptr() for s in st], sizes.ptr, L.stream())
    # a caller whose buffers were sized for another layout is turned away, not written over:
    # the pooled-1 map and the st_feat row width (the one the round-2 ABI did not check)
    for bad in (wrong(0, -8), wrong(5, -4)):
        with pytest.raises(RuntimeError, match="ss_roi_cnn_fwd_stash"):
            L.call("ss_roi_cnn_fwd_stash", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, out.data_ptr(), 32,
                   *[s.data_ptr() for s in st], bad.ptr, L.stream())
    sync()
    assert_close("roi_e", out, out_ref, atol=2e-5, rtol=1e-4)

    def unhalo(st, ch, hh, ww):  # (N, ch*plane) haloed image -> (N, ch, hh, ww); the halo itself must be zero
        img = st.view(N, ch, -1)[:, :, : (hh + 2) * (ww + 2)].reshape(N, ch, hh + 2, ww + 2)
        assert float(img[:, :, 0].abs().max()) == 0 and float(img[:, :, :, 0].abs().max()) == 0
        assert float(img[:, :, -1].abs().max()) == 0 and float(img[:, :, :, -1].abs().max()) == 0
        return img[:, :, 1:-1, 1:-1]

    assert_close("stash a1", unhalo(st_a1, 8, H2, W2), a1, atol=1e-5, rtol=1e-5)
    assert_close("stash a2", unhalo(st_a2, 16, H4, W4), a2, atol=2e-5, rtol=1e-5)
    assert_close("stash feat", st_feat[:, :24], feat, atol=1e-5, rtol=1e-5)

    # argmax: compare where the winner is positive and clearly separated (ties / relu zeros carry no gradient)
    def idx_to_win(idx, w_in):  # flat index in the (2h x 2w) plane -> 0..3 inside its window
        yy, xx = idx // w_in, idx % w_in
        return ((yy % 2) * 2 + (xx % 2)).to(torch.uint8)

    def top2_gap(c):  # gap between the best and second best of every 2x2 window
        n_, ch, hh, ww = c.shape
        win = c.reshape(n_, ch, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n_, ch, hh // 2, ww // 2, 4)
        top = win.topk(2, dim=-1).values
        return top[..., 0] - top[..., 1]

    st_i1v = st_i1.view(N, 8, -1)[:, :, : H2 * W2].reshape(N, 8, H2, W2)  # planes are padded by 4 bytes
    for name, st_i, idx, c, a in (("i1", st_i1v, i1, c1, a1), ("i2", st_i2.permute(0, 3, 1, 2), i2, c2, a2)):
        sure = (a > 1e-4) & (top2_gap(c.detach()) > 1e-4)
        got = st_i.cpu()[sure]
        want = idx_to_win(idx, c.shape[3])[sure]
        assert torch.equal(got, want), f"{name}: {(got != want).sum()} argmax mismatches of {sure.sum()}"
    m3_ref = (c3.detach() > 0).reshape(N, 24, -1)
    sure3 = (c3.detach().abs() > 1e-4).reshape(N, 24, -1)
    assert torch.equal(st_m3.cpu()[:, :, :24].permute(0, 2, 1).bool()[sure3], m3_ref[sure3])
    assert int(st_m3[:, :, 24:].sum()) == 0

    G = [torch.zeros_like(p) for p in P]
    for bad in (wrong(2, 32), wrong(5, 4), wrong(4, -32)):
        with pytest.raises(RuntimeError, match="ss_roi_cnn_bwd"):
            L.call("ss_roi_cnn_bwd", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, *[s.data_ptr() for s in st],
                   bad.ptr, dev(d_out).data_ptr(), 32, *[gg.data_ptr() for gg in G], L.stream())
    L.call("ss_roi_cnn_bwd", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, *[s.data_ptr() for s in st],
           sizes.ptr, dev(d_out).data_ptr(), 32, *[gg.data_ptr() for gg in G], L.stream())
    sync()
    for k, gg in zip(CNN_KEYS, G):
        ref = leaves[k].grad
        scale = float(ref.abs().max())
        assert_close("grad " + k, gg, ref, atol=3e-4 * max(scale, 1e-3), rtol=1e-3)
    # gradients accumulate: a second call doubles them
    L.call("ss_roi_cnn_bwd", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, *[s.data_ptr() for s in st],
           sizes.ptr, dev(d_out).data_ptr(), 32, *[gg.data_ptr() for gg in G], L.stream())
    sync()
    assert_close("accumulate", G[4], 2 * leaves[CNN_KEYS[4]].grad, atol=6e-4 * float(leaves[CNN_KEYS[4]].grad.abs().max()),
                 rtol=1e-3)

    # The frame PIPELINE (prefetch one frame ahead, the next frame's front inside the current frame's last stage) only
    # runs when a workgroup walks several frames: cap the grid so that every workgroup takes 4+ frames, check the same
    # references, then repeat the launch: identical launches may differ by the order of the float atomics only
    # (a missing barrier once made d W1 move by 4e-2 between launches while every single-frame test passed).
    cap = 16 if N > 100 else 3
    L.call("ss_roi_cnn_set_max_workgroups", cap)
    try:
        out2 = torch.empty_like(out)
        L.call("ss_roi_cnn_fwd_stash", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, out2.data_ptr(), 32,
               *[s.data_ptr() for s in st], sizes.ptr, L.stream())
        sync()
        assert torch.equal(out2, out), "the forward output of a frame must not depend on which workgroup computes it"
        runs = []
        for _ in range(8):
            G2 = [torch.zeros_like(p) for p in P]
            L.call("ss_roi_cnn_bwd", R_d.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], 32, *[s.data_ptr() for s in st],
                   sizes.ptr, dev(d_out).data_ptr(), 32, *[gg.data_ptr() for gg in G2], L.stream())
            sync()
            runs.append(G2)
        for k, gg in zip(CNN_KEYS, runs[0]):
            ref = leaves[k].grad
            assert_close("walked grad " + k, gg, ref, atol=3e-4 * max(float(ref.abs().max()), 1e-3), rtol=1e-3)
        for r in runs[1:]:
            for k, g0, g1 in zip(CNN_KEYS, runs[0], r):
                spread = float((g1 - g0).abs().max()) / max(float(g0.abs().max()), 1e-30)
                assert spread < 2e-5, f"{k}: identical launches differ by {spread:.1e} of the largest entry"
    finally:
        L.call("ss_roi_cnn_set_max_workgroups", 0)


# ------------------------------------------------------------------------------------- features / crop
def _anchors(idxs):
    idxs = [int(v) for v in idxs]
    return idxs.index(61), idxs.index(291), idxs.index(13), idxs.index(14)


@pytest.mark.parametrize("tag", ["88", "40"])
@pytest.mark.parametrize("variant", [0, 1])
def test_feature_fuse_vs_golden(L, golden_dir, tag, variant):
    d = np.load(os.path.join(golden_dir, "features.npz"))
    idxs = d["idx" + tag]
    lm = torch.from_numpy(d["lm"][:, idxs]).unsqueeze(0)  # (1,T,K,2)
    T, K = lm.shape[1], lm.shape[2]
    reset = torch.from_numpy(d["reset"].astype(np.uint8)).unsqueeze(0)
    X = torch.zeros(1, T, 2 * K + 4, device="cuda")
    cen = torch.zeros(1, T, 2, device="cuda")
    fourth = torch.zeros(1, T, device="cuda", dtype=torch.float64)
    L.call("ss_feature_fuse", dev(lm).data_ptr(), dev(reset).data_ptr(), 1, T, K, int(d["w"]), int(d["h"]), *_anchors(idxs),
           variant, X.data_ptr(), 2 * K + 4, cen.data_ptr(), fourth.data_ptr(), L.stream())
    sync()
    vname = "record" if variant == 0 else "live"
    ref = d[f"feat_{vname}_{tag}"]
    if not np.array_equal(cen[0].cpu().numpy(), d[f"center_{vname}_{tag}"]):
        pytest.fail("centre must be bit-exact: max diff %g" % np.abs(cen[0].cpu().numpy() - d[f"center_{vname}_{tag}"]).max(),
                    pytrace=False)
    np.testing.assert_allclose(fourth[0].cpu().numpy(), d[f"fourth_{vname}_{tag}"], rtol=1e-15)
    got = X[0].cpu().numpy()
    np.testing.assert_allclose(got[:, : 2 * K], ref[:, : 2 * K], rtol=0, atol=1.2e-7)
    np.testing.assert_allclose(got[:, 2 * K:], ref[:, 2 * K:], rtol=1e-6, atol=1e-7)
    assert np.all(got[d["reset"], 2 * K] == 0.0)


def test_feature_fuse_batched_vs_oracle(L):
    B, T, K, w, h = 33, 30, 40, 640, 480
    rng = np.random.default_rng(0)
    lm = (rng.uniform(0.3, 0.7, (B, 1, K, 2)) + rng.normal(0, 0.004, (B, T, K, 2))).astype(np.float32)
    lm[:, :, 8] = [0.42, 0.61]; lm[:, :, 25] = [0.58, 0.61]; lm[:, :, 1] = [0.5, 0.59]; lm[:, :, 2] = [0.5, 0.63]
    lm += rng.normal(0, 0.002, lm.shape).astype(np.float32)
    X = torch.zeros(B, T, 2 * K + 4, device="cuda")
    cen = torch.zeros(B, T, 2, device="cuda")
    fourth = torch.zeros(B, T, device="cuda", dtype=torch.float64)
    L.call("ss_feature_fuse", dev(torch.from_numpy(lm)).data_ptr(), None, B, T, K, w, h, 8, 25, 1, 2, 0, X.data_ptr(),
           2 * K + 4, cen.data_ptr(), fourth.data_ptr(), L.stream())
    sync()
    for b in (0, 7, 32):
        Xr, cr, fr = FR.extract_clip(lm[b], w, h, (8, 25, 1, 2), None, "record")
        assert np.array_equal(cen[b].cpu().numpy(), cr)
        np.testing.assert_allclose(fourth[b].cpu().numpy(), fr, rtol=1e-15)
        np.testing.assert_allclose(X[b].cpu().numpy(), Xr, rtol=1e-6, atol=1.2e-7)


def test_crop_idx_bit_exact(L, golden_dir):
    d = np.load(os.path.join(golden_dir, "crop.npz"))
    checked = 0
    for (w, h) in {tuple(v) for v in d["wh"].tolist()}:
        for variant in (0, 1):
            sel = (d["wh"][:, 0] == w) & (d["wh"][:, 1] == h) & (d["variant"] == variant)
            n = int(sel.sum())
            box = torch.zeros(n, 5, device="cuda", dtype=torch.int32)
            L.call("ss_roi_crop_idx", dev(torch.from_numpy(d["center"][sel])).data_ptr(),
                   dev(torch.from_numpy(d["scale"][sel])).data_ptr(), n, int(w), int(h), variant, box.data_ptr(),
                   L.stream())
            sync()
            got = box.cpu().numpy()
            assert np.array_equal(got[:, 4], d["valid"][sel])
            ok = d["valid"][sel] == 1
            assert np.array_equal(got[ok][:, :4], d["box"][sel][ok])
            checked += int(ok.sum())
    assert checked > 2000
    # random sweep against the oracle (which the golden file pins), including invalid boxes' coordinates
    rng = np.random.default_rng(1)
    n = 20000
    cen = rng.uniform(-50, 700, (n, 2)).astype(np.float32)
    sc = rng.uniform(0, 200, n)
    for variant in (0, 1):
        box = torch.zeros(n, 5, device="cuda", dtype=torch.int32)
        L.call("ss_roi_crop_idx", dev(torch.from_numpy(cen)).data_ptr(), dev(torch.from_numpy(sc)).data_ptr(), n, 640, 480,
               variant, box.data_ptr(), L.stream())
        sync()
        got = box.cpu().numpy()
        ref = np.array([FR.crop_box(cen[k], sc[k], 640, 480, "record" if variant == 0 else "live") for k in range(n)])
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------- batch assembly
def test_device_clip_store_matches_reference_batches(L, tmp_path):
    """Clips resident in HBM + two gather launches == the reference's NPZWordDataset(augment=True) + collate_fn,
    bit for bit, when the host makes the reference's random draws (tests/golden/dataset.npz)."""
    import random

    from test_host_formats import _golden_clips
    import silent_speech_amd as ss

    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d, files = _golden_clips(str(tmp_path), golden_dir)
    store = ss.DeviceClipStore(files, {"no": 0, "yes": 1}, max_t=int(d["max_t"]))
    for b in range(int(d["n_batches"])):
        random.seed(1000 + b)
        np.random.seed(2000 + b)
        X, T, R, y = store.batch(d[f"batch{b}::order"].tolist(), augment=True, rng="reference")
        sync()
        assert np.array_equal(X.cpu().numpy(), d[f"batch{b}::X"]) and np.array_equal(T.cpu().numpy(), d[f"batch{b}::T"])
        assert np.array_equal(R.cpu().numpy(), d[f"batch{b}::R"]) and np.array_equal(y.cpu().numpy(), d[f"batch{b}::y"])
    X, T, R, y = store.batch(range(len(store)), augment=False)
    sync()
    assert np.array_equal(X.cpu().numpy(), d["plain::X"]) and np.array_equal(R.cpu().numpy(), d["plain::R"])
    assert np.array_equal(T.cpu().numpy(), d["plain::T"]) and np.array_equal(y.cpu().numpy(), d["plain::y"])
    # device-side randomness: same rules, different stream -- lengths within the drop range, ROI untouched, the noise
    # has the reference's scale, padding stays exactly zero
    gen = np.random.default_rng(3)
    seen_noise, seen_drop = [], 0
    for _ in range(30):
        X, T, R, y = store.batch(range(len(store)), augment=True, rng="device", generator=gen)
        sync()
        Xc, Tc = X.cpu().numpy(), T.cpu().numpy()
        plain_T = d["plain::T"]
        assert np.all(Tc <= plain_T) and np.all(Tc >= plain_T - 2)  # at most two interior frames dropped
        assert np.array_equal(R.cpu().numpy()[:, :1], d["plain::R"][:, :1])
        for bb in range(len(store)):
            assert not Xc[bb, Tc[bb]:].any()
            if Tc[bb] == plain_T[bb] and len(d[f"clip{bb}::X"]) <= int(d["max_t"]):
                diff = Xc[bb, :Tc[bb]] - d["plain::X"][bb, :Tc[bb]]
                if np.abs(diff).max() > 0 and np.abs(diff).max() < 0.1:  # noised, nothing dropped
                    seen_noise.append(diff.std())
            seen_drop += int(Tc[bb] < plain_T[bb])
    assert seen_noise and abs(np.mean(seen_noise) - 0.01) < 0.002, seen_noise[:5]
    assert seen_drop > 0


# ------------------------------------------------------------------------------------- crop + gray + resize
@pytest.mark.parametrize("variant", ["record", "live"])
def test_crop_gray_resize_equals_restatement(L, variant):
    """ss_crop_gray_resize == oracle/resize_ref.py bit for bit (the restatement of OpenCV's algorithms; parity with
    OpenCV itself is unpinned): reduced, enlarged, integer-scale and invalid boxes, both interpolations."""
    from oracle import resize_ref as RR
    import silent_speech_amd as ss

    rng = np.random.default_rng(7)
    h, w, RH, RW = 240, 320, 48, 96
    boxes = np.asarray([[40, 286, 30, 235, 1],     # 246 x 205 -> reduced, fractional scales
                        [100, 160, 90, 115, 1],    # 60 x 25   -> enlarged
                        [10, 202, 20, 116, 1],     # 192 x 96  -> integer 2 x 2
                        [0, 288, 0, 192, 1],       # 288 x 192 -> integer 3 x 4
                        [50, 50, 60, 90, 0],       # invalid
                        [300, 320, 200, 240, 1]],  # at the frame's corner, mixed: x enlarged, y reduced
                       np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.stack([np.clip(np.stack([127 + 90 * np.sin(xx / (9.0 + k) + c) * np.cos(yy / 13.0) for c in range(3)], -1)
                               + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8) for k in range(len(boxes))])
    out = ss.crop_rois(dev(torch.from_numpy(frames)), dev(torch.from_numpy(boxes)), (RH, RW), variant)
    sync()
    interp = "linear" if variant == "record" else "area"
    for k, b in enumerate(boxes):
        want = RR.crop_gray_resize(frames[k], b, RH, RW, interp)
        got = out[k].cpu().numpy()
        assert np.array_equal(got, want), f"box {k}: {np.abs(got.astype(int) - want).max()} grey levels off, {(got != want).sum()} pixels"
