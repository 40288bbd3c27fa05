"""GPU: ss_gru_dx_f32, the d layer_in product of a GRU layer -- C[M][N] = A0[M][K] B0[K][N] + A1[M][K] B1[K][N], both directions as
one contraction, plain stores -- against float64 NumPy written from that formula, and the f32 engine's backward pass that uses it.

Every operand and C live in a flat buffer of NaN: the elements of the operands are the only finite values, so a read outside
them poisons the result, and the NaN around C[0..M)[0..N) must survive the call.  The 64 x 192 form serves N > 32, the 32 x 32
form N <= 32; operands that are 16-byte aligned throughout (and N a multiple of 4) go through the LDS-DMA ring, the others
through registers -- the cases below reach all four.
"""

import numpy as np
import pytest
import torch

import weights as W  # noqa: E402
from gemm_ref import assert_exact_range, f32_bound, int_operands
from oracle import model_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 64        # floats of NaN in front of and behind every buffer (a multiple of 4: the operands stay 16-byte aligned)
GAP = 8         # floats of NaN between the (A0, A1) and the (B0, B1) of a case
TILE_M = {True: 32, False: 64}  # rows of an output tile: the 32-column form, the 192-column form
TILE_N = 192
RING_K = 64     # k rows the ring of four 16-wide tiles holds


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from silent_speech_amd import _lib

    return _lib.load()


def rows_of(N):
    t = TILE_M[N <= 32]
    return (1, t - 1, t, t + 1, 2 * t + 3)


class Case:
    """Flat NaN buffers around the operands of one call; ``shift`` floats move A and B off their 16-byte alignment."""

    def __init__(self, M, N, K, pairs, lda=None, ldb=None, ldc=None, col0=0, shift=0):
        self.M, self.N, self.K, self.col0 = M, N, K, col0
        self.lda = lda if lda is not None else K + 4
        self.ldb = ldb if ldb is not None else col0 + N + (4 - N % 4) % 4 + 4
        self.ldc = ldc if ldc is not None else N + (4 - N % 4) % 4 + 4
        self.sa, self.sb = M * self.lda + GAP, K * self.ldb + GAP
        self.a0, self.b0 = PAD + shift, PAD + shift
        a = np.full(2 * PAD + 2 * self.sa, np.nan, dtype=np.float32)
        b = np.full(2 * PAD + 2 * self.sb, np.nan, dtype=np.float32)
        self.ia = self.a0 + np.arange(M)[:, None] * self.lda + np.arange(K)[None, :]
        self.ib = self.b0 + np.arange(K)[:, None] * self.ldb + col0 + np.arange(N)[None, :]
        for d, (A, B) in enumerate(pairs):
            a[self.ia + d * self.sa] = A
            b[self.ib + d * self.sb] = B
        self.pairs = pairs
        self.a, self.b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        self.c = torch.full((2 * PAD + M * self.ldc,), float("nan"), dtype=torch.float32, device="cuda")
        self.ic = torch.from_numpy(PAD + np.arange(M)[:, None] * self.ldc + np.arange(N)[None, :]).cuda()

    def run(self, lib):
        self.c.fill_(float("nan"))
        st = lib.ss_gru_dx_f32(self.M, self.N, self.K, self.a.data_ptr() + 4 * self.a0, self.lda, self.sa,
                               self.b.data_ptr() + 4 * self.b0, self.ldb, self.col0, self.sb, self.c.data_ptr() + 4 * PAD, self.ldc,
                               torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        torch.cuda.synchronize()
        out = self.c[self.ic]
        mask = torch.ones_like(self.c, dtype=torch.bool)
        mask[self.ic.reshape(-1)] = False
        assert torch.isnan(self.c[mask]).all(), "something outside C[0..M)[0..N) was written"
        return out

    def reference(self):
        return sum(np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64) for A, B in self.pairs)


def int_pairs(M, N, K, seed, zero=None):
    pairs = [(int_operands((M, K), seed + 2 * d), int_operands((K, N), seed + 2 * d + 1)) for d in range(2)]
    if zero is not None:
        pairs[zero] = (np.zeros((M, K), np.float32), np.zeros((K, N), np.float32))
    assert_exact_range(pairs)
    return pairs


def check_exact(lib, case):
    got = case.run(lib)
    want = torch.from_numpy(case.reference().astype(np.float32)).cuda()
    assert torch.equal(got, want), (f"M={case.M} N={case.N} K={case.K}: {int((got != want).sum())} elements differ, "
                                    f"max {float((got - want).abs().max())}")


@pytest.mark.parametrize("N", [1, 31, 32, 33, TILE_N - 1, TILE_N + 1, 384])
def test_exact_at_the_tile_edges(lib, N):
    """Integer operands, every partial sum below 2**24: bit equality with the float64 product, at every edge of both tile forms.
    K = 16 and 48 are shorter than the ring, 100 ends in a ragged k tile (so each direction runs its own loop), 576 is the GRU's."""
    assert 48 < RING_K
    for M in rows_of(N):
        for K in (16, 48, 100, 576):
            check_exact(lib, Case(M, N, K, int_pairs(M, N, K, seed=1000 * N + 10 * M + K)))


@pytest.mark.parametrize("N,M", [(32, 67), (384, 131), (116, 65)])
@pytest.mark.parametrize("zero", [0, 1])
def test_each_half_of_the_loop_reads_its_own_pair(lib, N, M, zero):
    """With one (A, B) pair all zeros the result is the other pair's product alone."""
    for K in (48, 100, 576):
        case = Case(M, N, K, int_pairs(M, N, K, seed=7 + zero, zero=zero))
        check_exact(lib, case)
        assert float(np.abs(case.reference()).max()) > 0


@pytest.mark.parametrize("N,M,K,kw", [
    (32, 67, 576, dict(col0=84, ldb=116, ldc=116)),    # layer 0's call: the ROI-embedding columns of W_ih into those of d Z
    (116, 65, 576, dict(col0=0, ldb=116, ldc=116)),    # ... with d X asked for: all in_dim columns
    (384, 131, 576, dict(lda=768, ldb=384, ldc=384)),  # layer 1's call: ldc == N
    (32, 33, 100, dict(col0=5)),                       # a column offset that breaks B's alignment: through registers
    (28, 40, 80, dict(ldc=33)),                        # a leading dimension of C that rules out 16-byte stores
    (192, 70, 64, dict(lda=67)),                       # lda no multiple of 4
    (64, 64, 96, dict(shift=1)),                       # A and B one float off their alignment
    (4, 5, 16, dict()),                                # the smallest N the DMA form takes
])
def test_exact_with_offsets_and_leading_dimensions(lib, N, M, K, kw):
    check_exact(lib, Case(M, N, K, int_pairs(M, N, K, seed=N + M + K), **kw))


FLOAT_SHAPES = [(131, 384), (67, 32), (65, 116), (33, 31)]


def float_case(M, N, K=576, seed=3):
    rng = np.random.default_rng(seed)
    pairs = [(rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)) for _ in range(2)]
    return Case(M, N, K, pairs, lda=768 if N != 31 else None)


@pytest.mark.parametrize("M,N", FLOAT_SHAPES)
def test_float_operands_within_the_f32_bound(lib, M, N):
    case = float_case(M, N)
    got = case.run(lib).cpu().numpy().astype(np.float64)
    absA = np.concatenate([np.abs(A) for A, _ in case.pairs], axis=1)
    absB = np.concatenate([np.abs(B) for _, B in case.pairs], axis=0)
    bound = f32_bound(absA, absB, 2 * case.K)
    err = np.abs(got - case.reference())
    print(f"M={M} N={N}: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())


def test_the_same_operands_give_the_same_bits(lib):
    case = float_case(131, 384)
    first = case.run(lib).clone()
    assert torch.equal(case.run(lib), first)
    narrow = float_case(67, 32)
    first = narrow.run(lib).clone()
    assert torch.equal(narrow.run(lib), first)


def test_bad_arguments_are_refused(lib):
    c = Case(8, 8, 16, int_pairs(8, 8, 16, seed=1))
    a, b, cc, s = c.a.data_ptr() + 4 * c.a0, c.b.data_ptr() + 4 * c.b0, c.c.data_ptr() + 4 * PAD, torch.cuda.current_stream().cuda_stream
    good = dict(M=8, N=8, K=16, A=a, lda=c.lda, sa=c.sa, B=b, ldb=c.ldb, col0=0, sb=c.sb, C=cc, ldc=c.ldc)
    for bad in (dict(M=0), dict(N=0), dict(K=0), dict(A=None), dict(B=None), dict(C=None), dict(lda=15), dict(ldb=7), dict(col0=-1),
                dict(col0=c.ldb - 7), dict(ldc=7)):
        q = {**good, **bad}
        st = lib.ss_gru_dx_f32(q["M"], q["N"], q["K"], q["A"], q["lda"], q["sa"], q["B"], q["ldb"], q["col0"], q["sb"], q["C"], q["ldc"], s)
        assert st == -1, (bad, st)
    torch.cuda.synchronize()
    assert torch.isnan(c.c).all()


# ---------------------------------------------------------------------------------------------------------------- engine level
def train_workspace(m):
    (ws,) = [w for w in m._ws_cache.values() if w.train]
    assert ws.dx_one_launch  # the form under test
    return ws


@pytest.fixture
def one_launch(monkeypatch):
    """The engine takes ss_gru_dx_f32 for batches whose tiles fill most of the chip (engine.DX_ONE_LAUNCH_MIN_FILL); the shapes
    below are a handful of tiles, so the tests lower the bar to nothing: every training workspace built meanwhile uses it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from silent_speech_amd import engine as E

    monkeypatch.setattr(E, "DX_ONE_LAUNCH_MIN_FILL", 0.0)
    return E


def test_which_batches_take_the_one_launch_form():
    """The rule, at the shapes it was measured at on the 256-CU chip: config 2 and the shipped shape at B = 256 do, B = 16 does not."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from silent_speech_amd import engine as E

    cfg = E.Config(x_dim=84, num_classes=5, use_roi=True)
    cus = torch.cuda.get_device_properties("cuda").multi_processor_count
    for rows in (256 * 30, 256 * 90, 16 * 90, 24):
        assert E.dx_one_launch(cfg, rows, "cuda") == (-(-rows // 64) * 2 >= 0.8 * cus), rows
    if cus == 256:
        assert [E.dx_one_launch(cfg, rows, "cuda") for rows in (256 * 30, 256 * 90, 16 * 90, 24)] == [True, True, False, False]


@pytest.mark.parametrize("B,T", [(3, 5), (17, 4)])
def test_backward_matches_the_oracle_and_leaves_nothing_stale(one_launch, B, T):
    """H = 192, 64 x 64 ROI: parameter gradients against oracle/model_ref.py within the bounds tests/test_gpu_model.py holds them
    to; then the same backward once more on the same workspace, its d layer_in destinations filled with NaN in between -- they
    are not cleared any more, so every element the pass reads must be one it has written: bit-equal to the first call."""
    import silent_speech_amd as ss

    E = one_launch
    sd = W.make_state_dict(13, 84, 5, True)
    X, Lh, R, y = W.make_inputs(13, B, T, 84, 5, (64, 64))
    m = ss.BiGRUClassifier(84, 5, use_roi=True)
    m.load_state_dict(sd)
    m.cuda().eval()
    Xc, Rc = X.cuda(), R.cuda()
    logits = m(Xc, Lh.cuda(), Rc)
    logits.retain_grad()
    loss = torch.nn.functional.cross_entropy(logits, y.cuda(), label_smoothing=0.05)
    loss.backward()
    _, _, grads = MR.loss_and_grads(sd, X, Lh, R, y)
    for k, p in m.named_parameters():
        ref, got = grads[k], p.grad.cpu()
        if k == "pool.score.bias":  # exactly 0 in exact arithmetic: rounding noise on both sides (tests/test_gpu_model.py)
            assert float(got.abs().max()) < 1e-6 and float(ref.abs().max()) < 1e-6
            continue
        scale = max(float(ref.abs().max()), 1e-4)
        bad = (got - ref).abs() > 2e-4 * scale + 2e-3 * ref.abs()
        assert not bad.any(), f"{k}: max err {float((got - ref).abs().max()):.3e} vs scale {scale:.3e}"
    ws = train_workspace(m)
    x_dim = m.cfg.x_dim
    first = ws.d_lower[1].clone(), ws.dZ[:, x_dim:].clone()
    assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all()
    ws.d_lower[1].fill_(float("nan"))
    ws.dZ.fill_(float("nan"))
    G = m._views_of(torch.zeros_like(m.flat_params))
    E.backward(m._param_dict(), G, m.cfg, ws, Xc, Rc, logits.grad.contiguous(), train=False, seed=0)
    torch.cuda.synchronize()
    assert torch.equal(ws.d_lower[1], first[0])
    assert torch.equal(ws.dZ[:, x_dim:], first[1])
    assert torch.isnan(ws.dZ[:, :x_dim]).all()  # nobody asked for d X: those columns are neither written nor read
    assert all(torch.isfinite(g).all() for g in G.values())
    for k, p in m.named_parameters():  # the second pass computed the same gradients (sums in another order)
        scale = max(float(p.grad.abs().max()), 1e-4)
        assert float((G[k] - p.grad).abs().max()) <= 2e-4 * scale, k


@pytest.mark.parametrize("use_roi", [False, True])
def test_d_x_of_the_autograd_path(one_launch, use_roi):
    """d X is layer 0's d layer_in product written straight into the caller's tensor (landmark-only model) or all in_dim columns
    of d Z (ROI model): against the float64 product of the gate gradients the pass left in its workspace."""
    import silent_speech_amd as ss

    B, T, H = 5, 7, 192
    hw = (32, 32) if use_roi else None
    sd = W.make_state_dict(17, 84, 5, use_roi)
    X, Lh, R, y = W.make_inputs(17, B, T, 84, 5, hw)
    m = ss.BiGRUClassifier(84, 5, use_roi=use_roi)
    m.load_state_dict(sd)
    m.cuda().eval()
    Xg = X.cuda().requires_grad_()
    loss = torch.nn.functional.cross_entropy(m(Xg, Lh.cuda(), R.cuda() if use_roi else None), y.cuda(), label_smoothing=0.05)
    loss.backward()
    ws = train_workspace(m)
    dG = ws.dG[0].cpu().numpy().astype(np.float64).reshape(2, B * T, 4 * H)[:, :, :3 * H]
    Wd = [sd[k].numpy().astype(np.float64) for k in ("gru.weight_ih_l0", "gru.weight_ih_l0_reverse")]
    want = (dG[0] @ Wd[0] + dG[1] @ Wd[1])[:, :84]
    bound = f32_bound(np.concatenate([np.abs(dG[0]), np.abs(dG[1])], axis=1), np.concatenate([np.abs(Wd[0]), np.abs(Wd[1])], axis=0)[:, :84],
                      2 * 3 * H)
    got = Xg.grad.cpu().numpy().astype(np.float64).reshape(B * T, 84)
    assert float(np.abs(want).max()) > 0
    assert (np.abs(got - want) <= bound + 1e-30).all(), float((np.abs(got - want) / (bound + 1e-30)).max())
