"""GPU: mixup on the device-planned path -- ss_batch_plan_mixup and ss_batch_mixup against tests/mixup_ref.py, the two-label loss
(ss_ce_ls_mix_fwd_bwd, ss_tail_fwd_mix) against float64 ``lam * CE(y) + (1 - lam) * CE(y_b)``, ``Trainer.step(mix=)`` against the CPU
oracle under autograd, ``DeviceClipStore.batch`` with mixup on, and ``fit`` with a resumed plan.  Figures are printed before they
are compared."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mixup_ref as M  # noqa: E402
import weights as W  # noqa: E402
from gpu_support import L, WORDS, cuda, make_weights, ss, tail_call, write_clips  # noqa: E402, F401
from oracle import model_ref as MR  # noqa: E402
from oracle import model_ref_bf16 as MB  # noqa: E402

U = 2.0 ** -24
SS_ERR_ARG = -1


@pytest.fixture(scope="module")
def table():
    from silent_speech_amd.device_data import mixup_table

    host = mixup_table(0.4)
    return host, torch.from_numpy(host.astype(np.int16)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the plan kernel
def plan_call(L, lens_d, y_d, B, augment, first, seed, prob, table_d, N=None):
    out = dict(perm=torch.full((max(B, 1),), -5, dtype=torch.int32, device="cuda"),
               y_b=torch.full((max(B, 1),), -5, dtype=torch.int64, device="cuda"),
               lens_m=torch.full((max(B, 1),), -5, dtype=torch.int64, device="cuda"),
               k=torch.full((1,), -5, dtype=torch.int32, device="cuda"), lam=torch.full((1,), -5.0, device="cuda"))
    st = L.load().ss_batch_plan_mixup(lens_d.data_ptr(), y_d.data_ptr(), B, int(augment), first, seed, prob, table_d.data_ptr(),
                                      table_d.numel() if N is None else N, out["perm"].data_ptr(), out["y_b"].data_ptr(),
                                      out["lens_m"].data_ptr(), out["k"].data_ptr(), out["lam"].data_ptr(), L.stream())
    torch.cuda.synchronize()
    return st, out


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 256, 1024])
def test_plan_kernel_equals_the_restatement(L, table, B):
    host, table_d = table
    rng = np.random.default_rng(B)
    lens, y = rng.integers(0, 91, B), rng.integers(0, 100, B)
    lens_d, y_d = torch.from_numpy(lens).cuda(), torch.from_numpy(y).cuda()
    ks = set()
    for seed in (0, 0x1234567887654321):
        for first in (17, 2 ** 32 + 2 ** 40 + 3):
            for augment in (0, 1):
                for prob in (0.0, 0.5, 1.0):
                    st, got = plan_call(L, lens_d, y_d, B, augment, first, seed, prob, table_d)
                    want = M.plan(lens, y, augment, first, seed, prob, host)
                    assert st == 0
                    assert np.array_equal(got["perm"].cpu().numpy(), want["perm"]), (seed, first, augment, prob)
                    assert np.array_equal(got["y_b"].cpu().numpy(), want["y_b"])
                    assert np.array_equal(got["lens_m"].cpu().numpy(), want["lens_m"])
                    assert int(got["k"]) == want["k"] and float(got["lam"]) == float(want["lam"]) == want["k"] / 256.0
                    assert want["mixed"] == bool(augment and (prob == 1.0 or (prob == 0.5 and want["mixed"])))
                    ks.add(want["k"])
    print(f"B={B}: k values seen {sorted(ks)}")
    assert 256 in ks and len(ks) > 1


def test_plan_kernel_refuses_and_writes_nothing(L, table):
    _, table_d = table
    lens_d = torch.zeros(1025, dtype=torch.int64, device="cuda")
    for B, N, prob in ((1025, None, 1.0), (0, None, 1.0), (4, 1000, 1.0), (4, None, 1.5)):
        st, got = plan_call(L, lens_d, lens_d, B, 1, 0, 0, prob, table_d, N)
        assert st == SS_ERR_ARG, (B, N, prob, st)
        assert all(bool((v == -5).all()) for v in got.values())


# ------------------------------------------------------------------------------------------------ 2. the blend kernel
def blend_call(L, X_d, ld_x, D, R_d, perm_d, k_d, B, T):
    Xm = None if X_d is None else torch.full_like(X_d, 7.0)
    Rm = None if R_d is None else torch.full_like(R_d, 7)
    fb = 0 if R_d is None else R_d[0, 0].numel()
    st = L.load().ss_batch_mixup(L.ptr(X_d), ld_x, D, L.ptr(Xm), L.ptr(R_d), L.ptr(Rm), fb, perm_d.data_ptr(), k_d.data_ptr(), B, T,
                                 L.stream())
    torch.cuda.synchronize()
    return st, Xm, Rm


def blend_inputs(B, T, D, hw, ld_x):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + D)
    X = torch.randn(B, T, ld_x, generator=g)
    X[:, :, D:] = 3.0  # (the columns behind D are nobody's)
    X[0, 0, :2] = torch.tensor([-0.0, 0.0])
    if B > 2:
        X[2] = 0.0  # a clip of zeros: where its partner has zeros too, the bound is zero
        X[B - 1, T - 1] = 0.0
    R = None if hw is None else torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8)
    perm = torch.randperm(B, generator=g)
    if B > 2:  # fixed points: a clip that is its own partner
        i, j = 1, int((perm == 1).nonzero()[0])
        perm[j], perm[i] = perm[i], 1
    return X, R, perm.to(torch.int32)


def check_blend(L, tag, X, R, perm, D, ks=(0, 1, 128, 255, 256)):
    B, T, ld_x = X.shape
    X_d, R_d, perm_d = cuda(X), None if R is None else cuda(R), cuda(perm)
    pn = perm.numpy()
    for k in ks:
        k_d = torch.tensor([k], dtype=torch.int32, device="cuda")
        st, Xm, Rm = blend_call(L, X_d, ld_x, D, R_d, perm_d, k_d, B, T)
        assert st == 0
        got = Xm.cpu().numpy()
        ref, tol = M.blend_f64(X.numpy()[:, :, :D], pn, k)
        err = np.abs(got[:, :, :D].astype(np.float64) - ref)
        print(f"{tag} k={k}: X max err {err.max():.3e}, largest err / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert np.all(err <= tol)
        keep = M.passthrough_rows(pn, k)
        assert got[keep][:, :, :D].tobytes() == X.numpy()[keep][:, :, :D].tobytes()  # byte for byte: -0.0 stays -0.0
        assert np.all(got[:, :, D:] == 7.0)  # the columns behind D are not written
        if R is not None:
            assert np.array_equal(Rm.cpu().numpy(), M.blend_u8(R.numpy(), pn, k)), k


@pytest.mark.parametrize("B,T,D,hw", [(1, 1, 83, (32, 32)), (3, 2, 84, (48, 96)), (40, 30, 84, (64, 64)), (33, 63, 83, (64, 64))])
def test_blend_kernel(L, B, T, D, hw):
    """The shapes of the issue and (33, 63): 2079 frames of 256 chunks, the smallest batch above the 2048 workgroups of 256 lanes
    the frame stream is capped at, so a lane walks more than one chunk.  Every k on every shape."""
    X, R, perm = blend_inputs(B, T, D, hw, D)
    check_blend(L, f"({B},{T},{D},{hw[0]}x{hw[1]})", X, R, perm, D)


def test_blend_kernel_wide_rows_null_pairs_and_the_feature_grid_cap(L):
    # ld_x > D, 16 bytes per lane (84 | 88) and one element per lane (83 | 90); each NULL pair
    for D, ld in ((84, 88), (83, 90)):
        X, R, perm = blend_inputs(5, 3, D, (32, 32), ld)
        check_blend(L, f"ld_x {ld} > D {D}", X, R, perm, D)
        check_blend(L, f"ld_x {ld} > D {D}, R NULL", X, None, perm, D, ks=(77,))
        k_d = torch.tensor([77], dtype=torch.int32, device="cuda")
        st, _, Rm = blend_call(L, None, 0, 0, cuda(R), cuda(perm), k_d, 5, 3)
        assert st == 0 and np.array_equal(Rm.cpu().numpy(), M.blend_u8(R.numpy(), perm.numpy(), 77))
    # past the 2048 x 256 lanes of the feature stream: 50 x 500 x 84 / 4 = 525 000 chunks of 16 bytes > 524 288
    X, _, perm = blend_inputs(50, 500, 84, None, 84)
    check_blend(L, "features past the grid cap", X, None, perm, 84, ks=(200,))
    # refusals: both pairs NULL, half a pair, in place, ld_x < D, frames that are no multiple of 16 bytes or not 16-byte aligned
    lib, s = L.load(), L.stream()
    X_d, R_d, p_d = cuda(X[:2, :2]), torch.zeros(2, 2, 32, 32, dtype=torch.uint8, device="cuda"), cuda(perm[:2] * 0)
    k_d = torch.tensor([128], dtype=torch.int32, device="cuda")
    Xm, Rm = torch.empty_like(X_d), torch.empty_like(R_d)
    x, xm, r, rm, p, k = (t.data_ptr() for t in (X_d, Xm, R_d, Rm, p_d, k_d))
    assert lib.ss_batch_mixup(None, 84, 84, None, None, None, 1024, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(x, 84, 84, None, None, None, 0, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(None, 0, 0, None, r, None, 1024, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(x, 84, 84, x, None, None, 0, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(x, 80, 84, xm, None, None, 0, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(None, 0, 0, None, r + 4, rm, 1008, p, k, 2, 2, s) == SS_ERR_ARG
    assert lib.ss_batch_mixup(None, 0, 0, None, r, rm, 1000, p, k, 2, 2, s) == -3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the two-label loss
def reference(lg, y, y_b, lam, w, eps):
    """float64 on the CPU: (lam CE(y) + (1 - lam) CE(y_b), its gradient), both terms over the one normaliser of y (the sum of
    w[y], or the row count)."""
    x = lg.double().clone().requires_grad_(True)
    w64 = None if w is None else w.double()
    den = float(len(y)) if w is None else float(w64[y].sum())
    ce = lambda t: F.cross_entropy(x, t, weight=w64, label_smoothing=eps, reduction="sum") / den  # noqa: E731
    loss = lam * ce(y) + (1.0 - lam) * ce(y_b)
    loss.backward()
    return float(loss.detach()), x.grad


def ce_mix(L, lg_d, y_d, yb_d, lam_d, eps, w_d=None, den_d=None, denom=None):
    B, C = lg_d.shape
    d = torch.full((B, C), 9.0, device="cuda")
    loss, correct = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    L.call("ss_ce_ls_mix_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), yb_d.data_ptr(), lam_d.data_ptr(), B, C, eps,
           float(B if denom is None else denom), L.ptr(w_d), L.ptr(den_d), d.data_ptr(), loss.data_ptr(), correct.data_ptr(),
           L.stream())
    torch.cuda.synchronize()
    return d, loss, correct


def ce_plain(L, lg_d, y_d, eps, w_d=None, den_d=None):
    B, C = lg_d.shape
    d = torch.full((B, C), 5.0, device="cuda")
    loss, correct = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    if w_d is None:
        L.call("ss_ce_ls_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, float(B), d.data_ptr(), loss.data_ptr(),
               correct.data_ptr(), L.stream())
    else:
        L.call("ss_ce_ls_w_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, w_d.data_ptr(), den_d.data_ptr(), d.data_ptr(),
               loss.data_ptr(), correct.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return d, loss, correct


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 10, 64, 65, 100, 129])
@pytest.mark.parametrize("B", [1, 16, 65])
def test_mix_ce_kernel(L, B, C, weighted):
    g = torch.Generator().manual_seed(1000 * B + C)
    lg = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    y_b = y[torch.randperm(B, generator=g)] if B > 1 else (y + 1) % C
    w = make_weights(g, C) if weighted else None
    lg_d, y_d, yb_d = cuda(lg), cuda(y), cuda(y_b)
    w_d = None if w is None else cuda(w)
    den_d = None
    if weighted:
        den_d = torch.empty(1, device="cuda")
        L.call("ss_class_weight_sum", y_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
    hits = int((torch.from_numpy(np.argmax(lg.numpy(), 1)) == y).sum())
    for eps in (0.0, 0.05):
        for k in (0, 1, 77, 128, 255):
            lam = k / 256.0
            d, loss, correct = ce_mix(L, lg_d, y_d, yb_d, torch.tensor([lam], device="cuda"), eps, w_d, den_d)
            loss_ref, grad_ref = reference(lg, y, y_b, lam, w, eps)
            e_loss, err = abs(float(loss) - loss_ref), (d.double().cpu() - grad_ref).abs()
            if k in (0, 77):
                print(f"B={B} C={C} w={weighted} eps={eps} k={k}: loss err {e_loss:.3e} (ref {loss_ref:.6f}), "
                      f"d_logits max err {float(err.max()):.3e}")
            assert e_loss < 2e-6 * max(1.0, abs(loss_ref))
            assert bool((err <= 1e-7 + 1e-5 * grad_ref.abs()).all()), float((err - 1e-5 * grad_ref.abs()).max())
            assert int(correct) == hits  # argmax == y, the rows' own labels
        # k = 256: the bits of the one-label kernels
        d, loss, correct = ce_mix(L, lg_d, y_d, yb_d, torch.ones(1, device="cuda"), eps, w_d, den_d)
        d1, loss1, correct1 = ce_plain(L, lg_d, y_d, eps, w_d, den_d)
        assert torch.equal(d, d1), float((d - d1).abs().max())
        assert int(correct) == int(correct1)
        if B <= 64:  # one wave: one atomic into a zero
            assert loss.cpu().numpy().tobytes() == loss1.cpu().numpy().tobytes()
        else:
            assert abs(float(loss) - float(loss1)) <= (B - 1) * U * abs(float(loss1))
    # a label outside the classes in either vector: a zero row that adds nothing
    if B >= 16:
        ya, yb = y.clone(), y_b.clone()
        ya[3], yb[5], yb[7] = -1, C, 2 ** 32 + 1
        keep = [b for b in range(B) if b not in (3, 5, 7)]
        d, loss, _ = ce_mix(L, lg_d, cuda(ya), cuda(yb), torch.tensor([0.25], device="cuda"), 0.05, w_d, den_d)
        # (the normaliser stays the one of the call: the sum over y as planned, or B)
        x = lg.double().clone().requires_grad_(True)
        w64 = None if w is None else w.double()
        den = float(B) if w is None else float(den_d)
        ce = lambda t: F.cross_entropy(x[keep], t[keep], weight=w64, label_smoothing=0.05, reduction="sum") / den  # noqa: E731
        ref = 0.25 * ce(ya) + 0.75 * ce(yb)
        ref.backward()
        ref = ref.detach()
        assert not bool(d[[3, 5, 7]].any())
        assert abs(float(loss) - float(ref)) < 2e-6 * max(1.0, abs(float(ref)))
        assert bool(((d.double().cpu() - x.grad).abs() <= 1e-7 + 1e-5 * x.grad.abs()).all())


@pytest.mark.parametrize("C", [2, 10, 64, 65, 100, 129])
def test_mix_tail(L, C):
    """ss_tail_fwd_mix on its own logits against the float64 two-label loss, weighted and not; lam = 1 gives the bits of ss_tail_fwd
    and ss_tail_fwd_w; a label outside the classes in either vector gives a zero row."""
    B, T, Hd, lengths = 16, 11, 192, [4, 1, 5, 9, 2, 11, 3, 7, 11, 6, 1, 2, 10, 8, 5, 3]
    g = torch.Generator().manual_seed(B * 7 + C)
    sd = {k: v for k, v in W.make_state_dict(31 + C, 84, C, False, hidden=Hd).items() if k.startswith(("pool.", "head."))}
    P = {k: cuda(v) for k, v in sd.items()}
    h = torch.randn(B, T, 2 * Hd, generator=g)
    for b in range(B):
        h[b, lengths[b]:] = 0
    y = torch.randint(0, C, (B,), generator=g)
    y_b = y[torch.randperm(B, generator=g)]
    w = make_weights(g, C)
    h_d, len_d, y_d, yb_d, w_d = cuda(h), cuda(torch.tensor(lengths, dtype=torch.int32)), cuda(y), cuda(y_b), cuda(w)
    den_d = torch.empty(1, device="cuda")
    L.call("ss_class_weight_sum", y_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
    dims = (B, T, 2 * Hd, 128, C)
    one = torch.ones(1, device="cuda")
    for weights, norm_mix, old_name, norm_old in ((None, (float(B), None, None), "ss_tail_fwd", (float(B),)),
                                                  (w, (1.0, w_d.data_ptr(), den_d.data_ptr()), "ss_tail_fwd_w",
                                                   (w_d.data_ptr(), den_d.data_ptr()))):
        for lam in (0.0, 1 / 256, 0.3125):
            lam_d = torch.tensor([lam], device="cuda")
            out = tail_call(L, "ss_tail_fwd_mix", P, h_d, len_d, y_d, dims, 0.05, norm_mix, (yb_d.data_ptr(), lam_d.data_ptr()))
            logits = out["logits"].cpu()
            loss_ref, grad_ref = reference(logits, y, y_b, lam, weights, 0.05)
            err = (out["d_logits"].double().cpu() - grad_ref).abs()
            print(f"tail C={C} weighted={weights is not None} lam={lam}: loss err {abs(float(out['loss']) - loss_ref):.3e}, "
                  f"d_logits max err {float(err.max()):.3e}")
            assert abs(float(out["loss"]) - loss_ref) < 2e-6 * max(1.0, abs(loss_ref))
            assert bool((err <= 1e-7 + 1e-5 * grad_ref.abs()).all())
            assert int(out["correct"]) == int((torch.from_numpy(np.argmax(logits.numpy(), 1)) == y).sum())
        new = tail_call(L, "ss_tail_fwd_mix", P, h_d, len_d, y_d, dims, 0.05, norm_mix, (yb_d.data_ptr(), one.data_ptr()))
        old = tail_call(L, old_name, P, h_d, len_d, y_d, dims, 0.05, norm_old)
        for k in ("logits", "d_logits", "attn", "xhat", "rstd", "ln", "mid", "mid_d"):
            assert torch.equal(old[k], new[k]), k
        assert int(old["correct"]) == int(new["correct"])
        assert abs(float(old["loss"]) - float(new["loss"])) <= (B - 1) * U * abs(float(old["loss"]))  # (sixteen atomics, any order)
        ya, yb = y.clone(), y_b.clone()
        ya[0], yb[4] = -1, C
        keep = [b for b in range(B) if b not in (0, 4)]
        lam_d = torch.tensor([0.75], device="cuda")
        ya_d, ybad_d = cuda(ya), cuda(yb)  # (held here: a pointer alone does not keep a tensor alive)
        out = tail_call(L, "ss_tail_fwd_mix", P, h_d, len_d, ya_d, dims, 0.05, norm_mix, (ybad_d.data_ptr(), lam_d.data_ptr()))
        x = out["logits"].cpu().double().requires_grad_(True)
        den = float(B) if weights is None else float(den_d)
        w64 = None if weights is None else weights.double()
        ce = lambda t: F.cross_entropy(x[keep], t[keep], weight=w64, label_smoothing=0.05, reduction="sum") / den  # noqa: E731
        ref = 0.75 * ce(ya) + 0.25 * ce(yb)
        ref.backward()
        ref = ref.detach()
        assert not bool(out["d_logits"][0].any()) and not bool(out["d_logits"][4].any())
        assert abs(float(out["loss"]) - float(ref)) < 2e-6 * max(1.0, abs(float(ref)))
        assert bool(((out["d_logits"].double().cpu() - x.grad).abs() <= 1e-7 + 1e-5 * x.grad.abs()).all())


# ------------------------------------------------------------------------------------------------ 4. Trainer.step(mix=)
def two_label_loss(logits, y, y_b, lam, eps=0.05):
    return lam * F.cross_entropy(logits, y, label_smoothing=eps) + (1.0 - lam) * F.cross_entropy(logits, y_b, label_smoothing=eps)


def mixed_batch(seed, B, T, x_dim, C, hw, k):
    """A batch, its partners and the blended batch the store would hand the trainer (tests/mixup_ref.py)."""
    X, Lh, R, y = W.make_inputs(seed, B, T, x_dim, C, hw, zero_padding=True)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed)).numpy()
    Xm = torch.from_numpy(M.blend_f32(X.numpy(), perm, k))
    Rm = None if R is None else torch.from_numpy(M.blend_u8(R.numpy(), perm, k))
    return Xm, torch.maximum(Lh, Lh[perm]), Rm, y, y[perm]


@pytest.mark.parametrize("name,hw", [("landmarks", None), ("roi32", (32, 32))])
def test_trainer_step_with_mix_matches_the_oracle(ss, name, hw):
    """Dropout off, B = 16, T = 12: loss and every gradient tensor of ``Trainer.step(mix=)`` against oracle/model_ref.py run on the
    mixed batch with the two-label loss under autograd.  Bounds of the existing trainer tests: loss 3e-6 * max(1, |ref|), gradients
    2e-5 * max|ref| + 1e-8 + 1e-4 |ref| per tensor."""
    B, T, C, k = 16, 12, 10, 77
    lam = k / 256.0
    sd = W.make_state_dict(11, 84, C, hw is not None)
    Xm, Lm, Rm, y, y_b = mixed_batch(5, B, T, 84, C, hw, k)
    m = ss.BiGRUClassifier(84, C, use_roi=hw is not None)
    m.load_state_dict(sd)
    m.cuda().eval()
    tr = ss.Trainer(m, dropout=False)
    Xd, Rd = cuda(Xm), None if Rm is None else cuda(Rm)
    loss, correct = tr.step(Xd, cuda(Lm), Rd, cuda(y), mix=(cuda(y_b), torch.tensor([lam], device="cuda")))
    torch.cuda.synchronize()
    bucket = m.flat_grads.clone()
    leaves = {k_: v.detach().clone().requires_grad_(True) for k_, v in sd.items()}
    logits = MR.forward(leaves, Xm, Lm, Rm)
    loss_ref = two_label_loss(logits, y, y_b, lam)
    grads = dict(zip(leaves, torch.autograd.grad(loss_ref, list(leaves.values()))))
    loss_ref, logits = loss_ref.detach(), logits.detach()
    print(f"{name}: step loss {float(loss):.7f}, oracle {float(loss_ref):.7f}, diff {abs(float(loss) - float(loss_ref)):.3e}")
    G = m._views_of(bucket)
    worst = {}
    for k_, ref in grads.items():
        err = (G[k_].cpu() - ref).abs()
        bound = 2e-5 * float(ref.abs().max()) + 1e-8 + 1e-4 * ref.abs()
        worst[k_] = float((err / bound).max())
        print(f"  {k_}: max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e}, err / bound {worst[k_]:.3f}")
    assert abs(float(loss) - float(loss_ref)) < 3e-6 * max(1.0, abs(float(loss_ref)))
    assert int(correct) == int((logits.argmax(1) == y).sum())
    assert all(v <= 1.0 for v in worst.values()), {k_: v for k_, v in worst.items() if v > 1.0}
    # the refusals
    with pytest.raises(ValueError, match="micro_batches"):
        ss.Trainer(m, dropout=False, micro_batches=2).step(Xd, cuda(Lm), Rd, cuda(y), mix=(cuda(y_b), torch.ones(1, device="cuda")))
    with pytest.raises(ValueError, match="mix"):
        tr.step_embedded(Xd, cuda(Lm), cuda(y), mix=(cuda(y_b), torch.ones(1, device="cuda")))
    with pytest.raises(ValueError, match="partner label"):
        tr.step(Xd, cuda(Lm), Rd, cuda(y), mix=(cuda(y_b[:3]), torch.ones(1, device="cuda")))


def test_bf16_engine_step_with_mix(ss):
    """One mixed step of the bf16 engine at the shape of tests/test_gpu_model_c5.py::test_c5_fused_trainer, at the distances that test
    allows its step: loss within 1e-2 and gradient norm within 3 % of the oracle's (the bf16 restatement for the loss, the f32 model
    under autograd for the norm); and the fused tail's own 3e-6 against float64 on the step's logits."""
    C5 = dict(roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96))
    B, T, k = 12, 6, 77
    lam = k / 256.0
    sd = W.make_state_dict(4, 84, 100, True, **C5)
    Xm, Lm, Rm, y, y_b = mixed_batch(4, B, T, 84, 100, (96, 96), k)
    m = ss.BiGRUClassifier(84, 100, use_roi=True, precision="bf16", **C5)
    m.load_state_dict(sd)
    m.cuda().eval()
    tr = ss.Trainer(m, dropout=False)
    Xd, Rd = cuda(Xm), cuda(Rm)
    loss, correct = tr.step(Xd, cuda(Lm), Rd, cuda(y), mix=(cuda(y_b), torch.tensor([lam], device="cuda")))
    torch.cuda.synchronize()
    logits = m._workspace(Xd, Rd, train=True, slot=0).logits.cpu()
    own = float(two_label_loss(logits.double(), y, y_b, lam))
    _, logits_emu, _ = MB.loss_and_grads(sd, Xm, Lm, Rm, y)
    emu = float(two_label_loss(logits_emu.double(), y, y_b, lam))
    leaves = {k_: v.detach().clone().requires_grad_(True) for k_, v in sd.items()}
    grads = torch.autograd.grad(two_label_loss(MR.forward(leaves, Xm, Lm, Rm), y, y_b, lam), list(leaves.values()))
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
    print(f"bf16 mixed step: loss {float(loss):.7f}, float64 on its logits {own:.7f}, bf16 restatement {emu:.7f}; "
          f"gradient norm {float(tr.grad_norm()):.6f}, f32 oracle {total:.6f}")
    assert abs(float(loss) - own) < 3e-6 * max(1.0, abs(own))
    assert abs(float(loss) - emu) < 1e-2
    assert abs(float(tr.grad_norm()) - total) < 3e-2 * total
    assert int(correct) == int((logits.argmax(1) == y).sum())
    m.check_health()


# ------------------------------------------------------------------------------------------------ 5. the store and fit
COUNTS = (8, 5, 2)


@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    """3 words x (8, 5, 2) clips, built the way the other fit tests build their directory."""
    return write_clips(str(tmp_path_factory.mktemp("mixup") / "clips_npz"), WORDS, counts=COUNTS)


def test_store_batch_with_mixup(ss, L, clip_dir):
    from silent_speech_amd import harness as Hn
    from silent_speech_amd.device_data import mixup_table

    info = Hn.scan_clips(clip_dir)
    store = ss.DeviceClipStore(info["files"], info["label_to_id"], max_t=24)
    idx = [3, 0, 7, 7, 12, 1, 14, 9, 2]
    base = ss.AugmentPolicy.lineage(time_mask_prob=0.5, time_mask_max=4, feat_mask_prob=0.5, feat_mask_max=3)
    host = mixup_table(0.4)
    seen = set()
    for seed, first in ((5, 100), (6, 2 ** 33 + 9), (7, 0)):
        kw = dict(augment=True, rng="philox", seed=seed, first_row=first)
        X0, T0, R0, y0 = (t.cpu().clone() for t in store.batch(idx, policy=base, **kw))
        Xm, Tm, Rm, ym = store.batch(idx, policy=ss.AugmentPolicy.lineage(**{**base.mask_fields(), "mixup_prob": 1.0, "mixup_alpha": 0.4}),
                                     **kw)
        y_b, lam, perm, k = store.mix
        torch.cuda.synchronize()
        want = M.plan(T0.numpy(), y0.numpy(), True, first, seed, 1.0, host)
        assert np.array_equal(perm.cpu().numpy(), want["perm"]) and int(k) == want["k"] and float(lam) == want["k"] / 256.0
        assert np.array_equal(y_b.cpu().numpy(), want["y_b"]) and np.array_equal(Tm.cpu().numpy(), want["lens_m"])
        assert torch.equal(ym.cpu(), y0)
        assert np.array_equal(Rm.cpu().numpy(), M.blend_u8(R0.numpy(), want["perm"], want["k"]))
        ref, tol = M.blend_f64(X0.numpy(), want["perm"], want["k"])
        err = np.abs(Xm.cpu().numpy().astype(np.float64) - ref)
        print(f"seed {seed}: k {want['k']}, perm {want['perm'].tolist()}, X max err {err.max():.3e}")
        assert np.all(err <= tol)
        seen.add(want["k"])
    assert len(seen) > 1
    # mixup_prob = 0: the launches and the outputs of the policy without the fields
    kw = dict(augment=True, rng="philox", seed=5, first_row=100)
    outs, launches = [], []
    for pol in (base, ss.AugmentPolicy.lineage(**{**base.mask_fields(), "mixup_prob": 0.0, "mixup_alpha": 0.4})):
        store.mix = None
        L.PROFILE = {}
        try:
            outs.append([None if t is None else t.cpu().clone() for t in store.batch(idx, policy=pol, **kw)])
            launches.append({name: len(v) for name, v in L.PROFILE.items()})
        finally:
            L.PROFILE = None
        assert store.mix is None
    assert launches[0] == launches[1] and not any("mixup" in name for name in launches[1])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # what the path refuses
    mix = ss.AugmentPolicy(mixup_prob=1.0)
    with pytest.raises(ValueError):
        store.batch(idx, augment=True, rng="device", policy=mix)
    with pytest.raises(ValueError, match="mixup"):
        store.batch(idx, augment=True, rng="philox", policy=mix, embedded=True)
    with pytest.raises(ValueError, match="whole batch"):
        store.batch(idx, augment=True, rng="philox", policy=mix, first_row=4, batch_first_row=0)
    store.check()


def test_fit_with_mixup_and_a_resumed_plan(ss, clip_dir, tmp_path, monkeypatch):
    """Two epochs of ``fit(plan="device")`` with every batch mixed: it runs and the history is finite; the run resumed behind epoch 1
    plans epoch 2 with the partners and factors of the uninterrupted one (the plan only: the weights differ by float-atomic order)."""
    from silent_speech_amd import harness as Hn

    plans = []
    real = ss.DeviceClipStore._mixup

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        y_b, lam, perm, k = self.mix
        plans[-1].append((perm.cpu().tolist(), int(k), float(lam), y_b.cpu().tolist(), out[1].cpu().tolist()))
        return out

    monkeypatch.setattr(ss.DeviceClipStore, "_mixup", spy)
    pol = ss.AugmentPolicy(mixup_prob=1.0)
    FIT = dict(epochs=2, batch_size=4, patience=5, max_t=24, lr=3e-3, plan="device", augment_policy=pol, log=lambda *a: None)
    plans.append([])
    history = []
    best = Hn.fit(clip_dir, str(tmp_path / "a.pt"), history=history, state_path=str(tmp_path / "a.state"), **FIT)
    assert len(history) == 2 and best >= 0
    assert all(np.isfinite(h[key]) for h in history for key in ("train_loss", "train_acc", "val_loss", "val_acc"))
    assert all(h["train_loss"] > 0 for h in history)
    per_epoch = len(plans[0]) // 2
    assert per_epoch >= 3 and len(plans[0]) == 2 * per_epoch
    assert len({p[1] for p in plans[0]}) > 1 and any(p[0] != sorted(p[0]) for p in plans[0])
    plans.append([])
    Hn.fit(clip_dir, str(tmp_path / "b.pt"), state_path=str(tmp_path / "b.state"), **dict(FIT, epochs=1))
    plans.append([])
    hb = []
    Hn.fit(clip_dir, str(tmp_path / "b.pt"), state_path=str(tmp_path / "b.state"), resume=True, history=hb, **FIT)
    assert [h["epoch"] for h in hb] == [2]
    assert plans[1] == plans[0][:per_epoch]
    assert plans[2] == plans[0][per_epoch:]
    # a state file of a run without mixup is not resumed by one with it
    with pytest.raises(ValueError, match="augment_policy"):
        Hn.fit(clip_dir, str(tmp_path / "b.pt"), state_path=str(tmp_path / "b.state"), resume=True,
               **dict(FIT, augment_policy=ss.AugmentPolicy(mixup_prob=1.0, mixup_alpha=0.4)))
