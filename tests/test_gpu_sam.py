"""GPU: sharpness-aware minimisation in the fused train step (``Trainer.enable_sam``, ``harness.fit_sam``).

The three entry points -- ``ss_sumsq_absw_f32``, ``ss_sam_perturb``, ``ss_sam_restore_sumsq`` (csrc/optim.hip) -- at their tail, lane,
workgroup and grid-cap edges on NaN-guarded sub-ranges against tests/sam_ref.py (float64, bounds counted in rounded operations;
tests/test_sam_cpu.py pins it against torch autograd without a GPU), bit for bit where the arithmetic is exact; then the trainer:
against the CPU oracle stepped twice per step, the weights' bits around the step, the launch list, the returned loss, the state,
a resumed ``fit`` and the one-rank RCCL leg.  Every test prints what it measured before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import flat_ref as FR
import sam_ref as SR
import trainer_trace as TT
import weights as W
from gpu_support import L, WORDS, ss, write_clips  # noqa: F401
from oracle import model_ref as MR
from oracle import model_ref_bf16 as MB
from test_gpu_adamw_groups import WD, Guarded, check_against_oracle, groups_of, new_model
from test_gpu_ema_resume import ADAM, B_, FIT, LOSS_BOUND, ROI, T_, bits
from test_gpu_launch_trace import first_difference

pytestmark = pytest.mark.gpu

RHO, LR = 0.05, ADAM[2]
NS = [1, 3, 4, 5, 1023, 1024, 1027]
# one size just past each kernel's grid cap times its unroll: the sums walk as ss_sumsq_f32 does (flat_ref.sumsq_grid: 256 workgroups
# of 256 lanes, four quads in flight), ss_sam_perturb on ss_flat_grid's 2048 workgroups with two quads in flight
SUMSQ_PAST_CAP = FR.sumsq_grid(1 << 40)[1] * 4 * 4 + 7
PERTURB_PAST_CAP = 2048 * 256 * 4 * 2 + 7


def sam_trainer(ss, model, sam_rho=None, sam_adaptive=False, **kw):
    """A ``Trainer(model, **kw)``, with ``enable_sam(sam_rho, sam_adaptive)`` behind it when ``sam_rho`` is given."""
    tr = ss.Trainer(model, **kw)
    if sam_rho is not None:
        tr.enable_sam(sam_rho, sam_adaptive)
    return tr


def case(n, seed):
    w, g = FR.optimiser_case(n, seed)[:2]
    junk = np.random.default_rng(seed + 3).integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32).view(np.float32)
    return w, g, junk


def device_word(value=0.0):
    return torch.tensor([value], dtype=torch.float32).cuda()


def norm_word(L, W_, G_, n, adaptive):
    """The sumsq word the trainer would hand to ss_sam_perturb: taken on the device from the guarded buffers."""
    s = device_word()
    if adaptive:
        L.call("ss_sumsq_absw_f32", W_.ptr, G_.ptr, n, s.data_ptr(), L.stream())
    else:
        L.call("ss_sumsq_f32", G_.ptr, n, s.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return s


def run_perturb(L, w, g, junk, s, rho, adaptive, grad_scale=1.0):
    """One launch on guarded sub-ranges (each begins 8 floats into its allocation) -> (new w, backup); asserts the guards, the +0
    gradient, the cleared scalars and their untouched neighbours, and the sumsq word."""
    n = w.size
    W_, G_, B_k = Guarded(w, 1), Guarded(g, 2), Guarded(junk, 3)
    zf, zi = torch.tensor([5.0, 6.0, 7.0]).cuda(), torch.tensor([8, 9], dtype=torch.int32).cuda()
    s0 = float(s[0])
    L.call("ss_sam_perturb", W_.ptr, G_.ptr, B_k.ptr, n, s.data_ptr(), grad_scale, rho, int(adaptive), zf.data_ptr(), 2, zi.data_ptr(), 1,
           L.stream())
    torch.cuda.synchronize()
    for b, name in ((W_, "w"), (G_, "g"), (B_k, "backup")):
        b.check_guards(name)
    assert np.array_equal(B_k.values().view(np.int32), w.view(np.int32)), "backup is not the old w, bit for bit"
    assert not G_.values().view(np.int32).any(), "g is not all +0"
    assert zf.tolist() == [0.0, 0.0, 7.0] and zi.tolist() == [0, 9] and float(s[0]) == s0
    return W_.values(), B_k.values()


# ------------------------------------------------------------------------------------------------------------ ss_sam_perturb
@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("n", NS + [PERTURB_PAST_CAP])
def test_perturb_against_float64(L, n, adaptive):
    w, g, junk = case(n, 40 + n % 1000)
    worst = 0.0
    s = norm_word(L, Guarded(w, 5), Guarded(g, 6), n, adaptive)
    for grad_scale in (1.0, 0.25):
        got, _ = run_perturb(L, w, g, junk, s, RHO, adaptive, grad_scale)
        want, bound = SR.perturb_expected(w, g, np.float32(float(s[0])), RHO, adaptive, grad_scale)
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n, adaptive, grad_scale, worst, int(np.argmax(err / bound)))
        assert not np.array_equal(got, w)  # (the launch did something)
    print(f"sam_perturb n={n} adaptive={adaptive}: largest err / bound {worst:.4f}")


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("n", NS + [PERTURB_PAST_CAP])
def test_perturb_is_exact_where_the_arithmetic_is(L, n, adaptive):
    """One nonzero gradient element, 0.5, at a weight 2; rho = 2**-4; the other weights nonzero multiples of 1/8.  The norm is 0.5
    (plain) or 1 (adaptive: |2| x 0.5), ``+ 1e-12`` rounds away, the scale is a power of two and ``e`` is 2**-4 (plain: rho x 0.5 /
    0.5) or 2**-3 (adaptive: rho x 0.5 x 2^2 / 1), a few ulps of 2: every operation is exact, so there is one right bit pattern
    whatever the kernel fuses.  ``grad_scale`` = 1/4 cancels exactly.  Every other weight gets ``+ 0`` and keeps its bits."""
    rng = np.random.default_rng(n)
    w = (rng.integers(1, 32, n) / 8.0).astype(np.float32) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
    for k in (sorted({0, n // 2, n - 1}) if n < 2000 else [n - 5]):
        g = np.zeros(n, np.float32)
        w_k = w.copy()
        w_k[k], g[k] = 2.0, 0.5
        for grad_scale in (1.0, 0.25):
            s = norm_word(L, Guarded(w_k, 5), Guarded(g, 6), n, adaptive)
            assert float(s[0]) == (1.0 if adaptive else 0.25)
            got, _ = run_perturb(L, w_k, g, w.copy(), s, 2.0 ** -4, adaptive, grad_scale)
            want = w_k.copy()
            want[k] = 2.0 + (2.0 ** -4 * 0.5 * 4.0 / 1.0 if adaptive else 2.0 ** -4 * 0.5 / 0.5)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, k, adaptive, grad_scale, got[k], want[k])


# ------------------------------------------------------------------------------------- ss_sam_restore_sumsq, ss_sumsq_absw_f32
@pytest.mark.parametrize("n", NS + [SUMSQ_PAST_CAP])
def test_restore_puts_the_bits_back_and_sums_as_sumsq_does(L, n):
    w, g, junk = case(n, 70 + n % 1000)
    exact = FR.sumsq_exact_input(n)
    for grads, is_exact in ((g, False), (exact, True)):
        P_, B_k, G_ = Guarded(w, 1), Guarded(junk, 2), Guarded(grads, 3)  # (backup: arbitrary bit patterns, NaN payloads included)
        acc, ref = device_word(), device_word()
        L.call("ss_sam_restore_sumsq", P_.ptr, B_k.ptr, G_.ptr, n, acc.data_ptr(), L.stream())
        L.call("ss_sumsq_f32", G_.ptr, n, ref.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert np.array_equal(P_.values().view(np.int32), junk.view(np.int32)), "w is not backup, bit for bit"
        P_.check_guards("w")
        B_k.check_untouched("backup")
        G_.check_untouched("g")
        want = float((grads.astype(np.float64) ** 2).sum())
        err, bound = abs(float(acc[0]) - want), SR.sumsq_bound(n, want)
        print(f"sam_restore_sumsq n={n} exact={is_exact}: err / bound {err / bound if bound else 0.0:.4f}")
        assert err <= bound
        if is_exact:
            assert want < 2 ** 24 and float(acc[0]) == want == float(ref[0])
        # it adds onto the word it is given
        L.call("ss_sam_restore_sumsq", P_.ptr, B_k.ptr, G_.ptr, n, acc.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert abs(float(acc[0]) - 2 * want) <= 2 * bound + FR.U * 2 * want


@pytest.mark.parametrize("n", NS + [SUMSQ_PAST_CAP])
def test_sumsq_absw_against_float64_and_exactly_on_small_integers(L, n):
    w, g, _ = case(n, 90 + n % 1000)
    wi = FR.sumsq_exact_input(n) * np.where(np.arange(n) % 3 == 0, -1, 1).astype(np.float32)  # (the sign must not matter)
    gi = FR.sumsq_exact_input(n + 1)[:n]
    for a, b, is_exact in ((w, g, False), (wi, gi, True)):
        A_, B_k = Guarded(a, 1), Guarded(b, 2)
        acc = device_word()
        L.call("ss_sumsq_absw_f32", A_.ptr, B_k.ptr, n, acc.data_ptr(), L.stream())
        torch.cuda.synchronize()
        A_.check_untouched("w")
        B_k.check_untouched("g")
        want = float(((np.abs(a).astype(np.float64) * b.astype(np.float64)) ** 2).sum())
        err, bound = abs(float(acc[0]) - want), SR.sumsq_bound(n, want, extra_ops=2)
        print(f"sumsq_absw n={n} exact={is_exact}: err / bound {err / bound if bound else 0.0:.4f}")
        assert err <= bound
        if is_exact:
            t = device_word()
            prod = torch.from_numpy((np.abs(a) * b).astype(np.float32)).cuda()
            L.call("ss_sumsq_f32", prod.data_ptr(), n, t.data_ptr(), L.stream())
            torch.cuda.synchronize()
            assert want < 2 ** 24 and float(acc[0]) == want == float(t[0])


def test_entry_points_refuse_bad_arguments_and_write_nothing(L):
    """(tests/test_sam_cpu.py walks every case on host memory; here on device buffers, then the good calls run.)"""
    n = 1031
    w, g, junk = case(n, 7)
    P_, G_, B_k = Guarded(w, 1), Guarded(g, 2), Guarded(junk, 3)
    s, zf, zi = device_word(1.0), torch.tensor([5.0]).cuda(), torch.tensor([8], dtype=torch.int32).cuda()
    lib = L.load()

    def perturb(p=P_.ptr, g_=G_.ptr, b=B_k.ptr, n_=n, s_=s.data_ptr(), rho=RHO, zf_=zf.data_ptr(), nzf=1, adaptive=0):
        return lib.ss_sam_perturb(p, g_, b, n_, s_, 1.0, rho, adaptive, zf_, nzf, zi.data_ptr(), 1, L.stream())

    def restore(p=P_.ptr, b=B_k.ptr, g_=G_.ptr, n_=n, s_=s.data_ptr()):
        return lib.ss_sam_restore_sumsq(p, b, g_, n_, s_, L.stream())

    for bad in (dict(p=None), dict(g_=None), dict(b=None), dict(s_=None), dict(n_=0), dict(n_=-1), dict(p=P_.ptr + 4, n_=n - 1),
                dict(g_=G_.ptr + 4, n_=n - 1), dict(b=B_k.ptr + 8, n_=n - 2), dict(b=P_.ptr), dict(b=P_.ptr + 16, n_=n - 4),
                dict(b=G_.ptr), dict(b=G_.ptr + 16 * 50, n_=n - 200)):
        assert perturb(**bad) == -1 and perturb(adaptive=1, **bad) == -1 and restore(**bad) == -1, bad
    for bad in (dict(rho=0.0), dict(rho=-1.0), dict(rho=float("nan")), dict(rho=float("inf")), dict(zf_=None), dict(nzf=257),
                dict(zf_=s.data_ptr())):
        assert perturb(**bad) == -1 and perturb(adaptive=1, **bad) == -1, bad
    for bad in (dict(w_=None), dict(g_=None), dict(s_=None), dict(n_=0), dict(w_=P_.ptr + 4, n_=n - 1), dict(g_=G_.ptr + 4, n_=n - 1)):
        kw = dict(dict(w_=P_.ptr, g_=G_.ptr, n_=n, s_=s.data_ptr()), **bad)
        assert lib.ss_sumsq_absw_f32(kw["w_"], kw["g_"], kw["n_"], kw["s_"], L.stream()) == -1, bad
    torch.cuda.synchronize()
    for b in (P_, G_, B_k):
        b.check_untouched("a refused call wrote")
    assert float(s[0]) == 1.0 and float(zf[0]) == 5.0 and int(zi[0]) == 8
    assert perturb() == 0 and restore() == 0
    torch.cuda.synchronize()
    assert np.array_equal(P_.values().view(np.int32), w.view(np.int32)) and float(zf[0]) == 0.0 and int(zi[0]) == 0
    for b in (P_, G_, B_k):
        b.check_guards("the good calls")


# ------------------------------------------------------------------------------------------- Trainer against the CPU oracle
@pytest.fixture(scope="module")
def tiny():
    sd = W.make_state_dict(11, 84, 5, True)
    return sd, W.make_inputs(31, B_, T_, 84, 5, ROI)


def oracle_sam_steps(ss, sd, inputs, rho, adaptive, steps, groups=None, frozen=False, engine=MR, model_kw=None):
    """The oracle's ``loss_and_grads`` twice per step -- at ``w`` and at ``w + e`` (tests/sam_ref.py's ``e`` over the trained
    parameters, float64 norm) -- then ``clip_grad_norm_`` + ``torch.optim.Adam`` (``AdamW`` with ``groups``) on the second gradient,
    dropout off.  -> (state dict after every step, first-pass loss of every step, norm of every second gradient)."""
    X, Lh, R, y = inputs
    host_model = ss.BiGRUClassifier(84, sd["head.4.bias"].numel(), **(model_kw or dict(use_roi=True)))
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
    if groups is None:
        trained = [k for k in sd if not (frozen and k.startswith("roi_cnn."))]
        opt = torch.optim.Adam([params[k] for k in trained], lr=LR)
    else:
        _, _, members = host_model.param_segments(groups, host_model.cnn_param_range() if frozen else 0)
        scales = [g.lr_scale for g in groups] + [1.0]
        decays = [WD if g.weight_decay is None else g.weight_decay for g in groups] + [WD]
        live = [(names, sc, wd) for names, sc, wd in zip(members, scales, decays) if names]
        trained = [k for names, _, _ in live for k in names]
        opt = torch.optim.AdamW([dict(params=[params[k] for k in names], lr=LR * sc, weight_decay=wd) for names, sc, wd in live], lr=LR)
    out, losses, norms = [], [], []
    for _ in range(steps):
        at_w = {k: p.detach().clone() for k, p in params.items()}
        loss, _, g1 = engine.loss_and_grads(at_w, X, Lh, R, y)
        w_flat = np.concatenate([at_w[k].double().reshape(-1).numpy() for k in trained])
        g_flat = np.concatenate([g1[k].double().reshape(-1).numpy() for k in trained])
        e_flat, at = SR.sam_perturbation(w_flat, g_flat, rho, adaptive), 0
        at_we = dict(at_w)
        for k in trained:
            n = at_w[k].numel()
            at_we[k] = at_w[k] + torch.from_numpy(e_flat[at:at + n]).reshape(at_w[k].shape).float()
            at += n
        _, _, g2 = engine.loss_and_grads(at_we, X, Lh, R, y)
        for k in trained:
            params[k].grad = g2[k].clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([params[k] for k in trained], 1.0)))
        opt.step()
        out.append({k: p.detach().clone() for k, p in params.items()})
        losses.append(float(loss))
    return out, losses, norms


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
def test_trainer_against_the_cpu_oracle(ss, tiny, adaptive):
    """Three SAM steps, dropout off, to the tolerances tests/test_gpu_model.py holds the parameters after Adam to
    (``check_against_oracle``); the returned loss is the first pass's and ``grad_norm()`` the second gradient's."""
    sd, (X, Lh, R, y) = tiny
    rho = 0.5 if adaptive else RHO  # (ASAM's radius is relative to the weights: its papers use ten times SAM's)
    want, losses, norms = oracle_sam_steps(ss, sd, (X, Lh, R, y), rho, adaptive, 3)
    model = new_model(ss, sd)
    tr = sam_trainer(ss, model, dropout=False, sam_rho=rho, sam_adaptive=adaptive)
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    for step in range(1, 4):
        loss, _ = tr.step(*dev)
        print(f"step {step}: loss {float(loss):.7f} (oracle {losses[step - 1]:.7f}), second-pass loss {float(tr.sam_scal[0]):.7f}, "
              f"|g'| {float(tr.grad_norm()):.6f} (oracle {norms[step - 1]:.6f})")
        assert abs(float(loss) - losses[step - 1]) < 1e-4 and float(tr.sam_scal[0]) > float(loss)
        assert abs(float(tr.grad_norm()) - norms[step - 1]) < 1e-3 * norms[step - 1]
        check_against_oracle(model.state_dict(), want[step - 1], f"step {step}")
    # SAM is visible: a plain Trainer ends elsewhere by far more than the tolerance
    plain = new_model(ss, sd)
    tp = ss.Trainer(plain, dropout=False)
    for _ in range(3):
        tp.step(*dev)
    a, b = plain.state_dict(), model.state_dict()
    moved = max(float((a[k] - b[k]).abs().max()) for k in ("gru.weight_hh_l0", "roi_cnn.net.0.weight", "head.4.weight"))
    print(f"plain against SAM after three steps: max |diff| {moved:.3e}")
    assert moved > 3e-5


def test_trainer_with_ema_and_groups_against_the_cpu_oracle(ss, tiny):
    sd, (X, Lh, R, y) = tiny
    want, _, _ = oracle_sam_steps(ss, sd, (X, Lh, R, y), RHO, False, 3, groups=groups_of(ss))
    model = new_model(ss, sd)
    tr = sam_trainer(ss, model, dropout=False, sam_rho=RHO, weight_decay=WD, param_groups=groups_of(ss), ema_decay=0.9)
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    for step in range(1, 4):
        tr.step(*dev)
        check_against_oracle(model.state_dict(), want[step - 1], f"groups + ema step {step}")
    assert not torch.equal(tr.ema, model.flat_params) and bool(torch.isfinite(tr.ema).all())


def test_frozen_trainer_against_the_cpu_oracle(ss, tiny):
    """``freeze_cnn`` + ``step_embedded``: SAM on ``[n_cnn, n)``; the CNN range, its average's and its backup's keep their bits."""
    sd, (X, Lh, R, y) = tiny
    want, _, _ = oracle_sam_steps(ss, sd, (X, Lh, R, y), RHO, False, 3, frozen=True)
    with torch.no_grad():
        roi_e = MR.forward(sd, X, Lh, R, return_intermediates=True)[1]["roi_e"]
    Z = torch.cat([X, roi_e], dim=2).cuda()
    model = new_model(ss, sd)
    tr = sam_trainer(ss, model, dropout=False, freeze_cnn=True, sam_rho=RHO)
    n_cnn = model.cnn_param_range()
    p0 = model.flat_params.clone()
    tr.backup.fill_(123.0)
    for step in range(1, 4):
        tr.step_embedded(Z, Lh.cuda(), y.cuda())
        check_against_oracle(model.state_dict(), want[step - 1], f"frozen step {step}")
    assert torch.equal(bits(model.flat_params[:n_cnn]), bits(p0[:n_cnn])) and bool((tr.backup[:n_cnn] == 123.0).all())
    assert not torch.equal(model.flat_params[n_cnn:], p0[n_cnn:]) and not bool((tr.backup[n_cnn:] == 123.0).any())
    assert all(torch.equal(want[-1][k], sd[k]) for k in sd if k.startswith("roi_cnn."))


BF16 = dict(use_roi=False, hidden=128, gru_layers=2, precision="bf16")


def test_bf16_trainer_against_the_bf16_oracle(ss):
    """The bf16 engine against ``oracle/model_ref_bf16.py`` stepped twice per step, to the bounds tests/test_gpu_model_c5.py holds
    its fused trainer to: the loss within 2e-3 of the bf16 restatement's, the clipped norm within 3 %, the logits after each step
    within 0.1 and their loss within 2e-2 (Adam's first steps move weights whose gradient lies within the bf16 noise of zero the
    other way)."""
    sd = W.make_state_dict(13, 84, 5, False, hidden=128)
    X, Lh, R, y = W.make_inputs(33, B_, T_, 84, 5, None)
    want, losses, norms = oracle_sam_steps(ss, sd, (X, Lh, None, y), RHO, False, 3, engine=MB, model_kw=BF16)
    model = ss.BiGRUClassifier(84, 5, **BF16)
    model.load_state_dict(sd)
    model.cuda().train()
    tr = sam_trainer(ss, model, dropout=False, sam_rho=RHO)
    for step in range(1, 4):
        loss, _ = tr.step(X.cuda(), Lh.cuda(), None, y.cuda())
        model.eval()
        with torch.no_grad():
            after = model(X.cuda(), Lh, None).cpu()
        model.train()
        ref_after = MB.forward(want[step - 1], X, Lh, None)
        d_logits = float((after - ref_after).abs().max())
        d_loss = abs(float(MR.ce_label_smoothing(after, y)) - float(MR.ce_label_smoothing(ref_after, y)))
        print(f"bf16 step {step}: loss {float(loss):.6f} (oracle {losses[step - 1]:.6f}), |g'| {float(tr.grad_norm()):.5f} (oracle "
              f"{norms[step - 1]:.5f}), logits after the step within {d_logits:.3e}, their loss within {d_loss:.3e}")
        assert abs(float(loss) - losses[step - 1]) < 2e-3
        assert abs(float(tr.grad_norm()) - norms[step - 1]) < 3e-2 * norms[step - 1]
        assert d_logits < 0.1 and d_loss < 2e-2


# --------------------------------------------------------------------------------------------------------- weights restored
@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
def test_weights_after_the_step_are_adam_on_the_bits_before_it(ss, L, tiny, adaptive):
    """The bucket, m and v are copied, the step is taken, and the step's final launch is replayed alone on the copies with the
    step's own second gradient and sumsq word: equal bits, so the perturbation left no trace in the weights."""
    sd, (X, Lh, R, y) = tiny
    model = new_model(ss, sd)
    tr = sam_trainer(ss, model, dropout=True, sam_rho=RHO, sam_adaptive=adaptive)
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    tr.step(*dev)
    p, m, v = model.flat_params.detach().clone(), tr.m.clone(), tr.v.clone()
    tr.step(*dev)
    n = p.numel()
    assert float(tr.scal[1]) > 0 and float(tr.scal[2]) > 0 and float(tr.scal[1]) != float(tr.scal[2])
    L.call("ss_adam_clip", p.data_ptr(), model.flat_grads.data_ptr(), m.data_ptr(), v.data_ptr(), n, tr.scal.data_ptr() + 4, 1.0,
           tr.max_norm, tr.lr, *tr.betas, tr.eps, tr.step_count, L.stream())
    torch.cuda.synchronize()
    for name, got, want in (("p", model.flat_params, p), ("m", tr.m, m), ("v", tr.v, v)):
        assert torch.equal(bits(got), bits(want)), name
    assert not torch.equal(tr.backup, model.flat_params)  # (the backup holds the weights of before the step)


# -------------------------------------------------------------------------------------------------------------- launch list
@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_trace_parent.json")) as f:
        return json.load(f)


SAM_TRACES = {"default": dict(sam_rho=RHO), "groups_ema": dict(sam_rho=RHO, sam_adaptive=True), "frozen": dict(sam_rho=RHO),
              "bf16_landmarks": dict(sam_rho=RHO), "weights_mix_teacher": dict(sam_rho=RHO), "int32_lengths": dict(sam_rho=RHO)}


@pytest.mark.parametrize("name", list(SAM_TRACES))
def test_launch_list_is_the_plain_one_with_the_second_pass(ss, parent, monkeypatch, name):
    """Against the recorded trace of the same configuration without SAM (tests/trainer_trace_parent.json, which a trainer without
    ``enable_sam`` still matches: asserted here for the same configurations): everything up to the first backward's end, the norm and
    the perturb launch, the forward and backward again entry for entry -- the same arguments, the dropout seeds among them, the
    same records and waits, and no zeroing of any kind --, then the restore launch in the place of ``ss_sumsq_f32`` and the
    optimiser's launch as it was."""
    kw, tkw, B, extra = TT.CONFIGS[name]
    plain = parent["steps"][name]
    assert TT.run_config(monkeypatch, name) == plain
    plain_trainer, sam = ss.Trainer, SAM_TRACES[name]

    def trainer_with_sam(model, **k):  # (run_config builds its trainer as ss.Trainer(model, **keywords): SAM is switched on behind it)
        tr = plain_trainer(model, **k)
        tr.enable_sam(sam["sam_rho"], sam.get("sam_adaptive", False))
        return tr

    with monkeypatch.context() as m:
        m.setattr(ss, "Trainer", trainer_with_sam)
        got = TT.run_config(monkeypatch, name)
    names = [e[1] for e in plain]
    head = max(i for i, e in enumerate(plain) if e[0] == "zero" or e[1] in ("ss_train_prologue", "ss_class_weight_sum")) + 1
    assert names[-2] == "ss_sumsq_f32" and plain[-1][1].startswith("ss_adam")
    first, (sumsq, adam) = [list(e) for e in plain[:-2]], plain[-2:]
    if first[0][1] == "ss_train_prologue":  # (the prologue also clears the third float, the first gradient's sum of squares)
        assert first[0][4][3] == 2
        first[0] = first[0][:4] + [first[0][4][:3] + [3] + first[0][4][4:]]
    else:
        assert first[1] == ["zero", 2]
        first[1] = ["zero", 3]
    n = sumsq[4][1]
    adaptive = SAM_TRACES[name].get("sam_adaptive", False)
    norm = ["launch", "ss_sumsq_absw_f32", "ss_sumsq_absw_f32", "main", ["ptr", "ptr", n, "ptr"]] if adaptive else sumsq
    perturb = ["launch", "ss_sam_perturb", "ss_sam_perturb", "main", ["ptr", "ptr", "ptr", n, "ptr", 1.0, RHO, int(adaptive), "ptr", 1, "ptr", 1]]
    restore = ["launch", "ss_sam_restore_sumsq", "ss_sam_restore_sumsq", "main", ["ptr", "ptr", "ptr", n, "ptr"]]
    want = first + [norm, perturb] + first[head:] + [restore, adam]
    print(f"{name}: {len(plain)} entries without SAM, {len(got)} with; the passes are {len(first) - head} entries each")
    assert got == want, f"{name}: " + first_difference(got, want)
    # spelled out: between the passes no zeroing, no prologue, nothing that writes the bucket or the scalars but the two launches;
    # the second pass's launches carry the first pass's arguments by value, the dropout seed (the step count, 2) among them
    second = got[len(first) + 2:-2]
    assert second == first[head:] and not any(e[0] == "zero" or e[1] == "ss_train_prologue" for e in second)
    assert [e[1] for e in got].count(sumsq[1]) == (0 if adaptive else 1)
    seeded = [e for e in second if e[0] == "launch" and e[1].startswith(("ss_tail_fwd", "ss_tail_bwd"))]
    assert len(seeded) == 2 and all(2 in e[4] for e in seeded)


# ------------------------------------------------------------------------------------------------------------ loss variants
@pytest.mark.parametrize("variant", ["class_weights", "mix", "teacher"])
def test_returned_loss_is_the_first_pass_loss(ss, tiny, variant):
    """One SAM step with class weights, ``mix=`` or ``teacher_logits=`` returns the loss (and the hits) of a plain trainer's first
    step from the same state -- within ``LOSS_BOUND``, the order of the loss's float atomics -- and its second pass, which sees the
    same loss description, a larger one."""
    sd, (X, Lh, R, y) = tiny
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    g = torch.Generator().manual_seed(3)
    tkw, skw = {}, {}
    if variant == "class_weights":
        tkw["class_weights"] = [1.0, 2.0, 0.5, 1.5, 1.0]
    elif variant == "mix":
        skw["mix"] = (dev[3].flip(0).contiguous(), torch.tensor([0.75], device="cuda"))
    else:
        skw["teacher_logits"] = torch.randn(B_, 5, generator=g).cuda()
    out = {}
    for label, extra in (("plain", {}), ("sam", dict(sam_rho=RHO))):
        tr = sam_trainer(ss, new_model(ss, sd), dropout=False, **tkw, **extra)
        loss, hits = tr.step(*dev, **skw)
        out[label] = (float(loss), int(hits), None if tr.sam_scal is None else (float(tr.sam_scal[0]), int(tr.sam_correct[0])))
    print(f"{variant}: plain {out['plain'][0]:.9f} SAM {out['sam'][0]:.9f} (diff {abs(out['plain'][0] - out['sam'][0]):.3e}), second "
          f"pass {out['sam'][2][0]:.9f}")
    assert abs(out["plain"][0] - out["sam"][0]) <= LOSS_BOUND and out["plain"][1] == out["sam"][1]
    assert out["sam"][2][0] > out["sam"][0] and 0 <= out["sam"][2][1] <= B_


def test_an_empty_shard_joins_the_perturb_the_restore_and_adam(ss, tiny):
    sd, (X, Lh, R, y) = tiny
    model = new_model(ss, sd)
    tr = sam_trainer(ss, model, sam_rho=RHO)
    before = model.flat_params.clone()
    tr.backup.fill_(9.0)
    loss, hits = tr.step(X[:0].cuda(), Lh[:0].cuda(), R[:0].cuda(), y[:0].cuda(), global_batch=B_)
    assert float(loss) == 0.0 and int(hits) == 0 and float(tr.grad_norm()) == 0.0 and tr.step_count == 1
    assert torch.equal(bits(model.flat_params), bits(before)) and torch.equal(bits(tr.backup), bits(before))
    assert not bool(tr.m.any()) and not bool(tr.v.any())


# -------------------------------------------------------------------------------------------------------------------- state
def test_trainer_state_keys_round_trip_and_mismatch(ss, tiny):
    from silent_speech_amd import checkpoint as Ck

    sd, (X, Lh, R, y) = tiny
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    old_keys = {"m", "v", "ema", "step_count", "ema_decay", "ema_warmup", "betas", "eps", "lr", "max_norm", "numel"}
    plain = ss.Trainer(new_model(ss, sd))
    assert set(plain.state_dict()) == old_keys and plain.backup is None and plain.sam_scal is None and plain.scal.numel() == 2
    m1 = new_model(ss, sd)
    t1 = sam_trainer(ss, m1, sam_rho=RHO, sam_adaptive=True)
    for _ in range(2):
        t1.step(*dev)
    state = t1.state_dict()
    assert set(state) == old_keys | {"sam_rho", "sam_adaptive"} and state["sam_rho"] == RHO and state["sam_adaptive"] is True
    assert not any(isinstance(v, torch.Tensor) and v.data_ptr() == t1.backup.data_ptr() for v in state.values())
    m2 = new_model(ss, {k: v.cpu() for k, v in m1.state_dict().items()})
    t2 = sam_trainer(ss, m2, sam_rho=RHO, sam_adaptive=True)
    t2.load_state_dict(Ck._plain(state))  # (as read from a file)
    assert t2.step_count == 2
    l1, l2 = float(t1.step(*dev)[0]), float(t2.step(*dev)[0])  # (dropout on: the same seeds in both passes of both trainers)
    print(f"next step: {l1:.9f} against {l2:.9f} (diff {abs(l1 - l2):.3e})")
    assert abs(l1 - l2) <= LOSS_BOUND
    # two runs of the same step from the same bits differ by the order of the float atomics that sum the CNN and GRU-bias
    # gradients, which Adam turns into a fraction of lr: the bounds tests/test_gpu_model.py holds two such runs to
    worst = {k: float((v - m2.state_dict()[k]).abs().max()) for k, v in m1.state_dict().items()}
    print(f"weights after it: max |diff| {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    assert all(d <= (6.1e-4 if k == "pool.score.bias" else 2e-5) for k, d in worst.items()), worst
    for other in (dict(), dict(sam_rho=0.1, sam_adaptive=True), dict(sam_rho=RHO)):
        with pytest.raises(ValueError, match="sam_rho"):
            sam_trainer(ss, new_model(ss, sd), **other).load_state_dict(state)
    with pytest.raises(ValueError, match="sam_rho"):
        t2.load_state_dict(plain.state_dict())


def test_resumed_fit_with_sam_equals_the_uninterrupted_one(ss, tmp_path):
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    d = tmp_path
    clips = write_clips(str(d / "clips_npz"), WORDS)
    kw = dict(FIT, epochs=2, log=lambda *a, **k: None)
    hu, h1, h2 = [], [], []
    Hn.fit_sam(clips, str(d / "u.pt"), RHO, state_path=str(d / "u_state.pt"), history=hu, **kw)
    S = str(d / "r_state.pt")
    Hn.fit_sam(clips, str(d / "r.pt"), RHO, state_path=S, history=h1, **dict(kw, epochs=1))
    Hn.fit_calibrated(clips, str(d / "r.pt"), sam_rho=RHO, state_path=S, resume=True, history=h2, **kw)  # (fit_sam, then the temperature)
    assert [h["epoch"] for h in hu] == [1, 2] and [h["epoch"] for h in h1] == [1] and [h["epoch"] for h in h2] == [2]
    for a, b in zip(hu, h1 + h2):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {a['epoch']} {key}: uninterrupted {a[key]:.9f} resumed {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
    for a, b in zip(hu, h1 + h2):
        assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
    state = Ck.load_train_state(S)
    assert state["fingerprint"]["sam_rho"] == RHO and state["fingerprint"]["sam_adaptive"] is False
    assert state["trainer"]["sam_rho"] == RHO and state["trainer"]["step_count"] == 6
    with pytest.raises(ValueError, match="sam_"):  # a run without SAM, or with another radius, cannot resume it
        Hn.fit(clips, str(d / "never.pt"), state_path=S, resume=True, **dict(kw, epochs=3))
    with pytest.raises(ValueError, match="sam_rho"):
        Hn.fit_sam(clips, str(d / "never.pt"), 0.1, state_path=S, resume=True, **dict(kw, epochs=3))
    with pytest.raises(TypeError):  # (a name fit does not have)
        Hn.fit_sam(clips, str(d / "never.pt"), RHO, no_such_argument=1)


# ------------------------------------------------------------------------------------------------------------ data parallel
def test_one_rank_rccl_sam_step_equals_single_process(ss, tmp_path):
    """A FRESH child process (torch.distributed.run, one rank) joins an "nccl" (= RCCL) group and takes two SAM steps with
    ``always_allreduce=True``: two all-reduces of the bucket per step, and the single-process SAM step's weights to the bounds
    tests/test_gpu_model.py holds the plain one-rank step to."""
    import socket
    import subprocess
    import sys

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "child.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "_sam_nccl_child.py"), out],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out, map_location="cpu", weights_only=False)
    assert got["backend"] == "nccl" and got["world"] == 1
    assert got["all_reduces"] == [got["numel"]] * 4  # two per step, each the whole bucket
    B, T = 16, 9
    sd = W.make_state_dict(21, 84, 5, True)
    X, Lh, R, y = W.make_inputs(21, B, T, 84, 5, (64, 64))
    m = ss.BiGRUClassifier(84, 5, use_roi=True)
    m.load_state_dict(sd)
    m.cuda().train()
    tr = sam_trainer(ss, m, dropout=True, sam_rho=RHO)
    losses = [float(tr.step(X.cuda(), Lh.cuda(), R.cuda(), y.cuda())[0]) for _ in range(2)]
    print(f"losses {losses} against the child's {got['losses']}")
    assert abs(losses[0] - got["losses"][0]) < 1e-6 and abs(losses[1] - got["losses"][1]) < 1e-5, (losses, got["losses"])
    for k, v in m.state_dict().items():
        atol = 6.1e-4 if k == "pool.score.bias" else 2e-5
        assert float((v.cpu() - got["sd"][k]).abs().max()) <= atol, k
