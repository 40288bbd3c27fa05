"""GPU: knowledge distillation -- the loss row with a teacher's soft targets (ss_ce_ls_kd_fwd_bwd, ss_tail_fwd_kd) against
tests/distill_ref.py within its derived float32 bound, its bit-exact identities (alpha = 0 is the loss without a teacher; a teacher
that agrees adds nothing), the refusals, ``Trainer.step(teacher_logits=)`` against the CPU oracle under autograd, the launch list of
such a step, and ``fit(distill_from=)`` with a resumed run.  Figures are printed before they are compared."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import distill_ref as D  # noqa: E402
import launch_trace as LT  # noqa: E402
import weights as W  # noqa: E402
from gpu_support import L, STASH, WORDS, cuda, make_weights, ss, tail_call, write_clips  # noqa: E402, F401
from oracle import model_ref as MR  # noqa: E402
from oracle import model_ref_bf16 as MB  # noqa: E402

U = 2.0 ** -24
SS_ERR_ARG = -1
EPS = float(np.float32(0.05))  # the smoothing as the kernels see it
LOSS_BOUND = 10 * 9.781275e-08  # tests/test_gpu_ema_resume.py: a resumed epoch against the uninterrupted one


# ------------------------------------------------------------------------------------------------ 1. the row kernel
def ce_kd(L, lg_d, t_d, ld_t, y_d, alpha, tau, eps, denom, yb_d=None, lam_d=None, w_d=None, den_d=None, fill=9.0, status=False):
    B, C = lg_d.shape
    d = torch.full((B, C), fill, device="cuda")
    loss, correct = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    args = (lg_d.data_ptr(), y_d.data_ptr(), L.ptr(yb_d), L.ptr(lam_d), B, C, eps, float(denom), L.ptr(w_d), L.ptr(den_d),
            d.data_ptr(), loss.data_ptr(), correct.data_ptr(), L.ptr(t_d), ld_t, alpha, tau, L.stream())
    if status:
        st = L.load().ss_ce_ls_kd_fwd_bwd(*args)
        torch.cuda.synchronize()
        return st, d, loss, correct
    L.call("ss_ce_ls_kd_fwd_bwd", *args)
    torch.cuda.synchronize()
    return d, loss, correct


def ce_old(L, lg_d, y_d, eps, denom, yb_d=None, lam_d=None, w_d=None, den_d=None):
    """The matching entry point without a teacher: plain, _w, or _mix."""
    B, C = lg_d.shape
    d = torch.full((B, C), 5.0, device="cuda")
    loss, correct = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    out = (d.data_ptr(), loss.data_ptr(), correct.data_ptr(), L.stream())
    if yb_d is not None:
        L.call("ss_ce_ls_mix_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), yb_d.data_ptr(), lam_d.data_ptr(), B, C, eps, float(denom),
               L.ptr(w_d), L.ptr(den_d), *out)
    elif w_d is not None:
        L.call("ss_ce_ls_w_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, w_d.data_ptr(), den_d.data_ptr(), *out)
    else:
        L.call("ss_ce_ls_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, float(denom), *out)
    torch.cuda.synchronize()
    return d, loss, correct


def padded(t, ld):
    """(B, C) -> a (B, ld) device buffer holding it in its leading columns, the rest NaN (never to be read)."""
    buf = torch.full((t.shape[0], ld), float("nan"))
    buf[:, :t.shape[1]] = t
    return cuda(buf)


def check_against_ref(tag, d, loss, correct, ref, worst):
    e_loss = abs(float(loss) - ref["loss"]) / ref["loss_bound"]
    assert ref["grad_bound"].min() > 0
    e_grad = float((np.abs(d.double().cpu().numpy() - ref["grad"]) / ref["grad_bound"]).max())
    worst[0], worst[1] = max(worst[0], e_loss), max(worst[1], e_grad)
    if e_loss > 1.0 or e_grad > 1.0:
        print(f"{tag}: loss err / bound {e_loss:.3f}, d_logits err / bound {e_grad:.3f}")
    assert bool(torch.isfinite(d).all()) and np.isfinite(float(loss))
    assert e_loss <= 1.0, (tag, e_loss)
    assert e_grad <= 1.0, (tag, e_grad)
    assert int(correct) == ref["correct"], tag


def row_case(B, C, seed_shift=0):
    g = torch.Generator().manual_seed(1000 * B + C + seed_shift)
    lg, tl = torch.randn(B, C, generator=g) * 3, torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    y_b = y[torch.randperm(B, generator=g)] if B > 1 else (y + 1) % C
    return g, lg, tl, y, y_b


@pytest.mark.parametrize("C", [1, 2, 10, 64, 65, 100, 129])
@pytest.mark.parametrize("B", [1, 16, 65])
def test_kd_row_kernel(L, B, C):
    """ss_ce_ls_kd_fwd_bwd against tests/distill_ref.py within its derived bound: one lane, a partial wave, a second wave; tight and
    padded teacher rows; every weighted x mix combination."""
    g, lg, tl, y, y_b = row_case(B, C)
    w = make_weights(g, C)
    lg_d, y_d, yb_d, w_d = cuda(lg), cuda(y), cuda(y_b), cuda(w)
    den_d = torch.empty(1, device="cuda")
    L.call("ss_class_weight_sum", y_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
    lam = 77 / 256.0
    lam_d = torch.tensor([lam], device="cuda")
    teachers = {C: cuda(tl), C + 3: padded(tl, C + 3)}
    worst = [0.0, 0.0]
    for ld_t, tau, alpha, eps, weighted, mix in itertools.product((C, C + 3), (0.5, 1.0, 4.0), (0.25, 1.0), (0.0, EPS), (False, True),
                                                                  (False, True)):
        kw = dict(yb_d=yb_d if mix else None, lam_d=lam_d if mix else None, w_d=w_d if weighted else None,
                  den_d=den_d if weighted else None)
        d, loss, correct = ce_kd(L, lg_d, teachers[ld_t], ld_t, y_d, alpha, tau, eps, B, **kw)
        ref = D.evaluate(lg.numpy(), tl.numpy(), y.numpy(), tau, alpha, eps, float(B), w.numpy() if weighted else None,
                         float(den_d) if weighted else None, y_b.numpy() if mix else None, lam if mix else 1.0)
        check_against_ref(f"B={B} C={C} ld_t={ld_t} tau={tau} alpha={alpha} eps={eps} w={weighted} mix={mix}", d, loss, correct, ref, worst)
    print(f"B={B} C={C}: largest loss err / bound {worst[0]:.3f}, largest d_logits err / bound {worst[1]:.3f}")


def test_kd_row_with_a_span_of_200_at_a_low_temperature(L):
    """A row whose logits span 200 (and a teacher row that does) at tau = 0.5: exponents down to -400, probabilities that underflow
    to 0 -- every output finite and inside the bound."""
    B, C = 16, 10
    g, lg, tl, y, _ = row_case(B, C, seed_shift=7)
    lg[3, 0], lg[3, 1] = 100.0, -100.0
    tl[5, 2], tl[5, 7] = -100.0, 100.0
    lg[6, 4], tl[6, 4] = 120.0, -80.0
    worst = [0.0, 0.0]
    for alpha in (0.25, 1.0):
        d, loss, correct = ce_kd(L, cuda(lg), cuda(tl), C, cuda(y), alpha, 0.5, EPS, B)
        ref = D.evaluate(lg.numpy(), tl.numpy(), y.numpy(), 0.5, alpha, EPS, float(B))
        check_against_ref(f"span 200, alpha={alpha}", d, loss, correct, ref, worst)
    print(f"span 200 at tau 0.5: largest loss err / bound {worst[0]:.3f}, largest d_logits err / bound {worst[1]:.3f}")


# ------------------------------------------------------------------------------------------------ 2. bit-exact identities
@pytest.mark.parametrize("C", [1, 2, 10, 64, 65, 100, 129])
@pytest.mark.parametrize("B", [1, 16, 65])
def test_kd_row_identities(L, B, C):
    g, lg, tl, y, y_b = row_case(B, C)
    w = make_weights(g, C)
    lg_d, tl_d, y_d, yb_d, w_d = cuda(lg), cuda(tl), cuda(y), cuda(y_b), cuda(w)
    den_d = torch.empty(1, device="cuda")
    L.call("ss_class_weight_sum", y_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
    lam_d = torch.tensor([77 / 256.0], device="cuda")
    combos = (dict(), dict(w_d=w_d, den_d=den_d), dict(yb_d=yb_d, lam_d=lam_d), dict(yb_d=yb_d, lam_d=lam_d, w_d=w_d, den_d=den_d))
    for kw, tau, eps in itertools.product(combos, (0.5, 4.0), (0.0, EPS)):
        # alpha = 0: the bits of the entry point without a teacher
        d, loss, correct = ce_kd(L, lg_d, tl_d, C, y_d, 0.0, tau, eps, B, **kw)
        d1, loss1, correct1 = ce_old(L, lg_d, y_d, eps, B, **kw)
        assert torch.equal(d, d1), (sorted(kw), tau, eps, float((d - d1).abs().max()))
        assert int(correct) == int(correct1)
        if B <= 64:  # one wave: one atomic into a zero
            assert loss.cpu().numpy().tobytes() == loss1.cpu().numpy().tobytes(), (sorted(kw), tau, eps)
        else:
            assert abs(float(loss) - float(loss1)) <= (B - 1) * U * abs(float(loss1))
        # alpha = 1 and a teacher that agrees: nothing at all
        d, loss, _ = ce_kd(L, lg_d, lg_d, C, y_d, 1.0, tau, eps, B, **kw)
        assert not bool(d.any()) and float(loss) == 0.0, (sorted(kw), tau, eps, float(d.abs().max()), float(loss))
    # a label outside the classes, under weights or second labels: a zero row that adds nothing, teacher or not
    if B >= 16:
        ya, yb = y.clone(), y_b.clone()
        ya[3], yb[5], yb[7] = -1, C, 2 ** 32 + 1
        ya_d, ybad_d = cuda(ya), cuda(yb)
        for kw, gone in ((dict(w_d=w_d, den_d=den_d), [3]), (dict(yb_d=ybad_d, lam_d=lam_d), [3, 5, 7]),
                         (dict(yb_d=ybad_d, lam_d=lam_d, w_d=w_d, den_d=den_d), [3, 5, 7])):
            d, loss, correct = ce_kd(L, lg_d, tl_d, C, ya_d, 0.25, 2.0, EPS, B, **kw)
            mix = "yb_d" in kw
            ref = D.evaluate(lg.numpy(), tl.numpy(), ya.numpy(), 2.0, 0.25, EPS, float(B), w.numpy() if "w_d" in kw else None,
                             float(den_d) if "w_d" in kw else None, yb.numpy() if mix else None, 77 / 256.0 if mix else 1.0)
            assert not bool(d[gone].any()) and not ref["grad"][gone].any()
            keep = [b for b in range(B) if b not in gone]
            err = np.abs(d.double().cpu().numpy() - ref["grad"])[keep] / ref["grad_bound"][keep]
            assert float(err.max()) <= 1.0 and abs(float(loss) - ref["loss"]) <= ref["loss_bound"] and int(correct) == ref["correct"]


# ------------------------------------------------------------------------------------------------ 3. the fused tail
@pytest.mark.parametrize("C", [2, 10, 64, 65, 100, 129])
def test_kd_tail(L, C):
    """ss_tail_fwd_kd at the shape of test_mix_tail: logits and stashes are ss_tail_fwd's bits; d_logits and loss against
    tests/distill_ref.py on the kernel's own logits; alpha = 0 against ss_tail_fwd, _w and _mix; its own logits as the teacher."""
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
    tl = torch.randn(B, C, generator=g) * 3
    h_d, len_d, y_d, yb_d, w_d = cuda(h), cuda(torch.tensor(lengths, dtype=torch.int32)), cuda(y), cuda(y_b), cuda(w)
    den_d = torch.empty(1, device="cuda")
    L.call("ss_class_weight_sum", y_d.data_ptr(), B, w_d.data_ptr(), C, den_d.data_ptr(), L.stream())
    dims = (B, T, 2 * Hd, 128, C)
    lam = 0.3125
    lam_d = torch.tensor([lam], device="cuda")
    tl_d, tl_pad = cuda(tl), padded(tl, C + 3)
    plain = tail_call(L, "ss_tail_fwd", P, h_d, len_d, y_d, dims, EPS, (float(B),))
    logits = plain["logits"].cpu()
    old = {(False, False): plain,
           (True, False): tail_call(L, "ss_tail_fwd_w", P, h_d, len_d, y_d, dims, EPS, (w_d.data_ptr(), den_d.data_ptr())),
           (False, True): tail_call(L, "ss_tail_fwd_mix", P, h_d, len_d, y_d, dims, EPS, (float(B), None, None),
                                    (yb_d.data_ptr(), lam_d.data_ptr())),
           (True, True): tail_call(L, "ss_tail_fwd_mix", P, h_d, len_d, y_d, dims, EPS, (1.0, w_d.data_ptr(), den_d.data_ptr()),
                                   (yb_d.data_ptr(), lam_d.data_ptr()))}
    worst = [0.0, 0.0]
    for weighted, mix in itertools.product((False, True), (False, True)):
        norm = (float(B), w_d.data_ptr() if weighted else None, den_d.data_ptr() if weighted else None)
        labels = (yb_d.data_ptr(), lam_d.data_ptr()) if mix else (None, None)
        for (t_d, ld_t), tau, alpha in itertools.product(((tl_d, C), (tl_pad, C + 3)), (0.5, 4.0), (0.25, 1.0)):
            out = tail_call(L, "ss_tail_fwd_kd", P, h_d, len_d, y_d, dims, EPS, norm, labels, (t_d.data_ptr(), ld_t, alpha, tau))
            for k in STASH + ("logits",):
                assert torch.equal(out[k], plain[k]), k
            ref = D.evaluate(logits.numpy(), tl.numpy(), y.numpy(), tau, alpha, EPS, float(B), w.numpy() if weighted else None,
                             float(den_d) if weighted else None, y_b.numpy() if mix else None, lam if mix else 1.0)
            check_against_ref(f"tail C={C} w={weighted} mix={mix} ld_t={ld_t} tau={tau} alpha={alpha}", out["d_logits"], out["loss"],
                              out["correct"], ref, worst)
        # alpha = 0: the tail without a teacher, bit for bit
        new = tail_call(L, "ss_tail_fwd_kd", P, h_d, len_d, y_d, dims, EPS, norm, labels, (tl_d.data_ptr(), C, 0.0, 2.0))
        was = old[(weighted, mix)]
        for k in STASH + ("logits", "d_logits"):
            assert torch.equal(new[k], was[k]), (weighted, mix, k)
        assert int(new["correct"]) == int(was["correct"])
        assert abs(float(new["loss"]) - float(was["loss"])) <= (B - 1) * U * abs(float(was["loss"]))  # (sixteen atomics, any order)
        # its own logits, from the first launch, as the teacher: the soft term is exactly nothing
        same = tail_call(L, "ss_tail_fwd_kd", P, h_d, len_d, y_d, dims, EPS, norm, labels, (plain["logits"].data_ptr(), C, 1.0, 0.5))
        assert not bool(same["d_logits"].any()) and float(same["loss"]) == 0.0
    print(f"tail C={C}: largest loss err / bound {worst[0]:.3f}, largest d_logits err / bound {worst[1]:.3f}")


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_kd_entry_points_refuse_and_write_nothing(L):
    B, C = 16, 10
    g, lg, tl, y, _ = row_case(B, C)
    lg_d, tl_d, y_d = cuda(lg), cuda(tl), cuda(y)
    T, Hd = 5, 192
    P = {k: cuda(v) for k, v in W.make_state_dict(3, 84, C, False, hidden=Hd).items() if k.startswith(("pool.", "head."))}
    h_d, len_d = cuda(torch.randn(B, T, 2 * Hd, generator=g)), torch.full((B,), T, dtype=torch.int32, device="cuda")
    dims = (B, T, 2 * Hd, 128, C)
    for t_d, ld_t, alpha, tau in ((None, C, 0.5, 2.0), (tl_d, C - 1, 0.5, 2.0), (tl_d, C, 1.5, 2.0), (tl_d, C, 0.5, 0.0),
                                  (tl_d, C, 0.5, float("inf"))):
        st, d, loss, correct = ce_kd(L, lg_d, t_d, ld_t, y_d, alpha, tau, EPS, B, fill=7.0, status=True)
        assert st == SS_ERR_ARG, (ld_t, alpha, tau)
        assert bool((d == 7.0).all()) and float(loss) == 0.0 and int(correct) == 0
        out = tail_call(L, "ss_tail_fwd_kd", P, h_d, len_d, y_d, dims, EPS, (float(B), None, None), (None, None),
                        (L.ptr(t_d), ld_t, alpha, tau), status=True, fill=7.0)
        assert out["status"] == SS_ERR_ARG, (ld_t, alpha, tau)
        assert all(bool((out[k] == 7.0).all()) for k in STASH + ("logits", "d_logits")) and float(out["loss"]) == 0.0
        assert int(out["correct"]) == 0
    st, d, loss, _ = ce_kd(L, lg_d, tl_d, C, y_d, 0.5, 2.0, EPS, 0.0, fill=7.0, status=True)  # (the soft term's normaliser)
    assert st == SS_ERR_ARG and bool((d == 7.0).all()) and float(loss) == 0.0


# ------------------------------------------------------------------------------------------------ 5. Trainer.step(teacher_logits=)
def kd_torch_loss(logits, t, y, tau, alpha, eps=0.05, w=None, y_b=None, lam=1.0):
    """The loss the issue states, on torch tensors (tests/test_distill_cpu.py::torch_loss)."""
    B = logits.shape[0]
    norm = float(B) if w is None else float(w[y].sum())
    ce = lambda lab: F.cross_entropy(logits, lab, weight=w, label_smoothing=eps, reduction="sum") / norm  # noqa: E731
    hard = ce(y) if y_b is None else lam * ce(y) + (1.0 - lam) * ce(y_b)
    soft = F.kl_div(F.log_softmax(logits / tau, 1), F.softmax(t / tau, 1), reduction="sum") / B
    return (1.0 - alpha) * hard + alpha * tau * tau * soft


@pytest.mark.parametrize("full", [False, True], ids=["plain", "weights_and_mix"])
@pytest.mark.parametrize("name,hw", [("landmarks", None), ("roi32", (32, 32))])
def test_trainer_step_with_teacher_logits_matches_the_oracle(ss, name, hw, full):
    """Dropout off, B = 16, T = 12, C = 10: loss and every gradient tensor of ``Trainer.step(teacher_logits=)`` against
    oracle/model_ref.py under autograd with the torch loss on random teacher logits; once plain, once with class weights and
    ``mix=``.  Bounds of the existing trainer tests: loss 3e-6 max(1, |ref|), gradients 2e-5 max|ref| + 1e-8 + 1e-4 |ref|."""
    B, T, C, alpha, tau = 16, 12, 10, 0.5, 2.0
    lam = 77 / 256.0
    sd = W.make_state_dict(11, 84, C, hw is not None)
    X, Lh, R, y = W.make_inputs(5, B, T, 84, C, hw, zero_padding=True)
    g = torch.Generator().manual_seed(17)
    tl = torch.randn(B, C, generator=g) * 3
    y_b = y[torch.randperm(B, generator=g)]
    w = make_weights(g, C) if full else None
    m = ss.BiGRUClassifier(84, C, use_roi=hw is not None)
    m.load_state_dict(sd)
    m.cuda().eval()
    tr = ss.Trainer(m, dropout=False, class_weights=None if w is None else w.numpy())
    assert (tr.distill_alpha, tr.distill_temperature) == (alpha, tau)  # the defaults
    Xd, Rd, Ld, yd, tld = cuda(X), None if R is None else cuda(R), cuda(Lh), cuda(y), cuda(tl)
    mix = (cuda(y_b), torch.tensor([lam], device="cuda")) if full else None
    loss, correct = tr.step(Xd, Ld, Rd, yd, mix=mix, teacher_logits=tld)
    torch.cuda.synchronize()
    bucket = m.flat_grads.clone()
    leaves = {k_: v.detach().clone().requires_grad_(True) for k_, v in sd.items()}
    logits = MR.forward(leaves, X, Lh, R)
    loss_ref = kd_torch_loss(logits, tl, y, tau, alpha, 0.05, w, y_b if full else None, lam if full else 1.0)
    grads = dict(zip(leaves, torch.autograd.grad(loss_ref, list(leaves.values()))))
    loss_ref, logits = loss_ref.detach(), logits.detach()
    print(f"{name} full={full}: step loss {float(loss):.7f}, oracle {float(loss_ref):.7f}, diff {abs(float(loss) - float(loss_ref)):.3e}")
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


def test_trainer_alpha_zero_is_a_step_without_a_teacher_and_the_refusals(ss):
    """alpha = 0: the gradient bucket is within the atomic-order noise of a step without a teacher, that noise being the difference
    of two such steps, measured here.  Then what ``step(teacher_logits=)`` refuses."""
    B, T, C = 16, 12, 10
    sd = W.make_state_dict(11, 84, C, True)
    X, Lh, R, y = W.make_inputs(5, B, T, 84, C, (32, 32), zero_padding=True)
    Xd, Rd, Ld, yd = cuda(X), cuda(R), cuda(Lh), cuda(y)
    tld = cuda(torch.randn(B, C, generator=torch.Generator().manual_seed(3)) * 3)

    def bucket(**kw):
        m = ss.BiGRUClassifier(84, C, use_roi=True)
        m.load_state_dict(sd)
        m.cuda().eval()
        tr = ss.Trainer(m, dropout=False, **({"distill_alpha": 0.0} if kw else {}))
        loss, _ = tr.step(Xd, Ld, Rd, yd, **kw)
        torch.cuda.synchronize()
        return m.flat_grads.double().cpu(), float(loss), m, tr

    a, la, _, _ = bucket()
    b, lb, _, _ = bucket()
    c, _, _, _ = bucket()
    k, lk, m, tr = bucket(teacher_logits=tld)
    noise = max(float((p - q).abs().max()) for p, q in ((a, b), (a, c), (b, c)))
    diff = min(float((k - p).abs().max()) for p in (a, b, c))
    scale = float(a.abs().max())
    print(f"three plain steps differ by at most {noise:.3e} (two losses by {abs(la - lb):.3e}); alpha = 0 against the nearest of them "
          f"{diff:.3e} (losses {abs(lk - la):.3e}); max |gradient| {scale:.3e}")
    # d_logits of the alpha = 0 step are the plain step's bits (test_kd_tail), so its bucket is one more draw of the same atomic
    # orders: it lies as near to one of three plain draws as they lie to each other, give or take a rounding of the largest entry
    assert diff <= noise + 2 * U * scale
    assert abs(lk - la) <= (B - 1) * U * abs(la)
    with pytest.raises(ValueError, match="micro_batches"):
        ss.Trainer(m, dropout=False, micro_batches=2).step(Xd, Ld, Rd, yd, teacher_logits=tld)
    for bad in (tld[:, :C - 1].contiguous(), tld[:B - 1], tld.double(), tld.cpu(), tld.t().contiguous().t()):
        with pytest.raises(ValueError, match="teacher_logits"):
            tr.step(Xd, Ld, Rd, yd, teacher_logits=bad)


def test_bf16_engine_step_with_teacher_logits(ss):
    """One distillation step of the bf16 engine at the shape and the distances of test_bf16_engine_step_with_mix: loss within 1e-2
    and gradient norm within 3 % of the oracle's; and the fused tail's own 3e-6 against float64 on the step's logits."""
    C5 = dict(roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96))
    B, T, alpha, tau = 12, 6, 0.5, 2.0
    sd = W.make_state_dict(4, 84, 100, True, **C5)
    X, Lh, R, y = W.make_inputs(4, B, T, 84, 100, (96, 96), zero_padding=True)
    tl = torch.randn(B, 100, generator=torch.Generator().manual_seed(9)) * 3
    m = ss.BiGRUClassifier(84, 100, use_roi=True, precision="bf16", **C5)
    m.load_state_dict(sd)
    m.cuda().eval()
    tr = ss.Trainer(m, dropout=False)
    Xd, Rd = cuda(X), cuda(R)
    loss, correct = tr.step(Xd, cuda(Lh), Rd, cuda(y), teacher_logits=cuda(tl))
    torch.cuda.synchronize()
    logits = m._workspace(Xd, Rd, train=True, slot=0).logits.cpu()
    own = float(kd_torch_loss(logits.double(), tl.double(), y, tau, alpha))
    _, logits_emu, _ = MB.loss_and_grads(sd, X, Lh, R, y)
    emu = float(kd_torch_loss(logits_emu.double(), tl.double(), y, tau, alpha))
    leaves = {k_: v.detach().clone().requires_grad_(True) for k_, v in sd.items()}
    grads = torch.autograd.grad(kd_torch_loss(MR.forward(leaves, X, Lh, R), tl, y, tau, alpha), list(leaves.values()))
    total = float(torch.sqrt(sum((g_.double() ** 2).sum() for g_ in grads)))
    print(f"bf16 distillation step: loss {float(loss):.7f}, float64 on its logits {own:.7f}, bf16 restatement {emu:.7f}; "
          f"gradient norm {float(tr.grad_norm()):.6f}, f32 oracle {total:.6f}")
    assert abs(float(loss) - own) < 3e-6 * max(1.0, abs(own))
    assert abs(float(loss) - emu) < 1e-2
    assert abs(float(tr.grad_norm()) - total) < 3e-2 * total
    assert int(correct) == int((logits.argmax(1) == y).sum())
    m.check_health()


# ------------------------------------------------------------------------------------------------ 6. the launch list
@pytest.mark.parametrize("name", ["f32_roi32", "bf16_three_launch"])
def test_a_step_with_a_teacher_replaces_one_launch(ss, monkeypatch, name):
    kw, B, T, hw, _ = LT.CASES[name]
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    X = torch.randn(B, T, kw["x_dim"], generator=g).to(dev)
    R = torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8).to(dev) if hw else None
    y = torch.randint(0, kw["num_classes"], (B,), generator=g).to(dev)
    tl = torch.randn(B, kw["num_classes"], generator=g).to(dev)
    lengths = torch.tensor([max(1, T - b % 3) for b in range(B)], dtype=torch.int64, device=dev)
    model = ss.BiGRUClassifier(**kw).to(dev).train()
    tr = ss.Trainer(model, dropout=True)
    tr.step(X, lengths, R, y)
    without = LT.traced(monkeypatch, model, lambda: tr.step(X, lengths, R, y))
    with_t = LT.traced(monkeypatch, model, lambda: tr.step(X, lengths, R, y, teacher_logits=tl))
    assert len(without) == len(with_t) and sum(e[1] == "ss_tail_fwd" for e in LT.launches(without)) == 1
    n_arg = None
    for a, b in zip(without, with_t):
        if a[0] == "launch" and a[1] == "ss_tail_fwd":
            assert b[:4] == ["launch", "ss_tail_fwd_kd", "ss_tail_fwd_kd", a[3]]
            n_arg = (len(a[4]), len(b[4]))
            # h ... b4, y | y_b, lam | the dimensions ... the smoothing, denom | cw, den | the outputs | the soft targets
            # (the dropout seed follows the step count: it is the one argument that moves between two steps)
            assert a[4][18] != b[4][20] and isinstance(a[4][18], int)
            a[4][18] = b[4][20] = "seed"
            assert b[4][:11] == a[4][:11] and b[4][11:13] == ["null", "null"] and b[4][13:24] == a[4][11:22]
            assert b[4][24:26] == ["null", "null"] and b[4][26:36] == a[4][22:32]
            assert b[4][36:] == ["ptr", kw["num_classes"], 0.5, 2.0]
        elif a[0] == "launch":  # (the dropout seeds follow the step count: every other argument is the one it was)
            assert a[:4] == b[:4] and len(a[4]) == len(b[4]), (a[1], b[1])
        else:
            assert a == b
    assert n_arg == (32, 40)


# ------------------------------------------------------------------------------------------------ 7. fit
FIT = dict(batch_size=16, patience=5, max_t=24, lr=3e-3, plan="device", log=lambda *a: None)


@pytest.fixture(scope="module")
def runs(ss, tmp_path_factory):
    """A teacher trained for one epoch; then the student distilled from its checkpoint: (a) two epochs uninterrupted, (b) one epoch
    and resumed to two.  Each ``fit`` once."""
    from silent_speech_amd import harness as Hn

    d = tmp_path_factory.mktemp("distill")
    clip_dir = write_clips(str(d / "clips_npz"), WORDS)
    teacher = str(d / "teacher.pt")
    Hn.fit(clip_dir, teacher, epochs=1, **FIT)
    ha, hb1, hb2 = [], [], []
    kd = dict(FIT, distill_from=teacher)
    Hn.fit(clip_dir, str(d / "a.pt"), epochs=2, history=ha, state_path=str(d / "a.state"), **kd)
    Hn.fit(clip_dir, str(d / "b.pt"), epochs=1, history=hb1, state_path=str(d / "b.state"), **kd)
    Hn.fit(clip_dir, str(d / "b.pt"), epochs=2, history=hb2, state_path=str(d / "b.state"), resume=True, **kd)
    return dict(dir=d, clip_dir=clip_dir, teacher=teacher, ha=ha, hb1=hb1, hb2=hb2, kd=kd)


def test_fit_distils_from_a_checkpoint_and_resumes(ss, runs):
    from silent_speech_amd import harness as Hn

    ha, hb2 = runs["ha"], runs["hb2"]
    assert [h["epoch"] for h in ha] == [1, 2] and [h["epoch"] for h in hb2] == [2]
    assert all(np.isfinite(h[key]) for h in ha for key in ("train_loss", "train_acc", "val_loss", "val_acc"))
    assert all(h["train_loss"] > 0 for h in ha)
    model, id_to_label, max_t, use_roi = ss.load_classifier(str(runs["dir"] / "a.pt"))
    assert sorted(id_to_label.values()) == WORDS and max_t == 24 and use_roi and model.cfg.hidden == 192
    a, b = ha[1], hb2[0]
    for key in ("train_loss", "train_acc", "val_loss", "val_acc"):
        print(f"epoch 2 {key}: uninterrupted {a[key]:.9f} resumed {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
    assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
    # the blended loss is what is logged: it is not the loss of the same first epoch without a teacher
    plain = []
    Hn.fit(runs["clip_dir"], str(runs["dir"] / "p.pt"), epochs=1, history=plain, **FIT)
    print(f"epoch 1 train loss: distilled {ha[0]['train_loss']:.6f}, without a teacher {plain[0]['train_loss']:.6f}")
    assert abs(plain[0]["train_loss"] - ha[0]["train_loss"]) > 1e-3
    # the fingerprint: another alpha, another teacher file, no teacher
    out, state = str(runs["dir"] / "b.pt"), str(runs["dir"] / "b.state")
    with pytest.raises(ValueError, match="distill_alpha"):
        Hn.fit(runs["clip_dir"], out, epochs=3, state_path=state, resume=True, **dict(runs["kd"], distill_alpha=0.25))
    with pytest.raises(ValueError, match="distill_"):
        Hn.fit(runs["clip_dir"], out, epochs=3, state_path=state, resume=True, **FIT)


def test_fit_refuses_a_teacher_with_other_labels_and_takes_a_module(ss, runs, tmp_path):
    from silent_speech_amd import harness as Hn

    other_teacher = str(tmp_path / "t.pt")
    ck = torch.load(runs["teacher"], map_location="cpu", weights_only=False)
    ck["labels"] = ["no", "aura", "yes"]
    torch.save(ck, other_teacher)
    with pytest.raises(ValueError, match="labels"):
        Hn.fit(runs["clip_dir"], str(tmp_path / "o.pt"), epochs=1, **dict(FIT, distill_from=other_teacher))
    # a module teacher of another depth; and the fields a module is checked for
    teacher = ss.BiGRUClassifier(20, 3, use_roi=True, gru_layers=3).cuda()
    before = teacher.flat_params.clone()
    history = []
    Hn.fit(runs["clip_dir"], str(tmp_path / "m.pt"), epochs=1, history=history, state_path=str(tmp_path / "m.state"),
           **dict(FIT, distill_from=teacher, distill_alpha=0.75, distill_temperature=4.0))
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and not teacher.training
    assert torch.equal(teacher.flat_params, before)  # never trained
    assert torch.load(str(tmp_path / "m.state"), map_location="cpu", weights_only=False)["fingerprint"]["distill_from"] == "module"
    with pytest.raises(ValueError, match="x_dim"):
        Hn.fit(runs["clip_dir"], str(tmp_path / "o.pt"), epochs=1, **dict(FIT, distill_from=ss.BiGRUClassifier(21, 3, use_roi=True).cuda()))
    with pytest.raises(ValueError, match="use_roi"):
        Hn.fit(runs["clip_dir"], str(tmp_path / "o.pt"), epochs=1, **dict(FIT, distill_from=ss.BiGRUClassifier(20, 3).cuda()))
