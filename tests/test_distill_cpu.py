"""CPU: knowledge distillation away from the device -- tests/distill_ref.py against float64 torch autograd, the two new symbols
(header, library, ``_lib.SIGNATURES``, the ABI version, their host-side refusals), the host refusals of ``fit`` and ``Trainer``, and
the run fingerprint.  No device is touched."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_loss(x, t, y, tau, alpha, eps, w=None, y_b=None, lam=1.0):
    """(1 - alpha) CE(weight=, label_smoothing=, reduction="sum") / norm + alpha tau^2 kl_div(reduction="sum") / B, float64; with a
    second label the hard term is lam CE(y) + (1 - lam) CE(y_b) over the one normaliser of y."""
    B = x.shape[0]
    norm = float(B) if w is None else float(w[y].sum())
    ce = lambda lab: F.cross_entropy(x, lab, weight=w, label_smoothing=eps, reduction="sum") / norm  # noqa: E731
    hard = ce(y) if y_b is None else lam * ce(y) + (1.0 - lam) * ce(y_b)
    soft = F.kl_div(F.log_softmax(x / tau, 1), F.softmax(t / tau, 1), reduction="sum") / B
    return (1.0 - alpha) * hard + alpha * tau * tau * soft


@pytest.mark.parametrize("C", [1, 2, 10, 65, 100])
def test_restatement_equals_torch_autograd(C):
    B = 7
    g = torch.Generator().manual_seed(C)
    z, t = torch.randn(B, C, generator=g, dtype=torch.float64) * 3, torch.randn(B, C, generator=g, dtype=torch.float64) * 3
    y, y_b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    w = torch.rand(C, generator=g, dtype=torch.float64) * 2.8 + 0.2
    worst = 0.0
    for tau, alpha, weighted, mix in itertools.product((0.5, 1.0, 2.0, 4.0), (0.0, 0.3, 1.0), (False, True), (False, True)):
        x = z.clone().requires_grad_(True)
        ww, yb, lam = (w if weighted else None), (y_b if mix else None), (0.3125 if mix else 1.0)
        loss = torch_loss(x, t, y, tau, alpha, 0.05, ww, yb, lam)
        loss.backward()
        got = D.evaluate(z.numpy(), t.numpy(), y.numpy(), tau, alpha, 0.05, float(B), None if ww is None else ww.numpy(),
                         None if ww is None else float(ww[y].sum()), None if yb is None else yb.numpy(), lam)
        e_loss = abs(got["loss"] - float(loss.detach()))
        e_grad = float(np.abs(got["grad"] - x.grad.numpy()).max())
        worst = max(worst, e_loss, e_grad)
        assert e_loss <= 1e-13 * max(1.0, abs(float(loss.detach()))), (tau, alpha, weighted, mix)
        assert e_grad <= 1e-13, (tau, alpha, weighted, mix)
        assert got["correct"] == int((z.argmax(1) == y).sum())
        assert got["loss_bound"] > 0 and bool((got["grad_bound"] > 0).all())
    print(f"C={C}: worst difference from float64 autograd {worst:.3e}")


def test_counting_rule_and_the_two_normalisers():
    B, C = 6, 5
    g = np.random.default_rng(3)
    z, t = g.normal(size=(B, C)) * 3, g.normal(size=(B, C)) * 3
    y, y_b, w = g.integers(0, C, B), g.integers(0, C, B), g.random(C) + 0.5
    bad_y, bad_b = y.copy(), y_b.copy()
    bad_y[1], bad_b[4] = -1, C
    # plain: the labels are not looked at (the caller vouches); weighted: y alone; second labels: both
    assert D.counts(y, C).all() and D.counts(bad_y, C, weighted=True).tolist() == [True, False] + [True] * 4
    assert D.counts(bad_y, C, bad_b).tolist() == [True, False, True, True, False, True]
    keep = [0, 2, 3, 5]
    full = D.evaluate(z, t, bad_y, 2.0, 0.3, 0.05, 8.0, w, 5.5, bad_b, 0.25)
    part = D.evaluate(z[keep], t[keep], y[keep], 2.0, 0.3, 0.05, 8.0, w, 5.5, y_b[keep], 0.25)
    assert not full["grad"][[1, 4]].any() and np.allclose(full["grad"][keep], part["grad"], rtol=0, atol=1e-15)
    assert abs(full["loss"] - part["loss"]) < 1e-14
    # the hard term over den, the soft term over denom: alpha picks one of them out
    for alpha, scales in ((0.0, "den"), (1.0, "denom")):
        a = D.evaluate(z, t, y, 2.0, alpha, 0.05, 8.0, w, 5.5)
        b = D.evaluate(z, t, y, 2.0, alpha, 0.05, 8.0 * (2 if scales == "denom" else 1), w, 5.5 * (2 if scales == "den" else 1))
        c = D.evaluate(z, t, y, 2.0, alpha, 0.05, 8.0 * (1 if scales == "denom" else 2), w, 5.5 * (1 if scales == "den" else 2))
        assert np.allclose(a["grad"], 2 * b["grad"], rtol=1e-14) and np.allclose(a["loss"], 2 * b["loss"], rtol=1e-14)
        assert np.array_equal(a["grad"], c["grad"]) and a["loss"] == c["loss"]
    # a teacher that agrees: no soft term; a wide row at a low temperature: finite, bound included
    same = D.evaluate(z, z, y, 0.5, 1.0, 0.05, 8.0)
    assert same["loss"] == 0.0 and not same["grad"].any()
    wide = z.copy()
    wide[0, 0], wide[0, 1] = 100.0, -100.0
    r = D.evaluate(wide, t, y, 0.5, 1.0, 0.0, 8.0)
    assert np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all() and np.isfinite(r["grad_bound"]).all()


def test_symbols_signatures_abi_and_host_refusals():
    from silent_speech_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    assert "int ss_tail_fwd_kd(" in hdr and "int ss_ce_ls_kd_fwd_bwd(" in hdr
    S = _lib.SIGNATURES
    assert len(S["ss_tail_fwd_kd"]) == len(S["ss_tail_fwd_mix"]) + 4 and len(S["ss_ce_ls_kd_fwd_bwd"]) == len(S["ss_ce_ls_mix_fwd_bwd"]) + 4
    assert S["ss_tail_fwd_kd"][:-5] == S["ss_tail_fwd_mix"][:-1] and S["ss_ce_ls_kd_fwd_bwd"][:-5] == S["ss_ce_ls_mix_fwd_bwd"][:-1]
    lib = _lib.load()
    assert lib.ss_abi_version() == 3
    assert lib.ss_tail_fwd_kd and lib.ss_ce_ls_kd_fwd_bwd
    # every refusal returns before a launch: the pointers are never dereferenced on the host
    buf = (ctypes.c_float * 64)()
    one = ctypes.cast(buf, ctypes.c_void_p).value

    def ce(t=one, ld_t=4, alpha=0.5, tau=2.0, denom=2.0, y_b=None, lam=None, w=None, den=None):
        return lib.ss_ce_ls_kd_fwd_bwd(one, one, y_b, lam, 2, 4, 0.05, denom, w, den, one, one, one, t, ld_t, alpha, tau, None)

    def tail(t=one, ld_t=4, alpha=0.5, tau=2.0, denom=2.0, y_b=None, lam=None, w=None, den=None):
        return lib.ss_tail_fwd_kd(*[one] * 11, y_b, lam, 2, 3, 8, 4, 4, 1e-5, 0.0, 0, 0, 0.05, denom, w, den, *[one] * 10, t, ld_t, alpha,
                                  tau, None)

    for bad in (dict(t=None), dict(ld_t=3), dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(tau=0.0), dict(tau=-1.0),
                dict(tau=float("inf")), dict(tau=float("nan")), dict(denom=0.0), dict(denom=0.0, w=one, den=one), dict(y_b=one),
                dict(lam=one), dict(w=one), dict(den=one)):
        assert ce(**bad) == -1, bad
        assert tail(**bad) == -1, bad
    assert not any(buf)


def test_fit_and_trainer_refuse_on_the_host(tmp_path, monkeypatch):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    def never(*a, **k):
        raise AssertionError("fit went past its argument checks")

    monkeypatch.setattr(Hn, "scan_clips", never)
    monkeypatch.setattr(Hn, "DeviceClipStore", never)
    out, teacher = str(tmp_path / "o.pt"), str(tmp_path / "teacher.pt")
    fit = lambda **kw: Hn.fit(str(tmp_path), out, **{"plan": "device", "distill_from": teacher, **kw})  # noqa: E731
    for alpha in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="distill_alpha"):
            fit(distill_alpha=alpha)
    for tau in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="distill_temperature"):
            fit(distill_temperature=tau)
    with pytest.raises(ValueError, match="plan='device'"):
        fit(plan="host")
    with pytest.raises(ValueError, match="freeze_cnn"):
        fit(freeze_cnn=True, init_from="a.pt")
    with pytest.raises(TypeError, match="distill_from"):
        fit(distill_from=3)
    # the trainer's constructor: host code too (the model is on the CPU and is never asked to move)
    m = ss.BiGRUClassifier(84, 5)
    with pytest.raises(ValueError, match="distill_alpha"):
        ss.Trainer(m, distill_alpha=2.0)
    with pytest.raises(ValueError, match="distill_temperature"):
        ss.Trainer(m, distill_temperature=0.0)
    from silent_speech_amd.train import check_distill

    assert check_distill(0.5, 2.0) == (0.5, 2.0) and check_distill(0, 1) == (0.0, 1.0) and check_distill(1.0, 1e-3) == (1.0, 1e-3)
    # a teacher that does not fit the run: named by field
    for kw, field in ((dict(x_dim=83), "x_dim"), (dict(use_roi=False), "use_roi"), (dict(labels=["b", "a"]), "labels"),
                      (dict(labels=None, num_classes=3), "num_classes")):
        args = dict(x_dim=84, use_roi=True, num_classes=2, labels=["a", "b"], clip_x_dim=84, run_use_roi=True, clip_labels=["a", "b"])
        Hn.check_teacher(**args)
        with pytest.raises(ValueError, match=field):
            Hn.check_teacher(**dict(args, **kw))


FIELDS = dict(seed=42, batch_size=16, world_size=1, max_t=90, lr=3e-4, labels=["a", "b"], x_dim=84, use_roi=True, n_train=10, n_val=2,
              class_weights=None, augment_policy=None, ema_decay=None)


def test_fingerprint():
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    # without distill_from: the parent's fingerprint, field for field, whatever the other two say
    assert Hn.run_fingerprint(**FIELDS) == FIELDS and set(Hn.run_fingerprint(**FIELDS)) == set(Ck.FINGERPRINT_FIELDS)
    assert Hn.run_fingerprint(**FIELDS, distill_from=None, distill_alpha=0.9, distill_temperature=7.0) == FIELDS
    sha = "ab" * 32
    kd = Hn.run_fingerprint(**FIELDS, distill_from=sha, distill_alpha=0.5, distill_temperature=2.0)
    assert kd == dict(FIELDS, distill_from=sha, distill_alpha=0.5, distill_temperature=2.0)
    assert Hn.run_fingerprint(**FIELDS, distill_from="module")["distill_from"] == "module"
    assert Ck.fingerprint_difference(kd, kd) is None
    assert Ck.fingerprint_difference(kd, dict(kd, distill_alpha=0.25)) == "distill_alpha"
    assert Ck.fingerprint_difference(kd, dict(kd, distill_temperature=4.0)) == "distill_temperature"
    assert Ck.fingerprint_difference(kd, dict(kd, distill_from="cd" * 32)) == "distill_from"
    assert Ck.fingerprint_difference(FIELDS, kd) in ("distill_alpha", "distill_from", "distill_temperature")
