"""CPU: the sharpness-aware step's reference (tests/sam_ref.py) against a two-pass SAM written with torch autograd,
``clip_grad_norm_`` and ``torch.optim.Adam`` / ``AdamW``; the host-side refusals of ``Trainer.enable_sam``, ``fit_sam`` and the
three new entry points; the public surface (signatures, docstrings, the run fingerprint).  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import adamw_ref as AR
import flat_ref as FR
import sam_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, RHO = 3e-3, 0.05


# ------------------------------------------------------------------------------------------- sam_ref against torch autograd
class Mlp:
    """A small float64 MLP on a fixed batch, its parameters one flat vector: ``grad(flat)`` is d(loss)/d(flat) by autograd."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.shapes = [(7, 5), (7,), (3, 7), (3,)]
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.n = sum(self.sizes)
        self.x = torch.randn(11, 5, generator=g, dtype=torch.float64)
        self.y = torch.randint(0, 3, (11,), generator=g)
        self.p0 = 0.5 * torch.randn(self.n, generator=g, dtype=torch.float64)

    def loss(self, tensors):
        w1, b1, w2, b2 = tensors
        h = torch.tanh(self.x @ w1.T + b1)
        return torch.nn.functional.cross_entropy(h @ w2.T + b2, self.y, label_smoothing=0.05)

    def split(self, flat):
        return [t.reshape(s) for t, s in zip(torch.split(flat, self.sizes), self.shapes)]

    def grad(self, flat_np):
        flat = torch.from_numpy(np.asarray(flat_np, np.float64).copy()).requires_grad_(True)
        self.loss(self.split(flat)).backward()
        return flat.grad.numpy().copy()


def torch_sam(mlp, rho, adaptive, steps, decoupled_decay):
    """The SAM optimiser's two steps (``first_step``: ``e_w = (w^2 if adaptive else 1) * grad * rho / (grad_norm + 1e-12)`` with
    ``grad_norm = || (|w| if adaptive else 1) * grad ||``; ``second_step``: back to ``w``, the base optimiser on the new gradient)
    around ``clip_grad_norm_(1.0)`` and ``torch.optim.Adam`` (``AdamW`` with a decay on the two matrices) -> flat weights per step."""
    params = [torch.nn.Parameter(t.clone()) for t in mlp.split(mlp.p0)]
    if decoupled_decay:
        opt = torch.optim.AdamW([dict(params=[params[0], params[2]], weight_decay=decoupled_decay),
                                 dict(params=[params[1], params[3]], weight_decay=0.0)], lr=LR)
    else:
        opt = torch.optim.Adam(params, lr=LR)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        mlp.loss(params).backward()
        norm = torch.norm(torch.stack([((p.abs() if adaptive else 1.0) * p.grad).norm(p=2) for p in params]), p=2)
        scale = rho / (norm + 1e-12)
        old = [p.data.clone() for p in params]
        with torch.no_grad():
            for p in params:
                p.add_((p.pow(2) if adaptive else 1.0) * p.grad * scale)
        opt.zero_grad()
        mlp.loss(params).backward()
        with torch.no_grad():
            for p, o in zip(params, old):
                p.copy_(o)
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        out.append(torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy())
    return out


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
@pytest.mark.parametrize("decay", [0.0, 1e-2], ids=["adam", "adamw"])
def test_sam_ref_against_torch_autograd(adaptive, decay):
    mlp = Mlp(3 + adaptive)
    want = torch_sam(mlp, RHO, adaptive, 3, decay)
    p, m, v = mlp.p0.numpy().copy(), np.zeros(mlp.n), np.zeros(mlp.n)
    ends = list(np.cumsum(mlp.sizes))
    plain_p = mlp.p0.numpy().copy()
    for step in range(1, 4):
        if decay:
            def update(p_, g_):
                return AR.adamw_groups_step(p_, g_, m, v, step, ends, [0, 1, 0, 1], [1.0, 1.0], [decay, 0.0], lr=LR)
        else:
            update = SR.adam_update(m, v, np.zeros(mlp.n), step, lr=LR)
        g, e, g2, _ = SR.sam_step(p, mlp.grad, RHO, adaptive, update)
        assert np.isfinite(e).all() and np.isfinite(g2).all()
        if not adaptive:  # the perturbation of plain SAM has length rho
            assert abs(np.sqrt((e * e).sum()) - RHO) <= 1e-9
        err = np.abs(p - want[step - 1]).max()
        print(f"step {step}: max |sam_ref - torch| {err:.3e}")
        assert err <= 1e-12, (step, err)
    # SAM is visible: three plain Adam steps from the same start end elsewhere
    mp_, vp_ = np.zeros(mlp.n), np.zeros(mlp.n)
    for step in range(1, 4):
        SR.adam_update(mp_, vp_, np.zeros(mlp.n), step, lr=LR)(plain_p, mlp.grad(plain_p))
    assert np.abs(plain_p - p).max() > 1e-5


def test_perturb_bound_covers_fma_and_two_roundings():
    """The float32 evaluations a kernel may choose -- the product rounded on its own, or fused into the sum (emulated: float64
    holds the exact product of two float32 numbers) -- both stay inside ``perturb_expected``'s bound."""
    rng = np.random.default_rng(5)
    n = 4099
    w, g = rng.standard_normal(n).astype(np.float32), (0.05 * rng.standard_normal(n)).astype(np.float32)
    f32 = np.float32
    for adaptive in (False, True):
        t = (np.abs(w) * g if adaptive else g).astype(np.float64)
        ssq = f32((t * t).sum())
        for gs in (1.0, 0.25):
            want, bound = SR.perturb_expected(w, g, ssq, RHO, adaptive, gs)
            scale = f32(f32(f32(RHO) * f32(gs)) / f32(f32(np.sqrt(ssq) * f32(gs)) + f32(1e-12)))
            if adaptive:
                a, b = f32(scale * g), f32(w * w)
            else:
                a, b = np.full(n, scale, f32), g
            two = (w + f32(a * b)).astype(f32)
            fma = (w.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32)
            for name, got in (("two roundings", two), ("fma", fma)):
                ratio = (np.abs(got.astype(np.float64) - want) / bound).max()
                print(f"adaptive={adaptive} grad_scale={gs} {name}: largest err / bound {ratio:.3f}")
                assert ratio <= 1.0 and ratio > 0.0
            assert (bound < 1e-5).all()  # (a bound that means something: rho * |g| / s is ~1e-2 here)


# ---------------------------------------------------------------------------------------------------------- host refusals
def test_trainer_and_fit_refuse_on_the_host(tmp_path, monkeypatch):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn
    from silent_speech_amd.train import check_sam_rho

    # enable_sam's refusals are host code in front of its first touch of a device: a Trainer that was never initialised (there is
    # no GPU to build one on) holds nothing but the one field they read
    t = object.__new__(ss.Trainer)
    t.micro_batches = 1
    for bad in (0, 0.0, -0.05, float("nan"), float("inf"), 1e-60, 1e40, "x", None):
        with pytest.raises(ValueError, match="sam_rho"):
            t.enable_sam(bad)
        if bad is not None:
            with pytest.raises(ValueError, match="sam_rho"):
                check_sam_rho(bad)
    t.micro_batches = 2
    with pytest.raises(ValueError, match="micro_batches"):
        t.enable_sam(0.05, True)
    with pytest.raises(TypeError):  # the constructor's signature is what it always was
        ss.Trainer(ss.BiGRUClassifier(84, 5), sam_rho=0.05)
    assert check_sam_rho(None) is None and check_sam_rho(0.05) == 0.05 and check_sam_rho(2) == 2.0

    def never(*a, **k):
        raise AssertionError("fit went past its argument checks")

    monkeypatch.setattr(Hn, "scan_clips", never)
    monkeypatch.setattr(Hn, "DeviceClipStore", never)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="sam_rho"):
            Hn.fit_sam(str(tmp_path), str(tmp_path / "o.pt"), bad, plan="device")
        if bad is not None:  # (fit_calibrated hands its two SAM names to fit_sam)
            with pytest.raises(ValueError, match="sam_rho"):
                Hn.fit_calibrated(str(tmp_path), str(tmp_path / "o.pt"), plan="device", sam_rho=bad, sam_adaptive=True)
    with pytest.raises(TypeError):  # fit_args are fit's names
        Hn.fit_sam(str(tmp_path), str(tmp_path / "o.pt"), 0.05, no_such_argument=1)
    with pytest.raises(TypeError):
        Hn.fit(str(tmp_path), str(tmp_path / "o.pt"), sam_rho=0.05)
    with pytest.raises(ValueError, match="plan='device'"):  # a good rho goes on to fit's own checks
        Hn.fit_sam(str(tmp_path), str(tmp_path / "o.pt"), 0.05, True, plan="host", state_path=str(tmp_path / "s.pt"))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal returns before a launch: the pointers are host memory here and are never dereferenced."""
    from silent_speech_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    for name in ("ss_sumsq_absw_f32", "ss_sam_perturb", "ss_sam_restore_sumsq"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.ss_abi_version() == 3  # additions do not move it
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    n = 256
    p, g, b, s, zf, zi = base, base + 4 * 1024, base + 4 * 2048, base + 4 * 3072, base + 4 * 3080, base + 4 * 3088

    def perturb(p=p, g=g, b=b, n=n, s=s, rho=0.05, zf=zf, nzf=1, zi=zi, nzi=1, adaptive=0):
        return lib.ss_sam_perturb(p, g, b, n, s, 1.0, rho, adaptive, zf, nzf, zi, nzi, None)

    def restore(p=p, b=b, g=g, n=n, s=s):
        return lib.ss_sam_restore_sumsq(p, b, g, n, s, None)

    def absw(w=p, g=g, n=n, s=s):
        return lib.ss_sumsq_absw_f32(w, g, n, s, None)

    shared = (dict(p=None), dict(g=None), dict(b=None), dict(s=None), dict(n=0), dict(n=-4), dict(p=p + 4), dict(g=g + 8), dict(b=b + 4),
              dict(b=p), dict(b=p + 16 * 8), dict(b=p - 16), dict(b=g), dict(b=g + 16 * 63), dict(b=g - 16 * 63))
    for bad in shared:
        assert perturb(**bad) == -1, bad
        assert restore(**bad) == -1, bad
    for bad in (dict(rho=0.0), dict(rho=-0.05), dict(rho=float("nan")), dict(rho=float("inf")), dict(zf=None), dict(zi=None),
                dict(nzf=-1), dict(nzi=257), dict(zf=s), dict(zf=s - 4, nzf=2)):
        for adaptive in (0, 1):
            assert perturb(adaptive=adaptive, **bad) == -1, bad
    for bad in (dict(w=None), dict(g=None), dict(s=None), dict(n=0), dict(n=-1), dict(w=p + 4), dict(g=g + 12)):
        assert absw(**bad) == -1, bad
    assert not any(buf)


# --------------------------------------------------------------------------------------------------------- public surface
def test_signatures_docstrings_and_fingerprint():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    sig = inspect.signature(Hn.fit_sam).parameters
    assert list(sig) == ["clip_dir", "out_path", "sam_rho", "sam_adaptive", "fit_args"] and sig["sam_adaptive"].default is False
    assert sig["sam_rho"].default is inspect.Parameter.empty and sig["fit_args"].kind.name == "VAR_KEYWORD"
    sig = inspect.signature(ss.Trainer.enable_sam).parameters
    assert list(sig) == ["self", "rho", "adaptive"] and sig["adaptive"].default is False
    # the signatures callers and saved scripts depend on did not move (tests/test_interface_cpu.py spells them out)
    for fn in (Hn.fit, ss.Trainer.__init__, Hn.run_fingerprint):
        assert not any(name.startswith("sam_") for name in inspect.signature(fn).parameters)
    for doc in (Hn.fit_sam.__doc__, ss.Trainer.__doc__):
        for word in ("sam_rho", "sam_adaptive", "second forward"):
            assert word in doc, word
    assert "fit_sam" in Hn.fit.__doc__ and "enable_sam" in ss.Trainer.__doc__ and "micro_batches" in ss.Trainer.enable_sam.__doc__
    assert "bf16 resolution" in ss.Trainer.__doc__ and "ss_sam_perturb" in ss.Trainer.__doc__
    assert "sam_rho" in Hn.run_fingerprint.__doc__ and "sam_rho" in ss.Trainer.load_state_dict.__doc__
    # the fingerprint holds the two only when SAM is set: old state files still resume
    fields = dict(seed=42, batch_size=16, world_size=1, max_t=24, lr=3e-4, labels=["aura", "no"], x_dim=20, use_roi=True, n_train=38,
                  n_val=7, class_weights=None, augment_policy=None, ema_decay=None)
    assert Hn.run_fingerprint(**fields) == fields == Hn.sam_fingerprint(Hn.run_fingerprint(**fields), None, True)
    sam = Hn.sam_fingerprint(Hn.run_fingerprint(**fields), 0.05)
    assert sam == dict(fields, sam_rho=0.05, sam_adaptive=False)
    assert Ck.fingerprint_difference(fields, sam) in ("sam_rho", "sam_adaptive") and Ck.fingerprint_difference(sam, sam) is None
    assert Ck.fingerprint_difference(sam, dict(sam, sam_rho=0.1)) == "sam_rho"
    assert Ck.fingerprint_difference(sam, Hn.sam_fingerprint(fields, 0.05, True)) == "sam_adaptive"


def test_sumsq_bound_counts_the_extra_product():
    n = 1027
    assert SR.sumsq_bound(n, 1.0, 2) > SR.sumsq_bound(n, 1.0) == FR.sumsq_chain(n) * FR.U / (1 - FR.sumsq_chain(n) * FR.U)
