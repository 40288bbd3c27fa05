"""CPU: the LAMB restatement (tests/lamb_ref.py) against a per-parameter LAMB written with separate torch parameters,
``clip_grad_norm_`` and ``torch.linalg.vector_norm``, and against ``torch.optim.Adam`` where every tensor is excluded; the ratio's
invariance; the host-side refusals of ``Trainer.enable_lamb``, ``model.param_tensor_segments``, ``load_state_dict``, ``fit_lamb``
and the two entry points; the public surface.  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import flat_ref as FR
import lamb_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_, B1, B2, EPS = 3e-3, 0.9, 0.999, 1e-8
SHAPES = [(7, 5), (7,), (3, 7), (3,), (4, 4)]
SIZES = [int(np.prod(s)) for s in SHAPES]
ENDS = list(np.cumsum(SIZES))


def torch_lamb(p0, grads, groups, scales, decays, adapt, steps):
    """LAMB as its paper writes it, one torch parameter per tensor, float64: ``clip_grad_norm_(1.0)`` over all of them, Adam's
    moments, bias correction, the decay inside the update, ``vector_norm(w) / vector_norm(update)`` where the tensor adapts and both
    norms are positive -> the flat weights after every step, and every step's ratios."""
    params = [torch.nn.Parameter(t.clone()) for t in torch.split(torch.from_numpy(p0.copy()), SIZES)]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    out, ratios = [], []
    for step in range(1, steps + 1):
        for p, g in zip(params, torch.split(torch.from_numpy(grads[step - 1].copy()), SIZES)):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        rs = []
        with torch.no_grad():
            for k, p in enumerate(params):
                m[k].mul_(B1).add_(p.grad, alpha=1 - B1)
                v[k].mul_(B2).addcmul_(p.grad, p.grad, value=1 - B2)
                update = (m[k] / (1 - B1 ** step)) / ((v[k] / (1 - B2 ** step)).sqrt() + EPS) + decays[groups[k]] * p
                w_norm, u_norm = torch.linalg.vector_norm(p), torch.linalg.vector_norm(update)
                r = float(w_norm / u_norm) if adapt[k] and float(w_norm) > 0 and float(u_norm) > 0 else 1.0
                p.add_(update, alpha=-LR_ * scales[groups[k]] * r)
                rs.append(r)
        out.append(torch.cat([p.detach().reshape(-1) for p in params]).numpy().copy())
        ratios.append(rs)
    return out, ratios


def inputs(seed, steps):
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    return 0.5 * rng.standard_normal(n), [rng.standard_normal(n) * (3.0 if k == 1 else 0.02) for k in range(steps)]  # (step 2 clips)


@pytest.mark.parametrize("decay", [0.0, 1e-2], ids=["no_decay", "decay"])
def test_lamb_ref_against_a_per_parameter_torch_lamb(decay):
    p0, grads = inputs(3, 4)
    p0[ENDS[3]:] = 0.0  # (an all-zero tensor: ratio 1)
    groups, scales, decays, adapt = [0, 1, 0, 1, 0], [1.0, 0.5], [decay, 0.0], [1, 0, 1, 0, 1]
    want, want_r = torch_lamb(p0, grads, groups, scales, decays, adapt, 4)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 5):
        total, r = LR.lamb_step(p, grads[step - 1], m, v, step, ENDS, groups, scales, decays, adapt, lr=LR_, beta1=B1, beta2=B2, eps=EPS)
        assert (total > 1.0) == (step == 2)
        np.testing.assert_allclose(r, want_r[step - 1], rtol=1e-12)
        np.testing.assert_allclose(p, want[step - 1], rtol=0, atol=1e-13)
        assert r[1] == r[3] == 1.0 and r[0] != 1.0 and (r[4] == 1.0) == (step == 1)  # (the zero tensor has moved after step 1)


def test_every_tensor_excluded_and_no_decay_is_adam():
    p0, grads = inputs(5, 3)
    params = [torch.nn.Parameter(t.clone()) for t in torch.split(torch.from_numpy(p0.copy()), SIZES)]
    opt = torch.optim.Adam(params, lr=LR_, betas=(B1, B2), eps=EPS)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 4):
        for q, g in zip(params, torch.split(torch.from_numpy(grads[step - 1].copy()), SIZES)):
            q.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        _, r = LR.lamb_step(p, grads[step - 1], m, v, step, ENDS, [0] * 5, [1.0], [0.0], [0] * 5, lr=LR_, beta1=B1, beta2=B2, eps=EPS)
        assert r == [1.0] * 5
        np.testing.assert_allclose(p, torch.cat([q.detach().reshape(-1) for q in params]).numpy(), rtol=0, atol=1e-13)


def test_ratio_is_unchanged_when_a_tensor_and_its_update_are_scaled_together():
    """p and m of one segment times 4 (a power of two: every float32 operation scales exactly), v as it was: u = wd p + bc1 m /
    (sqrt(v) c + eps) is 4 u, so P and U both grow 16-fold and the ratio keeps its value; the other segment is untouched."""
    p, _, m, v = FR.optimiser_case(1024, 9)
    ends, ids, wd = [512, 1024], [0, 1], [1e-2, 0.0]
    (_, _), (_, _), (r0, b0) = LR.norms_expected(p, m, v, 3, ends, ids, wd, [1, 1])
    p4, m4 = p.copy(), m.copy()
    p4[:512] *= 4
    m4[:512] *= 4
    (P4, _), (U4, _), (r4, _) = LR.norms_expected(p4, m4, v, 3, ends, ids, wd, [1, 1])
    (P1, _), (U1, _), _ = LR.norms_expected(p, m, v, 3, ends, ids, wd, [1, 1])
    assert r4[0] == r0[0] and r4[1] == r0[1] and P4[0] == 4 * P1[0] and U4[0] == 4 * U1[0] and P4[1] == P1[1]
    assert 0 < b0[0] < 1e-5 * r0[0]  # (the derived bound is a few ulps, not a tolerance)
    # excluded, all-zero weights, all-zero update: exactly 1, bound 0
    z = np.zeros(512, np.float32)
    for pp, mm, adapt in ((p, m, [0, 1]), (np.concatenate([z, p[512:]]), m, [1, 1]), (p, np.concatenate([z, m[512:]]), [1, 1])):
        _, _, (r, b) = LR.norms_expected(pp, mm, v, 3, ends, ids, [0.0, 0.0], adapt)
        assert r[0] == 1.0 and b[0] == 0.0 and r[1] != 1.0


# ---------------------------------------------------------------------------------------------------------- host refusals
def skeleton(ss, model, **fields):
    """A ``Trainer`` that was never initialised (there is no GPU to build one on) with the fields the host code under test reads."""
    t = object.__new__(ss.Trainer)
    n = model.flat_params.numel()
    base = dict(model=model, param_groups=None, weight_decay=0.0, n_frozen=0, lamb=None, lamb_scratch=None, lamb_norms=None,
                lamb_ratio=None, m=torch.zeros(n), v=torch.zeros(n), ema=None, ema_decay=None, ema_warmup=True, step_count=0,
                betas=(0.9, 0.999), eps=1e-8, lr=3e-4, max_norm=1.0, freeze_cnn=False, table=None, lr_schedule=None, lr_scale=1.0,
                sam_rho=None, sam_adaptive=False, _ema_swapped=False, _bucket_version=model._bucket_version)
    for k, val in dict(base, **fields).items():
        setattr(t, k, val)
    return t


def test_enable_lamb_its_table_and_its_refusals():
    import silent_speech_amd as ss
    from silent_speech_amd.train import check_lamb_exclude

    model = ss.BiGRUClassifier(84, 5, use_roi=True)
    names = [n for n, _ in model.named_parameters()]
    for bad in ("", "*", [""], ["gru.", 3], 5, [None]):
        with pytest.raises(ValueError, match="exclude"):
            skeleton(ss, model).enable_lamb(bad)
        with pytest.raises(ValueError, match="exclude"):
            check_lamb_exclude(bad)
    assert check_lamb_exclude(None) == tuple(ss.no_decay().match) and check_lamb_exclude("gru.") == ("gru.",) and check_lamb_exclude([]) == ()
    t = skeleton(ss, model)
    for fn in (t.trust_ratios, t.lamb_segments):
        with pytest.raises(RuntimeError, match="enable_lamb"):
            fn()
    t.enable_lamb()
    # one segment per tensor, beside param_segments, which still merges neighbours of one group
    ends, ids, seg_names = model.param_tensor_segments()
    lay, total = model._layout()
    assert t.lamb_segments() == names == seg_names and len(names) <= 64 and ends[-1] == total == t.lamb.n
    assert ends == [off for _, off, _, _ in lay[1:]] + [total] and ids == [0] * len(names)
    assert model.param_segments() == ([total], [0], [names])
    assert t.lamb.adapt == [0 if (n.endswith("bias") or n.startswith(("gru.bias_", "head.0."))) else 1 for n in names]
    assert 0 < sum(t.lamb.adapt) < len(names)
    assert t.trust_ratios().tolist() == [1.0] * len(names) and t.lamb_norms.numel() == 2 * len(names)
    assert t.lamb_scratch.dtype == torch.float64 and t.lamb_scratch.numel() == len(names) * min((total // 4 + 255) // 256, 2048) * 2
    ratio = t.lamb_ratio
    t.enable_lamb(["roi_cnn."])  # (a second call only changes the exclusion)
    assert t.lamb_ratio is ratio and t.lamb.exclude == ("roi_cnn.",) and sum(t.lamb.adapt) == sum(not n.startswith("roi_cnn.") for n in names)
    # groups: the table carries the trainer's scales and decays; freeze_cnn: the tensors behind the CNN
    groups = [ss.ParamGroup("roi_cnn.", lr_scale=0.1), ss.no_decay()]
    t = skeleton(ss, model, param_groups=tuple(groups), weight_decay=1e-2)
    t.enable_lamb()
    assert t.lamb.lr_scale == [0.1, 1.0, 1.0] and t.lamb.weight_decay == [1e-2, 0.0, 1e-2]
    assert [t.lamb.seg_group[k] for k, n in enumerate(names) if n.startswith("roi_cnn.")] == [0] * sum(n.startswith("roi_cnn.") for n in names)
    n_cnn = model.cnn_param_range()
    t = skeleton(ss, model, n_frozen=n_cnn)
    t.enable_lamb()
    assert t.lamb_segments() == [n for n in names if not n.startswith("roi_cnn.")] and t.lamb.n == total - n_cnn
    with pytest.raises(ValueError, match="frozen ROI CNN"):
        skeleton(ss, model, n_frozen=n_cnn, param_groups=(groups[0],)).enable_lamb()
    # more than 64 tensors: eight GRU layers are 64 on their own
    deep = ss.BiGRUClassifier(84, 5, gru_layers=8)
    assert len(list(deep.named_parameters())) > 64 and len(deep.param_segments()[0]) == 1
    with pytest.raises(ValueError, match="64"):
        deep.param_tensor_segments()
    with pytest.raises(ValueError, match="64"):
        skeleton(ss, deep).enable_lamb()
    with pytest.raises(TypeError):  # the constructor's signature is what it always was
        ss.Trainer(model, lamb=True)


def test_state_dict_carries_lamb_and_a_disagreement_is_refused():
    import silent_speech_amd as ss

    model = ss.BiGRUClassifier(84, 5)
    plain, lamb, other = skeleton(ss, model), skeleton(ss, model), skeleton(ss, model)
    lamb.enable_lamb()
    other.enable_lamb(["gru."])
    old_keys = {"m", "v", "ema", "step_count", "ema_decay", "ema_warmup", "betas", "eps", "lr", "max_norm", "numel"}
    assert set(plain.state_dict()) == old_keys
    state = lamb.state_dict()
    assert set(state) == old_keys | {"lamb", "lamb_exclude"} and state["lamb"] is True
    assert state["lamb_exclude"] == list(ss.no_decay().match)
    lamb.load_state_dict(state)
    for a, b in ((plain, state), (other, state), (lamb, plain.state_dict()), (lamb, other.state_dict())):
        with pytest.raises(ValueError, match="lamb"):
            a.load_state_dict(b)
    plain.load_state_dict(plain.state_dict())


def test_fit_lamb_refuses_on_the_host(tmp_path, monkeypatch):
    from silent_speech_amd import harness as Hn

    def never(*a, **k):
        raise AssertionError("fit went past its argument checks")

    monkeypatch.setattr(Hn, "scan_clips", never)
    monkeypatch.setattr(Hn, "DeviceClipStore", never)
    out = str(tmp_path / "o.pt")
    for bad in ("", ["*"], 7):
        with pytest.raises(ValueError, match="exclude"):
            Hn.fit_lamb(str(tmp_path), out, bad, plan="device")
    with pytest.raises(TypeError):  # fit_args are fit's names
        Hn.fit_lamb(str(tmp_path), out, no_such_argument=1)
    with pytest.raises(TypeError):
        Hn.fit(str(tmp_path), out, lamb_exclude=None)
    with pytest.raises(ValueError, match="sam_rho"):
        Hn.fit_lamb(str(tmp_path), out, sam_rho=-1.0)
    with pytest.raises(ValueError, match="plan='device'"):  # good arguments go on to fit's own checks
        Hn.fit_lamb(str(tmp_path), out, ["gru."], plan="host", state_path=str(tmp_path / "s.pt"))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal returns before a launch: the pointers are host memory here and are never dereferenced."""
    from silent_speech_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    for name, n_args in (("ss_lamb_scratch_bytes", 3), ("ss_lamb_moments", 23), ("ss_lamb_apply", 20)):
        decl = hdr[hdr.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == n_args == len(_lib.SIGNATURES[name]), name
    lib = _lib.load()
    assert lib.ss_abi_version() == 3  # additions do not move it
    size = ctypes.c_long(-1)
    assert lib.ss_lamb_scratch_bytes(1031, 3, ctypes.addressof(size)) == 0 and size.value == 3 * 2 * 2 * 8
    assert lib.ss_lamb_scratch_bytes(1 << 30, 64, ctypes.addressof(size)) == 0 and size.value == 64 * 2048 * 2 * 8
    for bad in ((0, 1), (8, 0), (8, 65)):
        assert lib.ss_lamb_scratch_bytes(*bad, ctypes.addressof(size)) == -1
    assert lib.ss_lamb_scratch_bytes(8, 1, None) == -1
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15
    n = 1031
    p, g, m, v, e, s, scratch, norms, ratio = tuple(base + 4 * 1040 * k for k in range(6)) + (base + 4 * 6240, base + 4 * 6400, base + 4 * 6500)

    def table(ends=(4, 1028, n), ids=(0, 1, 0), scales=(1.0, 0.5), decays=(0.0, 0.1), adapt=(1, 0, 1)):
        arrs = ((ctypes.c_long * len(ends))(*ends), (ctypes.c_int * len(ids))(*ids), (ctypes.c_float * len(scales))(*scales),
                (ctypes.c_float * len(decays))(*decays), (ctypes.c_int * len(adapt))(*adapt))
        a = [ctypes.addressof(x) for x in arrs]
        return arrs, (a[0], a[1], len(ends), a[2], a[3], len(scales), a[4])

    def moments(p=p, g=g, m=m, v=v, n=n, s=s, step=1, scratch=scratch, norms=norms, ratio=ratio, **tk):
        keep, args = table(**tk)
        return lib.ss_lamb_moments(p, g, m, v, n, s, 1.0, 1.0, 0.9, 0.999, 1e-8, step, *args, scratch, norms, ratio, None)

    def apply(p=p, m=m, v=v, e=e, n=n, step=1, d=0.9, lr=3e-4, ratio=ratio, **tk):
        keep, args = table(**tk)
        return lib.ss_lamb_apply(p, m, v, e, n, 0.9, 0.999, 1e-8, step, d, lr, *args, ratio, None)

    long65 = dict(ends=tuple(4 * (k + 1) for k in range(64)) + (n,), ids=(0,) * 65, adapt=(1,) * 65)
    shared = (long65, dict(p=p + 4), dict(m=m + 8), dict(v=None), dict(n=0), dict(step=0), dict(decays=(0.0, float("nan"))),
              dict(decays=(0.0, -0.1)), dict(scales=(float("inf"), 1.0)), dict(ends=(4, 1026, n)), dict(ends=(4, 4, n)),
              dict(ends=(4, 1028, n - 1)), dict(ids=(0, 2, 0)), dict(ratio=None))
    for bad in shared:
        assert moments(**bad) == -1, bad
        assert apply(**bad) == -1, bad
    for bad in (dict(g=None), dict(g=g + 4), dict(s=None), dict(scratch=None), dict(scratch=scratch + 4), dict(norms=None)):
        assert moments(**bad) == -1, bad
    for bad in (dict(e=p), dict(e=p + 16 * 8), dict(e=p - 16), dict(e=e + 4), dict(d=1.0), dict(d=float("nan")), dict(d=-0.1),
                dict(lr=float("nan")), dict(lr=-1.0)):
        assert apply(**bad) == -1, bad
    assert not any(buf)


# --------------------------------------------------------------------------------------------------------- public surface
def test_signatures_docstrings_and_fingerprint():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    sig = inspect.signature(Hn.fit_lamb).parameters
    assert list(sig) == ["clip_dir", "out_path", "lamb_exclude", "fit_args"] and sig["lamb_exclude"].default is None
    assert sig["fit_args"].kind.name == "VAR_KEYWORD"
    sig = inspect.signature(ss.Trainer.enable_lamb).parameters
    assert list(sig) == ["self", "exclude"] and sig["exclude"].default is None
    for fn in (Hn.fit, ss.Trainer.__init__, Hn.run_fingerprint):  # (tests/test_interface_cpu.py spells them out)
        assert not any("lamb" in name for name in inspect.signature(fn).parameters)
    for word in ("enable_lamb", "ss_lamb_moments", "ss_lamb_apply", "trust_ratios", "lamb_segments", "lamb_exclude"):
        assert word in ss.Trainer.__doc__, word
    assert "fit_lamb" in Hn.fit.__doc__ and "lamb" in ss.Trainer.load_state_dict.__doc__ and "trust ratio" in Hn.fit_lamb.__doc__
    fields = dict(seed=42, batch_size=16, world_size=1, max_t=24, lr=3e-4, labels=["aura", "no"], x_dim=20, use_roi=True, n_train=38,
                  n_val=7, class_weights=None, augment_policy=None, ema_decay=None)
    assert Hn.lamb_fingerprint(Hn.run_fingerprint(**fields), None) == fields
    lamb = Hn.lamb_fingerprint(fields, ("*bias", "head.0."))
    assert lamb == dict(fields, lamb=True, lamb_exclude=["*bias", "head.0."])
    assert Ck.fingerprint_difference(fields, lamb) in ("lamb", "lamb_exclude") and Ck.fingerprint_difference(lamb, lamb) is None
    assert Ck.fingerprint_difference(lamb, Hn.lamb_fingerprint(fields, ())) == "lamb_exclude"
