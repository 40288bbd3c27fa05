"""GPU: the weight average fused into the Adam launch (``ss_adam_clip_ema``), the in-place exchange (``ss_swap_f32``),
``Trainer(ema_decay=)`` with ``ema_weights()`` and ``state_dict()``, and ``harness.fit(ema_decay=, state_path=, resume=)``.

Bounds.  The average: 2 float32 ulp of ``max(|ema_old|, |p_new|)`` round the float64 value of ``d * ema_old + float32(1 - d) *
p_new`` (two rounded products and one rounded sum: at most 1.5 ulp, with or without contraction; ``optim_ref.ema_expected``).
Losses of two runs that issue the same launches: ``LOSS_BOUND``, the atomic-order noise measured for exactly the ``FIT``
configuration below (tests/test_gpu_data_parallel.py: two uninterrupted single-process runs differed by at most 9.781275e-08
per epoch; ten times that).  ``p``, ``m``, ``v`` of the two optimiser entry points, and logits of the same weights: equal bits."""
import os

import numpy as np
import pytest
import torch

import flat_ref as FR
import optim_ref as OR
import weights as W
from gpu_support import L, WORDS, ss, write_clips  # noqa: F401

pytestmark = pytest.mark.gpu

SPREAD = 9.781275e-08
LOSS_BOUND = 10 * SPREAD
NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 256 * 4 * 3 + 2]  # tail alone, one vector, vector + tail, both sides of a workgroup's stride
# one sweep of the capped grid of ss_adam_clip_ema and ss_swap_f32 is 2048 x 256 x 4 = 2 097 152 elements: both sides of it, a
# second trip of one lane + a tail, a third trip
NS_LARGE = [2097151, 2097152, 2097157, 4194311]
N_FOUR_SWEEPS = 4 * 2097152 + 5  # four whole sweeps, then a fifth trip of one lane + one tail element
NS_FLOAT64 = (2097157, 4194311)
DECAYS = [0.0, 0.1, 0.999]
ADAM = (1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8)  # grad_scale, max_norm, lr, beta1, beta2, eps
FIT = dict(epochs=3, batch_size=16, patience=3, max_t=24, lr=3e-3, plan="device")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- kernels
def optimiser_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)

    def randn():  # (among millions of draws an exact 0.0 does turn up: that element gets 0.5)
        t = torch.randn(n, generator=g)
        return torch.where(t == 0, torch.full_like(t, 0.5), t)

    p, m, ema = randn(), 0.01 * randn(), randn()
    v = 1e-4 * torch.rand(n, generator=g) + 1e-8
    grads = [0.05 * torch.randn(n, generator=g), 3.0 * torch.randn(n, generator=g)]  # (the second one is clipped for n > 1)
    assert all(bool((t != 0).all()) for t in (p, m, v, ema))
    return p, m, v, ema, grads


def check_adam_clip_ema(L, n, decays, against_float64=False):
    """Two steps (step numbers 1 and 7) from nonzero moments: p, m, v of ``ss_adam_clip_ema`` are the bits of ``ss_adam_clip`` on
    copies of the same inputs; the average is within 2 ulp of its float64 value; d = 0 makes it p_new exactly.
    ``against_float64``: p, m, v are also within ``flat_ref.adam_clip_expected``'s bounds of the float64 step from the values and
    the sumsq word the kernel saw (first decay only) -> the largest error / bound ratios."""
    p, m, v, ema, grads = optimiser_inputs(n, 100 + n)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for d in decays:
        A = [t.cuda() for t in (p, m, v)]
        B = [t.cuda() for t in (p, m, v)]
        e_d, ssq = ema.cuda(), torch.zeros(1, device="cuda")
        for step, g in zip((1, 7), grads):
            g_d = g.cuda()
            ssq.zero_()
            L.call("ss_sumsq_f32", g_d.data_ptr(), n, ssq.data_ptr(), L.stream())
            ema_old = e_d.cpu().numpy().copy()
            before = [t.cpu().numpy() for t in B] if against_float64 and d == decays[0] else None
            L.call("ss_adam_clip", A[0].data_ptr(), g_d.data_ptr(), A[1].data_ptr(), A[2].data_ptr(), n, ssq.data_ptr(), *ADAM, step,
                   L.stream())
            L.call("ss_adam_clip_ema", B[0].data_ptr(), g_d.data_ptr(), B[1].data_ptr(), B[2].data_ptr(), e_d.data_ptr(), n,
                   ssq.data_ptr(), *ADAM, step, d, L.stream())
            torch.cuda.synchronize()
            for name, a, b in zip("pmv", A, B):
                assert torch.equal(a, b), (name, n, d, step, int((a != b).sum()))
            assert not torch.equal(A[0].cpu(), p)  # (the step did something)
            p_new, ema_new = B[0].cpu().numpy(), e_d.cpu().numpy()
            want, bound = OR.ema_expected(ema_old, p_new, d)
            err = np.abs(ema_new.astype(np.float64) - want)
            assert (err <= bound).all(), (n, d, step, float((err / bound).max()))
            if d == 0.0:
                assert np.array_equal(ema_new, p_new)
            else:
                assert not np.array_equal(ema_new, p_new) and not np.array_equal(ema_new, ema_old)
            if before is not None:
                want, bound = FR.adam_clip_expected(before[0], g.numpy(), before[1], before[2], np.float32(float(ssq[0])), step,
                                                    lr=ADAM[2], max_norm=ADAM[1], beta1=ADAM[3], beta2=ADAM[4], eps=ADAM[5],
                                                    grad_scale=ADAM[0])
                for name, b in zip("pmv", B):
                    err = np.abs(b.cpu().numpy().astype(np.float64) - want[name])
                    worst[name] = max(worst[name], float((err / bound[name]).max()))
                    assert (err <= bound[name]).all(), (name, n, step, worst[name])
    return worst


@pytest.mark.parametrize("n", NS)
def test_adam_clip_ema_against_adam_clip(L, n):
    check_adam_clip_ema(L, n, DECAYS)


@pytest.mark.parametrize("n", NS_LARGE + [N_FOUR_SWEEPS])
def test_adam_clip_ema_past_one_sweep_of_the_capped_grid(L, n):
    """The same checks where the 2048-workgroup grid strides a second, a third and a fifth time (two decays; d = 0 still makes the
    average p_new exactly), and at two of the sizes p, m, v against the float64 step as well, not only against ``ss_adam_clip``."""
    worst = check_adam_clip_ema(L, n, [0.0, 0.999], against_float64=n in NS_FLOAT64)
    if n in NS_FLOAT64:
        print(f"adam_clip_ema n={n}: largest err / bound  m {worst['m']:.4f}  v {worst['v']:.4f}  p {worst['p']:.4f}")


def test_adam_clip_ema_refuses_bad_arguments_and_writes_nothing(L):
    n = 1025
    p, m, v, ema, grads = optimiser_inputs(n, 7)
    dev = [t.cuda() for t in (p, grads[0], m, v, ema)]
    ssq = torch.ones(1, device="cuda")
    lib = L.load()

    def status(p_ptr, ema_ptr, n_, decay, step=1):
        return lib.ss_adam_clip_ema(p_ptr, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), ema_ptr, n_, ssq.data_ptr(),
                                    *ADAM, step, decay, L.stream())

    P, E = dev[0].data_ptr(), dev[4].data_ptr()
    assert status(P, P, n, 0.9) == -1                 # ema == p
    assert status(P, P + 16, n - 4, 0.9) == -1        # ... or anywhere inside it
    assert status(P, E, n, 1.0) == -1                 # ema_decay = 1
    assert status(P, E, n, -0.5) == -1 and status(P, E, n, float("nan")) == -1
    assert status(P, E, 0, 0.9) == -1                 # n = 0
    assert status(P, E, n, 0.9, step=0) == -1
    assert status(P, None, n, 0.9) == -1 and status(None, E, n, 0.9) == -1
    assert status(P, E + 4, n - 1, 0.9) == -1         # a pointer the 16-byte lanes cannot take
    torch.cuda.synchronize()
    for t, h in zip(dev, (p, grads[0], m, v, ema)):
        assert torch.equal(bits(t), bits(h))
    with pytest.raises(RuntimeError, match="invalid argument"):
        L.call("ss_adam_clip_ema", P, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), P, n, ssq.data_ptr(), *ADAM, 1, 0.9,
               L.stream())
    assert status(P, E, n, 0.9) == 0                  # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not torch.equal(dev[0].cpu(), p) and not torch.equal(dev[4].cpu(), ema)


GUARD = 8  # words behind each buffer (behind the whole 16-byte lanes the buffer's end lies in)


def guarded(n, seed):
    """-> (allocation, its original bits on the host): arbitrary bit patterns (NaN payloads included), the first n words are
    the buffer, the rest the guard."""
    g = torch.Generator().manual_seed(seed)
    host = torch.randint(-2 ** 31, 2 ** 31 - 1, ((n + 3) // 4 * 4 + GUARD,), generator=g, dtype=torch.int64).to(torch.int32)
    return host.cuda().view(torch.float32), host


@pytest.mark.parametrize("n", NS + NS_LARGE)
def test_swap_exchanges_two_buffers_in_place(L, n):
    a, a0 = guarded(n, 2 * n)
    b, b0 = guarded(n, 2 * n + 1)
    lib = L.load()
    L.call("ss_swap_f32", a.data_ptr(), b.data_ptr(), n, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(a)[:n], b0[:n]) and torch.equal(bits(b)[:n], a0[:n]) and not torch.equal(a0[:n], b0[:n])
    assert torch.equal(bits(a)[n:], a0[n:]) and torch.equal(bits(b)[n:], b0[n:])  # the guard words
    L.call("ss_swap_f32", a.data_ptr(), b.data_ptr(), n, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(a), a0) and torch.equal(bits(b), b0)
    # overlap is refused (the second range begins inside the first, or is the first), so are n = 0 and a misaligned pointer
    assert lib.ss_swap_f32(a.data_ptr(), a.data_ptr(), n, L.stream()) == -1
    if n > 8:
        assert lib.ss_swap_f32(a.data_ptr(), a.data_ptr() + 16, n - 4, L.stream()) == -1
    if n > 4:
        assert lib.ss_swap_f32(a.data_ptr() + 16 * ((n - 1) // 4), a.data_ptr(), n, L.stream()) == -1
        assert lib.ss_swap_f32(a.data_ptr() + 4, b.data_ptr(), n - 1, L.stream()) == -1
    assert lib.ss_swap_f32(a.data_ptr(), b.data_ptr(), 0, L.stream()) == -1
    assert lib.ss_swap_f32(None, b.data_ptr(), n, L.stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(a), a0) and torch.equal(bits(b), b0)


# ---------------------------------------------------------------------------------------------------------------- Trainer
B_, T_, ROI = 16, 8, (32, 32)


def roi_model(ss, seed=11):
    m = ss.BiGRUClassifier(84, 5, use_roi=True)
    m.load_state_dict(W.make_state_dict(seed, 84, 5, True))
    return m.cuda().train()


def batch(seed):
    X, Lh, R, y = W.make_inputs(seed, B_, T_, 84, 5, ROI)
    return X.cuda(), Lh.cuda(), R.cuda(), y.cuda()


def test_trainer_ema_follows_the_recursion_and_leaves_the_steps_alone(ss):
    """Five steps (dropout on, five different batches).  After each: the average against the float64 recursion from the
    previous read with the warm-up decay of the step; the loss against a second Trainer without an average on an identically
    initialised model -- the same launches but for the optimiser's entry point, whose p, m, v are the same bits."""
    from silent_speech_amd.train import ema_decay_at

    m1, m2 = roi_model(ss), roi_model(ss)
    t1, t2 = ss.Trainer(m1, ema_decay=0.9), ss.Trainer(m2)
    assert t2.ema is None and torch.equal(t1.ema, m1.flat_params) and t1.ema.data_ptr() != m1.flat_params.data_ptr()
    ema_prev = t1.ema.cpu().numpy().copy()
    for step in range(1, 6):
        X, Lh, R, y = batch(30 + step)
        l1, _ = t1.step(X, Lh, R, y)
        l2, _ = t2.step(X, Lh, R, y)
        p_new, ema_new = m1.flat_params.cpu().numpy(), t1.ema.cpu().numpy().copy()
        d = ema_decay_at(0.9, step)
        assert d == min(0.9, (1 + step) / (10 + step)) and t1.step_count == step
        want, bound = OR.ema_expected(ema_prev, p_new, d)
        err = np.abs(ema_new.astype(np.float64) - want)
        print(f"step {step}: decay {d:.6f}, ema err / bound {float((err / bound).max()):.3f}, loss {float(l1):.9f} against "
              f"{float(l2):.9f} (diff {abs(float(l1) - float(l2)):.3e})")
        assert (err <= bound).all(), (step, float((err / bound).max()))
        assert not np.array_equal(ema_new, p_new) and not np.array_equal(ema_new, ema_prev)
        assert abs(float(l1) - float(l2)) <= LOSS_BOUND, (step, float(l1), float(l2))
        ema_prev = ema_new
    # without warm-up the decay is the constant
    t3 = ss.Trainer(roi_model(ss), ema_decay=0.9, ema_warmup=False)
    e0 = t3.ema.cpu().numpy().copy()
    t3.step(*batch(31))
    want, bound = OR.ema_expected(e0, t3.model.flat_params.cpu().numpy(), 0.9)
    assert (np.abs(t3.ema.cpu().numpy().astype(np.float64) - want) <= bound).all()


def check_ema_weights(ss, model, trainer, fresh, inputs):
    """``fresh``: an untrained model of the same architecture on the CPU.  Logits are compared bit for bit: inference here is
    reproducible from launch to launch (the existing model tests compare logits of repeated forwards with ``torch.equal``)."""
    X, Lh, R, y = inputs
    model.eval()
    with torch.no_grad():
        before = model(X, Lh, R)
        again = model(X, Lh, R)
    assert torch.equal(before, again)
    raw = model.flat_params.clone()
    avg = trainer.ema.clone()
    assert not torch.equal(raw, avg)
    fresh.load_state_dict({k: v.cpu() for k, v in model._views_of(avg).items()})
    fresh.cuda().eval()
    with torch.no_grad():
        ref = fresh(X, Lh, R)
    with trainer.ema_weights():
        assert torch.equal(model.flat_params, avg) and torch.equal(trainer.ema, raw)
        assert all(torch.equal(p.data, v) for p, v in zip(model.parameters(), model._views_of(avg).values()))
        with torch.no_grad():
            inside = model(X, Lh, R)
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.step(X, Lh, R, y)
        with pytest.raises(RuntimeError, match="nest"):
            with trainer.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            trainer.state_dict()
    assert torch.equal(inside, ref) and not torch.equal(inside, before)
    assert torch.equal(model.flat_params, raw) and torch.equal(trainer.ema, avg)
    with torch.no_grad():
        after = model(X, Lh, R)
    assert torch.equal(after, before)
    with pytest.raises(KeyError, match="thrown inside"):
        with trainer.ema_weights():
            assert torch.equal(model.flat_params, avg)
            raise KeyError("thrown inside")
    assert torch.equal(model.flat_params, raw) and torch.equal(trainer.ema, avg)
    model.train()  # and the trainer carries on
    count = trainer.step_count
    trainer.step(X, Lh, R, y)
    assert trainer.step_count == count + 1 and not torch.equal(model.flat_params, raw)


def test_ema_weights_puts_the_average_behind_the_module(ss):
    model = roi_model(ss)
    trainer = ss.Trainer(model, ema_decay=0.9)
    for k in range(3):
        trainer.step(*batch(40 + k))
    check_ema_weights(ss, model, trainer, ss.BiGRUClassifier(84, 5, use_roi=True), batch(50))
    with pytest.raises(RuntimeError, match="ema_decay"):
        with ss.Trainer(roi_model(ss)).ema_weights():
            pass


def test_ema_weights_on_the_bf16_engine(ss):
    """The bf16 engine converts its GRU weights to bf16 inside every forward (``ss_gru_bf16_prep``); a copy that outlived a
    forward would make the logits inside ``ema_weights()`` those of the raw weights.  A landmark-only three-layer model."""
    kw = dict(use_roi=False, hidden=512, gru_layers=3, precision="bf16")
    Bn, Tn = 64, 6
    model = ss.BiGRUClassifier(84, 7, **kw)
    model.load_state_dict(W.make_state_dict(8, 84, 7, False, hidden=512, gru_layers=3))
    model.cuda().train()
    X, Lh, _, y = W.make_inputs(8, Bn, Tn, 84, 7, None, lengths=[Tn] * Bn)
    inputs = (X.cuda(), Lh.cuda(), None, y.cuda())
    trainer = ss.Trainer(model, ema_decay=0.5, ema_warmup=False, lr=3e-3)
    for _ in range(2):
        trainer.step(*inputs)
    check_ema_weights(ss, model, trainer, ss.BiGRUClassifier(84, 7, **kw), inputs)


def test_trainer_state_round_trip(ss):
    m1 = roi_model(ss)
    t1 = ss.Trainer(m1, ema_decay=0.9, lr=1e-3)
    for k in range(2):
        t1.step(*batch(60 + k))
    state = t1.state_dict()
    assert set(state) == {"m", "v", "ema", "step_count", "ema_decay", "ema_warmup", "betas", "eps", "lr", "max_norm", "numel"}
    assert state["numel"] == m1.flat_params.numel() and state["step_count"] == 2 and state["ema_decay"] == 0.9
    assert state["m"].data_ptr() != t1.m.data_ptr()  # copies
    m2 = ss.BiGRUClassifier(84, 5, use_roi=True)
    m2.load_state_dict({k: v.cpu() for k, v in m1.state_dict().items()})
    m2.cuda().train()
    assert torch.equal(m2.flat_params, m1.flat_params)
    t2 = ss.Trainer(m2, ema_decay=0.5)
    ptrs = (t2.m.data_ptr(), t2.v.data_ptr(), t2.ema.data_ptr())
    t2.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})  # (as read from a file)
    assert ptrs == (t2.m.data_ptr(), t2.v.data_ptr(), t2.ema.data_ptr())  # copied into the buffers it had
    for name in ("m", "v", "ema"):
        assert torch.equal(bits(getattr(t2, name)), bits(state[name])) and bool(state[name].any()), name
    assert t2.step_count == 2 and t2.ema_decay == 0.9 and t2.lr == 1e-3 and t2.betas == (0.9, 0.999)
    nxt = batch(70)
    l1, l2 = float(t1.step(*nxt)[0]), float(t2.step(*nxt)[0])
    print(f"next step: {l1:.9f} against {l2:.9f} (diff {abs(l1 - l2):.3e})")
    assert abs(l1 - l2) <= LOSS_BOUND
    # another bucket, or an average on one side only, is refused
    small = ss.Trainer(ss.BiGRUClassifier(84, 5, use_roi=False).cuda(), ema_decay=0.9)
    with pytest.raises(ValueError, match="elements"):
        small.load_state_dict(state)
    with pytest.raises(ValueError, match="ema_decay"):
        ss.Trainer(m2).load_state_dict(state)
    plain = ss.Trainer(roi_model(ss)).state_dict()
    assert plain["ema"] is None and plain["ema_decay"] is None
    with pytest.raises(ValueError, match="ema_decay"):
        t2.load_state_dict(plain)


# -------------------------------------------------------------------------------------------------------------------- fit
@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    return write_clips(str(tmp_path_factory.mktemp("resume") / "clips_npz"), WORDS)


@pytest.fixture(scope="module")
def runs(ss, clip_dir, tmp_path_factory):
    """(a) three epochs uninterrupted; (b) one epoch, then resumed to three.  Each ``fit`` once."""
    from silent_speech_amd import harness as Hn

    d = tmp_path_factory.mktemp("runs")
    s1, s2 = str(d / "a_state.pt"), str(d / "b_state.pt")
    ha, hb1, hb2, logs = [], [], [], []
    best_a = Hn.fit(clip_dir, str(d / "a.pt"), state_path=s1, history=ha, log=logs.append, **FIT)
    best_b1 = Hn.fit(clip_dir, str(d / "b.pt"), state_path=s2, history=hb1, log=logs.append, **dict(FIT, epochs=1))
    after_one = torch.load(s2, map_location="cpu", weights_only=True)
    best_b = Hn.fit(clip_dir, str(d / "b.pt"), state_path=s2, resume=True, history=hb2, log=logs.append, **FIT)
    return dict(s1=s1, s2=s2, ha=ha, hb1=hb1, hb2=hb2, best_a=best_a, best_b1=best_b1, best_b=best_b, after_one=after_one, logs=logs,
                dir=d)


def test_resumed_fit_equals_the_uninterrupted_one(ss, runs, clip_dir):
    """Epochs 2 and 3 of the resumed run against those of the uninterrupted one: ``train_loss`` and ``val_loss`` within
    ``LOSS_BOUND`` (the bound measured between two uninterrupted runs of this configuration).  Losing the Adam moments or the
    step count (the bias corrections and the dropout seeds) moves the epoch-2 train loss by far more."""
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    ha, hb1, hb2 = runs["ha"], runs["hb1"], runs["hb2"]
    assert [h["epoch"] for h in ha] == [1, 2, 3] and [h["epoch"] for h in hb1] == [1] and [h["epoch"] for h in hb2] == [2, 3]
    for a, b in zip(ha, hb1 + hb2):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {a['epoch']} {key}: uninterrupted {a[key]:.9f} resumed {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
    for a, b in zip(ha, hb1 + hb2):
        assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
    assert runs["best_a"] >= 0.8 and runs["best_b"] >= 0.8 and runs["best_b"] >= runs["best_b1"]
    # the files: what they hold, and that the plain loader reads them
    one, three = runs["after_one"], Ck.load_train_state(runs["s2"])
    assert one["epoch"] == 1 and three["epoch"] == 3 and one["trainer"]["step_count"] == 3 and three["trainer"]["step_count"] == 9
    assert three["best"] == runs["best_b"] and three["trainer"]["ema"] is None and three["fingerprint"]["seed"] == 42
    assert three["fingerprint"]["labels"] == WORDS and three["fingerprint"]["n_train"] + three["fingerprint"]["n_val"] == 45
    model = ss.load_classifier(str(runs["dir"] / "b.pt"))[0]
    assert set(three["model"]) == set(model.state_dict())
    assert os.listdir(os.path.dirname(runs["s2"])).count("b_state.pt") == 1
    assert not [f for f in os.listdir(os.path.dirname(runs["s2"])) if ".tmp" in f]
    # a third call finds nothing left to do
    history = []
    assert Hn.fit(clip_dir, str(runs["dir"] / "b.pt"), state_path=runs["s2"], resume=True, history=history, log=lambda *a: None,
                  **FIT) == runs["best_b"]
    assert history == []
    # resume=True without a file starts fresh (one epoch is enough to see it)
    fresh_state, history = str(runs["dir"] / "fresh_state.pt"), []
    Hn.fit(clip_dir, str(runs["dir"] / "fresh.pt"), state_path=fresh_state, resume=True, history=history, log=lambda *a: None,
           **dict(FIT, epochs=1))
    assert [h["epoch"] for h in history] == [1] and abs(history[0]["train_loss"] - ha[0]["train_loss"]) <= LOSS_BOUND
    assert Ck.load_train_state(fresh_state)["epoch"] == 1


def test_resume_refuses_another_configuration(ss, runs, clip_dir):
    from silent_speech_amd import harness as Hn

    out = str(runs["dir"] / "never.pt")
    with pytest.raises(ValueError, match="batch_size"):
        Hn.fit(clip_dir, out, state_path=runs["s2"], resume=True, **dict(FIT, batch_size=8))
    with pytest.raises(ValueError, match="seed"):
        Hn.fit(clip_dir, out, state_path=runs["s2"], resume=True, seed=7, **FIT)
    with pytest.raises(ValueError, match="ema_decay"):
        Hn.fit(clip_dir, out, state_path=runs["s2"], resume=True, ema_decay=0.9, **FIT)
    assert not os.path.exists(out)


def test_state_path_needs_the_device_plan(ss, clip_dir, tmp_path):
    from silent_speech_amd import harness as Hn

    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(clip_dir, str(tmp_path / "m.pt"), state_path=str(tmp_path / "s.pt"), **dict(FIT, plan="host"))
    assert os.listdir(tmp_path) == []


def test_fit_with_ema_saves_the_averaged_weights(ss, clip_dir, tmp_path):
    """One epoch, so the epoch of the checkpoint is the epoch of the state file: the ``.pt`` (reference schema, read by
    ``load_classifier``) holds the average, the state file the raw weights next to it."""
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    out, S, history = str(tmp_path / "ema.pt"), str(tmp_path / "ema_state.pt"), []
    best = Hn.fit(clip_dir, out, ema_decay=0.9, state_path=S, history=history, log=lambda *a: None, **dict(FIT, epochs=1))
    print(f"fit(ema_decay=0.9), one epoch: {history[0]}")
    state = Ck.load_train_state(S)
    model, id_to_label, max_t, use_roi = ss.load_classifier(out)
    assert max_t == 24 and use_roi and sorted(id_to_label.values()) == WORDS
    assert state["epoch"] == 1 and state["trainer"]["ema_decay"] == 0.9 and state["fingerprint"]["ema_decay"] == 0.9
    assert torch.equal(bits(model.flat_params), bits(state["trainer"]["ema"]))
    raw = ss.BiGRUClassifier(20, 3, use_roi=True)
    raw.load_state_dict(state["model"])
    assert not torch.equal(raw.flat_params, model.flat_params.cpu())
    # (Adam moves every weight with a nonzero gradient by about lr per step and the average lags behind: most words differ)
    assert float((raw.flat_params != model.flat_params.cpu()).float().mean()) > 0.5
    assert history[0]["val_acc"] == best
    assert best >= 0.8, best
