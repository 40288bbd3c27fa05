"""GPU: the layer-wise adaptive optimiser LAMB in the fused train step (``Trainer.enable_lamb``, ``harness.fit_lamb``).

The two entry points -- ``ss_lamb_moments``, ``ss_lamb_apply`` (csrc/optim.hip) -- on NaN-guarded sub-ranges at their tail, segment,
piece and grid-cap edges: the moments bit for bit against ``ss_adam_clip``, the norms, ratios and weights within the bounds
tests/lamb_ref.py derives (float64 on the float32 values the kernels read; tests/test_lamb_cpu.py pins it against torch without
a GPU), exactly where the arithmetic is exact, and the same bits from two calls; then the trainer: against the CPU oracle on both
engines, with SAM, frozen, its launch list, and a resumed ``fit_lamb``.  Every test prints what it measured before it asserts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import flat_ref as FR
import lamb_ref as LR
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

LR0, BETAS_EPS = ADAM[2], ADAM[3:]
ADAM_KW = dict(beta1=ADAM[3], beta2=ADAM[4], eps=ADAM[5])
SWEEP = 2048 * 256 * 4  # elements one sweep of the capped grid covers: the workgroup cap times 1024
# name -> (n, segment ends).  n & 3 in {0, 1, 3}; a 4-element segment; an end inside a 256-quad piece (quad 100 of the first; and
# 1028 = quad 257, one quad into the second); 64 segments; a tail segment of three elements and no quad; one n past the capped
# grid's sweep whose first segment alone is 2049 pieces on the grid of 2048: workgroup 0 takes two pieces of it, so the grid-stride
# loop of both kernels runs a second trip and a thread adds two quads into its sums before the reduction
TABLES = {
    "one_segment_tail_0": (1028, [1028]),
    "one_segment_tail_1": (1025, [1025]),
    "four_elements_and_piece_edges_tail_3": (2051, [4, 400, 1028, 2051]),
    "sixty_four_segments": (64 * 12 + 1, [12 * (k + 1) for k in range(63)] + [64 * 12 + 1]),
    "a_tail_segment_of_its_own": (1027, [512, 1024, 1027]),
    "past_the_workgroup_cap": (SWEEP + 1203, [SWEEP + 400, SWEEP + 800, SWEEP + 1203]),
}
SCALES, DECAYS = [1.0, 0.1], [1e-2, 0.0]


def table_arrays(ends, ids, scales, decays, adapt):
    arrs = ((C.c_long * len(ends))(*ends), (C.c_int * len(ids))(*ids), (C.c_float * len(scales))(*scales),
            (C.c_float * len(decays))(*decays), (C.c_int * len(adapt))(*adapt))
    a = [C.addressof(x) for x in arrs]
    return arrs, (a[0], a[1], len(ends), a[2], a[3], len(scales), a[4])


def scratch_for(L, n, n_seg, fill):
    """The partial sums' buffer, as large as the library asks, filled with NaN (or any ``fill``): it need not be cleared."""
    size = C.c_long(0)
    L.call("ss_lamb_scratch_bytes", n, n_seg, C.addressof(size))
    assert size.value == n_seg * min(max((n // 4 + 255) // 256, 1), 2048) * 16
    return torch.full((size.value // 8,), fill, dtype=torch.float64, device="cuda")


def run_moments(L, host, sumsq, step, ends, ids, scales, decays, adapt, fill=float("nan"), seed=0):
    """One ``ss_lamb_moments`` call on guarded copies of (p, g, m, v) -> dict of m, v, norms (n_seg, 2), ratio; asserts that the
    guards, p, g, the sumsq word and the floats behind norms and ratio are as they were, and that no NaN reached a norm."""
    n, n_seg = host[0].size, len(ends)
    P, G, M, V = bufs = [Guarded(a, seed + i) for i, a in enumerate(host)]
    ssq = torch.tensor([sumsq], dtype=torch.float32).cuda()
    scratch = scratch_for(L, n, n_seg, fill)
    norms, ratio = torch.full((2 * n_seg + 4,), -7.0).cuda(), torch.full((n_seg + 4,), -7.0).cuda()
    keep, args = table_arrays(ends, ids, scales, decays, adapt)
    L.call("ss_lamb_moments", P.ptr, G.ptr, M.ptr, V.ptr, n, ssq.data_ptr(), ADAM[0], ADAM[1], *BETAS_EPS, step, *args,
           scratch.data_ptr(), norms.data_ptr(), ratio.data_ptr(), L.stream())
    torch.cuda.synchronize()
    for b, name in zip(bufs, "pgmv"):
        b.check_guards(name)
    P.check_untouched("p")
    G.check_untouched("g")
    assert float(ssq[0]) == float(np.float32(sumsq))
    norms, ratio = norms.cpu().numpy(), ratio.cpu().numpy()
    assert (norms[2 * n_seg:] == -7.0).all() and (ratio[n_seg:] == -7.0).all()
    assert np.isfinite(norms[:2 * n_seg]).all() and np.isfinite(ratio[:n_seg]).all()
    return dict(m=M.values(), v=V.values(), norms=norms[:2 * n_seg].reshape(n_seg, 2).copy(), ratio=ratio[:n_seg].copy())


def run_adam(L, host, sumsq, step, lr=LR0):
    dev = [torch.from_numpy(a.copy()).cuda() for a in host]
    ssq = torch.tensor([sumsq], dtype=torch.float32).cuda()
    L.call("ss_adam_clip", *(t.data_ptr() for t in dev), host[0].size, ssq.data_ptr(), ADAM[0], ADAM[1], lr, *BETAS_EPS, step, L.stream())
    torch.cuda.synchronize()
    return dict(p=dev[0].cpu().numpy(), m=dev[2].cpu().numpy(), v=dev[3].cpu().numpy())


def run_apply(L, p, m, v, ema, ratio, step, d, ends, ids, scales, decays, adapt, lr=LR0):
    """One ``ss_lamb_apply`` call on guarded copies -> (new p, new ema or None); m, v and the ratios are only read."""
    n = p.size
    P, M, V = Guarded(p, 1), Guarded(m, 2), Guarded(v, 3)
    E_ = None if ema is None else Guarded(ema, 4)
    r = torch.from_numpy(np.asarray(ratio, np.float32)).cuda()
    keep, args = table_arrays(ends, ids, scales, decays, adapt)
    L.call("ss_lamb_apply", P.ptr, M.ptr, V.ptr, None if E_ is None else E_.ptr, n, *BETAS_EPS, step, 0.0 if d is None else d, lr, *args,
           r.data_ptr(), L.stream())
    torch.cuda.synchronize()
    for b, name in ((P, "p"), (M, "m"), (V, "v")) + (() if E_ is None else ((E_, "ema"),)):
        b.check_guards(name)
    M.check_untouched("m")
    V.check_untouched("v")
    assert np.array_equal(r.cpu().numpy().view(np.int32), np.asarray(ratio, np.float32).view(np.int32))
    return P.values(), None if E_ is None else E_.values()


def case(n, seed):
    p, g, m, v = FR.optimiser_case(n, seed)
    return (p, g, m, v), np.random.default_rng(seed + 1).standard_normal(n).astype(np.float32)


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))  # (a bound of 0 asks for the exact value)
    assert (err <= bound).all(), (what, worst, int(np.argmax(err - bound)))
    return worst


# ---------------------------------------------------------------------------------------------------------- moments and norms
@pytest.mark.parametrize("name", list(TABLES))
def test_moments_are_adam_clips_bits_and_norms_lie_within_the_derived_bound(L, name):
    """Steps 1 and 7 from nonzero moments, the second one clipped: m and v are the bits of one ``ss_adam_clip`` launch on the whole
    range; sqrt P, sqrt U and the ratio of every segment lie within ``lamb_ref.norms_expected``'s bounds, taken from the float32
    moments the kernel stored; excluded segments (every third, from the second on) have the ratio 1 exactly.  The scratch is NaN-filled."""
    n, ends = TABLES[name]
    ids, adapt = [k % 2 for k in range(len(ends))], [int(k % 3 != 1) for k in range(len(ends))]
    host, _ = case(n, 500 + len(ends))
    for step, sumsq in ((1, 1e-3), (7, 4.0)):
        got = run_moments(L, host, sumsq, step, ends, ids, SCALES, DECAYS, adapt, seed=step)
        want = run_adam(L, host, sumsq, step)
        for k in "mv":
            a, b = got[k].view(np.int32), want[k].view(np.int32)
            assert np.array_equal(a, b), (name, step, k, int((a != b).sum()), int(np.flatnonzero(a != b)[0]))
        assert not np.array_equal(got["m"], host[2])
        (wp, bp), (wu, bu), (wr, br) = LR.norms_expected(host[0], got["m"], got["v"], step, ends, ids, DECAYS, adapt, **ADAM_KW)
        worst = [within(got["norms"][:, 0], wp, bp, "sqrt P"), within(got["norms"][:, 1], wu, bu, "sqrt U"), within(got["ratio"], wr, br, "ratio")]
        print(f"{name} step {step}: largest err / bound  sqrt P {worst[0]:.3f}  sqrt U {worst[1]:.3f}  ratio {worst[2]:.3f}; "
              f"ratios {got['ratio'].min():.4g} .. {got['ratio'].max():.4g}")
        assert all(got["ratio"][s] == 1.0 for s in range(len(ends)) if not adapt[s]) and (got["ratio"] != 1.0).any()
        host = (host[0], host[1], got["m"], got["v"])


@pytest.mark.parametrize("name", ["four_elements_and_piece_edges_tail_3", "sixty_four_segments", "past_the_workgroup_cap"])
def test_sum_of_squares_is_exact_on_small_integers_and_two_calls_give_the_same_bits(L, name):
    """p in {-2, ..., 2}: every square and every partial sum is an integer far below 2^53, so whatever the order of the adds
    ``norms[2 s]`` is ``float32(sqrt(exact))``.  A second call on equal inputs, its scratch filled with other garbage, writes the
    same bits of every norm and ratio (u^2 included, which is not exact): nothing depends on the schedule."""
    n, ends = TABLES[name]
    ids, adapt = [0] * len(ends), [1] * len(ends)
    (_, g, m, v), _ = case(n, 31)
    p = (FR.sumsq_exact_input(n) * np.where(np.arange(n) % 3 == 0, -1, 1)).astype(np.float32)
    a = run_moments(L, (p, g, m, v), 1e-3, 3, ends, ids, [1.0], [0.0], adapt, fill=float("nan"))
    b = run_moments(L, (p, g, m, v), 1e-3, 3, ends, ids, [1.0], [0.0], adapt, fill=-1e300, seed=50)
    exact = [float((p[lo:hi].astype(np.float64) ** 2).sum()) for lo, hi in LR.segments(ends)]
    want = np.sqrt(np.asarray(exact)).astype(np.float32)
    print(f"{name}: sum p^2 per segment {min(exact):.0f} .. {max(exact):.0f}")
    assert np.array_equal(a["norms"][:, 0].view(np.int32), want.view(np.int32))
    for k in ("norms", "ratio", "m", "v"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_ratio_is_exactly_one_for_zero_weights_a_zero_update_and_an_excluded_tensor(L):
    """Four segments: all-zero weights (P = 0); g = m = 0 and no decay (every u is 0: U = 0); an ordinary tensor that is excluded;
    an ordinary one that adapts.  The first three ratios are 1.0f, bit for bit; the zero sums are +0."""
    ends, ids, adapt = [512, 1024, 1536, 2051], [0, 0, 0, 0], [1, 1, 0, 1]
    (p, g, m, v), _ = case(2051, 77)
    p[:512] = 0.0
    g[512:1024] = 0.0
    m[512:1024] = 0.0
    got = run_moments(L, (p, g, m, v), 1e-3, 2, ends, ids, [1.0], [0.0], adapt)
    print(f"norms {got['norms'].tolist()} ratios {got['ratio'].tolist()}")
    assert got["ratio"][:3].view(np.int32).tolist() == [0x3F800000] * 3 and got["ratio"][3] != 1.0
    assert got["norms"][0, 0] == 0.0 and got["norms"][0, 1] > 0.0 and got["norms"][1, 0] > 0.0 and got["norms"][1, 1] == 0.0
    assert (got["norms"][2:] > 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("name", list(TABLES))
def test_apply_lies_within_the_derived_bound_and_the_average_is_ema_elem(L, name, with_ema):
    """The whole step: moments, then apply with the ratios the first call left on the device.  p within
    ``lamb_ref.apply_expected``'s bound (from the stored moments and the float32 ratios); the average bit for bit what
    ``ss_adam_clip_ema`` makes of the p just written (a launch with lr = 0, g = m = 0, v = 1, which leaves p as it is: the same
    ``ema_elem``).  Excluded segments and adapting ones both move."""
    n, ends = TABLES[name]
    ids, adapt = [k % 2 for k in range(len(ends))], [int(k % 3 != 1) for k in range(len(ends))]
    host, ema = case(n, 900 + len(ends))
    d = 0.9 if with_ema else None
    mom = run_moments(L, host, 4.0, 5, ends, ids, SCALES, DECAYS, adapt)
    p_new, e_new = run_apply(L, host[0], mom["m"], mom["v"], ema if with_ema else None, mom["ratio"], 5, d, ends, ids, SCALES, DECAYS, adapt)
    want, bound = LR.apply_expected(host[0], mom["m"], mom["v"], mom["ratio"], 5, ends, ids, SCALES, DECAYS, lr=LR0, **ADAM_KW)
    print(f"{name} ema={with_ema}: p largest err / bound {within(p_new, want, bound, 'p'):.3f}")
    assert (p_new != host[0]).mean() > 0.5
    if with_ema:
        dev = [torch.from_numpy(a).cuda() for a in (p_new, np.zeros(n, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32), ema)]
        L.call("ss_adam_clip_ema", *(t.data_ptr() for t in dev), n, torch.ones(1, device="cuda").data_ptr(), ADAM[0], ADAM[1], 0.0,
               *BETAS_EPS, 5, d, L.stream())
        torch.cuda.synchronize()
        assert np.array_equal(dev[0].cpu().numpy().view(np.int32), p_new.view(np.int32))  # (the comparator left p alone)
        assert np.array_equal(e_new.view(np.int32), dev[4].cpu().numpy().view(np.int32)) and not np.array_equal(e_new, ema)


@pytest.mark.parametrize("name", ["four_elements_and_piece_edges_tail_3", "past_the_workgroup_cap"])
def test_with_every_ratio_one_and_no_decay_apply_is_adam_clip(L, name):
    """Ratios forced to 1 in device memory, decay 0: p - lr (bc1 quot) against ``ss_adam_clip``'s p - step_size quot on the same
    inputs.  Both lie within their own bounds of the float64 value from the stored moments (``lamb_ref``), whose two forms differ by
    the roundings of ``step_size`` and ``bc1``: 2 ulp of the step."""
    n, ends = TABLES[name]
    ids, adapt = [0] * len(ends), [1] * len(ends)
    host, _ = case(n, 41)
    adam = run_adam(L, host, 4.0, 3)
    mom = run_moments(L, host, 4.0, 3, ends, ids, [1.0], [0.0], adapt)
    p_new, _ = run_apply(L, host[0], mom["m"], mom["v"], None, np.ones(len(ends), np.float32), 3, None, ends, ids, [1.0], [0.0], adapt)
    want_l, bound_l = LR.apply_expected(host[0], mom["m"], mom["v"], np.ones(len(ends)), 3, ends, ids, [1.0], [0.0], lr=LR0, **ADAM_KW)
    want_a, bound_a, t = LR.adam_from_moments_expected(host[0], mom["m"], mom["v"], 3, lr=LR0, **ADAM_KW)
    a, b = within(p_new, want_l, bound_l, "lamb p"), within(adam["p"], want_a, bound_a, "adam p")
    c = within(p_new, adam["p"].astype(np.float64), bound_l + bound_a + 2.0 * LR.f32_ulp(t), "lamb p against adam p")
    print(f"{name}: largest err / bound  lamb {a:.3f}  adam {b:.3f}  lamb against adam {c:.3f}")


def test_entry_points_refuse_bad_arguments_and_write_nothing(L):
    """(tests/test_lamb_cpu.py walks every case on host memory; here the listed ones on device buffers, then the good calls run.)"""
    n = 1031
    host, ema = case(n, 5)
    P, G, M, V, E_ = bufs = [Guarded(a, i) for i, a in enumerate(host + (ema,))]
    ssq = torch.ones(1, device="cuda")
    scratch = scratch_for(L, n, 64, 3.0)
    out = torch.full((3 * 64,), -7.0, device="cuda")
    lib = L.load()
    good = dict(ends=[4, 1028, n], ids=[0, 1, 0], scales=[1.0, 0.5], decays=[0.0, 0.1], adapt=[1, 0, 1])

    def moments(p=P.ptr, step=1, **tk):
        keep, args = table_arrays(**dict(good, **tk))
        return lib.ss_lamb_moments(p, G.ptr, M.ptr, V.ptr, n, ssq.data_ptr(), ADAM[0], ADAM[1], *BETAS_EPS, step, *args,
                                   scratch.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * 128, L.stream())

    def apply(p=P.ptr, e=E_.ptr, step=1, d=0.9, **tk):
        keep, args = table_arrays(**dict(good, **tk))
        return lib.ss_lamb_apply(p, M.ptr, V.ptr, e, n, *BETAS_EPS, step, d, LR0, *args, out.data_ptr() + 4 * 128, L.stream())

    long65 = dict(ends=[4 * (k + 1) for k in range(64)] + [n], ids=[0] * 65, adapt=[1] * 65)
    for bad in (long65, dict(p=P.ptr + 4), dict(decays=[0.0, float("nan")]), dict(step=0)):
        assert moments(**bad) == -1 and apply(**bad) == -1, bad
    for bad in (dict(e=P.ptr), dict(e=P.ptr + 16 * 8), dict(d=float("nan"))):
        assert apply(**bad) == -1, bad
    torch.cuda.synchronize()
    for b in bufs:
        b.check_untouched("a refused call wrote")
    assert bool((out == -7.0).all()) and bool((scratch == 3.0).all()) and float(ssq[0]) == 1.0
    assert moments() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert not np.array_equal(P.values(), host[0]) and not np.array_equal(E_.values(), ema) and not np.array_equal(M.values(), host[2])
    for b in bufs:
        b.check_guards("the good calls")
    G.check_untouched("g")


# ------------------------------------------------------------------------------------------- Trainer against the CPU oracle
@pytest.fixture(scope="module")
def tiny():
    sd = W.make_state_dict(11, 84, 5, True)
    return sd, W.make_inputs(31, B_, T_, 84, 5, ROI)


def lamb_trainer(ss, model, exclude=None, sam_rho=None, **kw):
    tr = ss.Trainer(model, **kw)
    if sam_rho is not None:
        tr.enable_sam(sam_rho)
    tr.enable_lamb(exclude)
    return tr


def oracle_lamb_steps(ss, sd, inputs, steps, groups=(), wd=0.0, sched=lambda step: 1.0, frozen=False, sam_rho=None, engine=MR,
                      model_kw=None):
    """The oracle's ``loss_and_grads`` (twice per step with ``sam_rho``: at ``w`` and at ``w + e``, tests/sam_ref.py), then
    ``lamb_ref.lamb_step`` in float64 with one segment per trained tensor, the default exclusion and the per-step learning rate;
    the weights go back to float32 between steps, as the trainer stores them.  Dropout off.
    -> (state dict after every step, loss of every step, ratios of every step, the tensors' names)."""
    from silent_speech_amd.train import check_lamb_exclude

    X, Lh, R, y = inputs
    host_model = ss.BiGRUClassifier(84, sd["head.4.bias"].numel(), **(model_kw or dict(use_roi=True)))
    _, ids, names = host_model.param_tensor_segments(groups, host_model.cnn_param_range() if frozen else 0)
    adapt = [0 if any(ss.ParamGroup.pattern_matches(p, n) for p in check_lamb_exclude(None)) else 1 for n in names]
    scales = [g.lr_scale for g in groups] + [1.0]
    decays = [wd if g.weight_decay is None else g.weight_decay for g in groups] + [wd]
    ends = list(np.cumsum([sd[k].numel() for k in names]))
    flat = lambda d: np.concatenate([d[k].double().reshape(-1).numpy() for k in names])  # noqa: E731

    def unflat(vec, base):
        out, at = dict(base), 0
        for k in names:
            out[k] = torch.from_numpy(vec[at:at + sd[k].numel()].copy()).reshape(sd[k].shape).float()
            at += sd[k].numel()
        return out

    cur = {k: t.clone() for k, t in sd.items()}
    m, v = np.zeros(ends[-1]), np.zeros(ends[-1])
    out, losses, ratios = [], [], []
    for step in range(1, steps + 1):
        loss, _, g1 = engine.loss_and_grads(cur, X, Lh, R, y)
        p, g = flat(cur), flat(g1)
        if sam_rho is not None:
            _, _, g2 = engine.loss_and_grads(unflat(p + SR.sam_perturbation(p, g, sam_rho, False), cur), X, Lh, R, y)
            g = flat(g2)
        _, r = LR.lamb_step(p, g, m, v, step, ends, ids, scales, decays, adapt, lr=LR0 * sched(step))
        cur = unflat(p, cur)
        out.append({k: t.clone() for k, t in cur.items()})
        losses.append(float(loss))
        ratios.append(r)
    return out, losses, ratios, names


def print_ratios(tr, want, step):
    got = tr.trust_ratios().cpu().numpy()
    rel = np.abs(got - np.asarray(want)) / np.asarray(want)
    print(f"step {step}: trust ratios {got.min():.4g} .. {got.max():.4g}, against the oracle's within {rel.max():.3e} (relative)")
    return got


def test_trainer_against_the_cpu_oracle(ss, tiny):
    """The shapes, settings and tolerances of tests/test_gpu_adamw_groups.py's Trainer test (three steps, dropout off,
    ``weight_decay=1e-2``, a tenth of the learning rate on the CNN, ``no_decay()``, two warm-up steps; ``check_against_oracle``),
    with ``enable_lamb()``: against the oracle's gradients stepped by ``lamb_ref``."""
    sd, (X, Lh, R, y) = tiny
    sched = ss.LrSchedule(warmup_steps=2)
    want, losses, ratios, names = oracle_lamb_steps(ss, sd, (X, Lh, R, y), 3, groups_of(ss), WD, sched)
    model = new_model(ss, sd)
    tr = lamb_trainer(ss, model, dropout=False, weight_decay=WD, param_groups=groups_of(ss), lr_schedule=sched)
    assert tr.lamb_segments() == names == [k for k, _ in model.named_parameters()]
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    for step in range(1, 4):
        loss, _ = tr.step(*dev)
        got = print_ratios(tr, ratios[step - 1], step)
        assert abs(float(loss) - losses[step - 1]) < 1e-4 and tr.current_lr() == LR0 * sched(step)
        assert all((got[s] == 1.0) == (not a) for s, a in enumerate(tr.lamb.adapt)) and (got > 0).all()
        check_against_oracle(model.state_dict(), want[step - 1], f"step {step}")
    # LAMB is visible: the grouped AdamW trainer ends elsewhere by far more than the tolerance
    plain = new_model(ss, sd)
    tp = ss.Trainer(plain, dropout=False, weight_decay=WD, param_groups=groups_of(ss), lr_schedule=sched)
    for _ in range(3):
        tp.step(*dev)
    a, b = plain.state_dict(), model.state_dict()
    moved = max(float((a[k] - b[k]).abs().max()) for k in ("gru.weight_hh_l0", "head.4.weight"))
    print(f"AdamW against LAMB after three steps: max |diff| {moved:.3e}")
    assert moved > 3e-5


def test_trainer_with_sam_and_ema_one_step_against_the_cpu_oracle(ss, tiny):
    sd, (X, Lh, R, y) = tiny
    want, losses, ratios, _ = oracle_lamb_steps(ss, sd, (X, Lh, R, y), 1, sam_rho=0.05)
    model = new_model(ss, sd)
    tr = lamb_trainer(ss, model, dropout=False, sam_rho=0.05, ema_decay=0.9)
    loss, _ = tr.step(X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    print_ratios(tr, ratios[0], 1)
    assert abs(float(loss) - losses[0]) < 1e-4 and float(tr.sam_scal[0]) > float(loss)
    check_against_oracle(model.state_dict(), want[0], "SAM + LAMB step 1")
    assert not torch.equal(tr.ema, model.flat_params) and bool(torch.isfinite(tr.ema).all())


BF16 = dict(use_roi=False, hidden=128, gru_layers=2, precision="bf16")


def test_bf16_trainer_against_the_bf16_oracle(ss):
    """The bf16 engine against ``oracle/model_ref_bf16.py`` stepped by ``lamb_ref``, to the bounds tests/test_gpu_sam.py holds that
    engine's trainer to (those of tests/test_gpu_model_c5.py): the loss within 2e-3, the logits after each step within 0.1 and
    their loss within 2e-2."""
    sd = W.make_state_dict(13, 84, 5, False, hidden=128)
    X, Lh, R, y = W.make_inputs(33, B_, T_, 84, 5, None)
    want, losses, ratios, _ = oracle_lamb_steps(ss, sd, (X, Lh, None, y), 3, engine=MB, model_kw=BF16)
    model = ss.BiGRUClassifier(84, 5, **BF16)
    model.load_state_dict(sd)
    model.cuda().train()
    tr = lamb_trainer(ss, model, dropout=False)
    for step in range(1, 4):
        loss, _ = tr.step(X.cuda(), Lh.cuda(), None, y.cuda())
        print_ratios(tr, ratios[step - 1], step)
        model.eval()
        with torch.no_grad():
            after = model(X.cuda(), Lh, None).cpu()
        model.train()
        ref_after = MB.forward(want[step - 1], X, Lh, None)
        d_logits = float((after - ref_after).abs().max())
        d_loss = abs(float(MR.ce_label_smoothing(after, y)) - float(MR.ce_label_smoothing(ref_after, y)))
        print(f"bf16 step {step}: loss {float(loss):.6f} (oracle {losses[step - 1]:.6f}), logits after the step within {d_logits:.3e}, "
              f"their loss within {d_loss:.3e}")
        assert abs(float(loss) - losses[step - 1]) < 2e-3 and d_logits < 0.1 and d_loss < 2e-2


def test_frozen_cnn_with_step_embedded_keeps_the_frozen_bits(ss, tiny):
    """``freeze_cnn`` + ``step_embedded``: LAMB on ``[n_cnn, n)`` against the oracle with the CNN left out; the CNN range of the
    weights and of the average keeps its exact bits, and the table holds the tensors behind the CNN only."""
    sd, (X, Lh, R, y) = tiny
    want, _, ratios, names = oracle_lamb_steps(ss, sd, (X, Lh, R, y), 2, frozen=True)
    with torch.no_grad():
        roi_e = MR.forward(sd, X, Lh, R, return_intermediates=True)[1]["roi_e"]
    Z = torch.cat([X, roi_e], dim=2).cuda()
    model = new_model(ss, sd)
    tr = lamb_trainer(ss, model, dropout=False, freeze_cnn=True, ema_decay=0.9)
    n_cnn = model.cnn_param_range()
    p0 = model.flat_params.clone()
    assert tr.lamb_segments() == names and not any(k.startswith("roi_cnn.") for k in names) and tr.lamb.n == p0.numel() - n_cnn
    for step in (1, 2):
        tr.step_embedded(Z, Lh.cuda(), y.cuda())
        print_ratios(tr, ratios[step - 1], step)
        check_against_oracle(model.state_dict(), want[step - 1], f"frozen step {step}")
    assert torch.equal(bits(model.flat_params[:n_cnn]), bits(p0[:n_cnn])) and torch.equal(bits(tr.ema[:n_cnn]), bits(p0[:n_cnn]))
    assert not torch.equal(model.flat_params[n_cnn:], p0[n_cnn:]) and not torch.equal(tr.ema[n_cnn:], model.flat_params[n_cnn:])


# -------------------------------------------------------------------------------------------------------------- launch list
@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_trace_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["default", "groups_ema", "frozen", "micro_batches", "bf16_landmarks"])
def test_launch_list_is_the_recorded_one_with_the_two_lamb_entry_points(ss, parent, monkeypatch, name):
    """Against the recorded trace of the same configuration without LAMB (tests/trainer_trace_parent.json, which a trainer without
    ``enable_lamb`` still matches: asserted here): every entry up to the optimiser's as recorded, then ``ss_lamb_moments`` and
    ``ss_lamb_apply`` where the Adam entry stood, on its range, with its sumsq word, betas, eps, step, learning rate and the
    average's decay."""
    plain = parent["steps"][name]
    assert TT.run_config(monkeypatch, name) == plain
    plain_trainer = ss.Trainer

    def trainer_with_lamb(model, **k):  # (run_config builds its trainer as ss.Trainer(model, **keywords))
        tr = plain_trainer(model, **k)
        tr.enable_lamb()
        return tr

    with monkeypatch.context() as m:
        m.setattr(ss, "Trainer", trainer_with_lamb)
        got = TT.run_config(monkeypatch, name)
    adam = plain[-1]
    assert adam[1].startswith("ss_adam") and plain[-2][1] == "ss_sumsq_f32"
    n, a = plain[-2][4][1], adam[4]
    wide = adam[1] != "ss_adam_clip"  # (the two entries that take the average's pointer and decay)
    ema, lr, d = (a[4], a[9], a[14]) if wide else ("null", a[8], 0.0)
    moments, apply = got[-2], got[-1]
    print(f"{name}: {len(plain)} entries without LAMB, {len(got)} with; n {n}, segments {moments[4][14]}, groups {moments[4][17]}")
    assert got[:-2] == plain[:-1], f"{name}: " + first_difference(got[:-2], plain[:-1])
    n_seg, n_groups = moments[4][14], moments[4][17]
    assert moments == ["launch", "ss_lamb_moments", "ss_lamb_moments", "main",
                       ["ptr"] * 4 + [n, "ptr", 1.0, 1.0, 0.9, 0.999, 1e-8, 2, "ptr", "ptr", n_seg, "ptr", "ptr", n_groups] + ["ptr"] * 4]
    assert apply == ["launch", "ss_lamb_apply", "ss_lamb_apply", "main",
                     ["ptr", "ptr", "ptr", ema, n, 0.9, 0.999, 1e-8, 2, d, lr, "ptr", "ptr", n_seg, "ptr", "ptr", n_groups, "ptr", "ptr"]]
    assert 1 < n_seg <= 64 and n_groups == (2 if "groups" in name else 1)


# -------------------------------------------------------------------------------------------------------------------- fit
def test_resumed_fit_lamb_equals_the_uninterrupted_one(ss, tmp_path):
    """The assertion tests/test_gpu_sam.py makes for its resumed fit, on the same synthetic clips: two epochs uninterrupted against
    one epoch, a state file, and a resumed second epoch -- the losses within ``LOSS_BOUND``; the log line and the history carry the
    trust ratios; a run without LAMB, or with another exclusion, cannot resume it."""
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    d = tmp_path
    clips = write_clips(str(d / "clips_npz"), WORDS)
    logs = []
    kw = dict(FIT, epochs=2, log=lambda *a, **k: None)
    hu, h1, h2 = [], [], []
    Hn.fit_lamb(clips, str(d / "u.pt"), state_path=str(d / "u_state.pt"), history=hu, **dict(kw, log=logs.append))
    S = str(d / "r_state.pt")
    Hn.fit_lamb(clips, str(d / "r.pt"), state_path=S, history=h1, **dict(kw, epochs=1))
    Hn.fit_lamb(clips, str(d / "r.pt"), state_path=S, resume=True, history=h2, **kw)
    assert [h["epoch"] for h in hu] == [1, 2] and [h["epoch"] for h in h1] == [1] and [h["epoch"] for h in h2] == [2]
    for a, b in zip(hu, h1 + h2):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {a['epoch']} {key}: uninterrupted {a[key]:.9f} resumed {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
        print(f"epoch {a['epoch']} trust ratio min / median / max: {a['trust_ratio']}")
    for a, b in zip(hu, h1 + h2):
        assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
        lo, med, hi = a["trust_ratio"]
        assert 0.0 < lo <= med <= hi and np.isfinite(hi)
    epochs = [str(line) for line in logs if str(line).startswith("ep ")]
    assert len(epochs) == 2 and all("trust ratio min" in line for line in epochs)
    state = Ck.load_train_state(S)
    assert state["fingerprint"]["lamb"] is True and state["fingerprint"]["lamb_exclude"] == list(ss.no_decay().match)
    assert state["trainer"]["lamb"] is True and state["trainer"]["step_count"] == 6
    with pytest.raises(ValueError, match="lamb"):  # a run without LAMB, or with another exclusion, cannot resume it
        Hn.fit(clips, str(d / "never.pt"), state_path=S, resume=True, **dict(kw, epochs=3))
    with pytest.raises(ValueError, match="lamb_exclude"):
        Hn.fit_lamb(clips, str(d / "never.pt"), ["gru."], state_path=S, resume=True, **dict(kw, epochs=3))
