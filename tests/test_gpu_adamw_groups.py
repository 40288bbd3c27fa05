"""GPU: the grouped AdamW step -- ``ss_adamw_clip_groups`` through the C ABI, ``Trainer(weight_decay=, param_groups=,
lr_schedule=)`` against the CPU oracle, its launch list and state, and ``harness.fit`` with a warm-up and a plateau schedule.

Bounds.  Against ``ss_adam_clip`` / ``ss_adam_clip_ema`` (one launch per segment on its sub-range, ``lr = lr_G``, the same sumsq
word; with decays: on ``p`` multiplied on the host by ``decay_G`` in NumPy float32, one rounded product): equal bits.  Against
float64: the bounds derived in tests/adamw_ref.py.  The average of a three-element tail segment: ``optim_ref.ema_expected``'s 2
ulp.  Trainer against the oracle: the figures tests/test_gpu_model.py holds the parameters after Adam to (atol 3e-6, 6.1e-4 for
pool.score.bias, rtol 2e-5 on ``weights.reduce_tensor``).  Resumed ``fit`` against the uninterrupted one: ``LOSS_BOUND`` of
tests/test_gpu_ema_resume.py.  Every buffer a launch writes has ``GUARD`` words of NaN patterns on BOTH sides, checked afterwards.

Run on the MI355X box with ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest
import torch

import adamw_ref as AR
import flat_ref as FR
import launch_trace as LT
import optim_ref as OR
import weights as W
from gpu_support import L, WORDS, ss, write_clips  # noqa: F401
from oracle import model_ref as MR
from test_gpu_ema_resume import ADAM, B_, FIT, LOSS_BOUND, ROI, T_, bits

pytestmark = pytest.mark.gpu

GUARD = 8  # words of NaN patterns in front of and behind every buffer (32 bytes: the buffer stays 16-byte aligned)
LR = ADAM[2]
SWEEP = 2048 * 256 * 4  # elements one sweep of the capped grid covers
NS = [1, 2, 3, 4, 5, 6, 1027, SWEEP - 1, SWEEP, SWEEP + 7, 4 * SWEEP + 5]


# ---------------------------------------------------------------------------------------------------------------- the kernel
class Guarded:
    """A device buffer of ``values`` (float32 NumPy) with NaN guard words on both sides."""

    def __init__(self, values, seed):
        n = values.size
        self.n, self.back = n, GUARD + n
        host = (0x7FC00000 + ((np.arange(2 * GUARD + (n + 3) // 4 * 4) * 2654435761 + seed) % 0x3FFFFF)).astype(np.int32)
        host[GUARD:GUARD + n] = values.view(np.int32)
        self.host = torch.from_numpy(host)
        self.dev = self.host.cuda().view(torch.float32)
        self.ptr = self.dev.data_ptr() + 4 * GUARD

    def values(self):
        return self.dev[GUARD:GUARD + self.n].cpu().numpy()

    def check_guards(self, what):
        now = bits(self.dev)
        assert torch.equal(now[:GUARD], self.host[:GUARD]), f"{what}: guard words in front"
        assert torch.equal(now[self.back:], self.host[self.back:]), f"{what}: guard words behind"

    def check_untouched(self, what):
        assert torch.equal(bits(self.dev), self.host), what


def table_arrays(ends, ids, scales, decays):
    import ctypes as C

    arrs = ((C.c_long * len(ends))(*ends), (C.c_int * len(ids))(*ids), (C.c_float * len(scales))(*scales), (C.c_float * len(decays))(*decays))
    return arrs, (C.addressof(arrs[0]), C.addressof(arrs[1]), len(ends), C.addressof(arrs[2]), C.addressof(arrs[3]), len(scales))


def run_grouped(L, host, ema, sumsq, step, d, ends, ids, scales, decays, seed=0):
    """One ``ss_adamw_clip_groups`` launch on guarded copies of the host arrays (p, g, m, v) and of ``ema`` (or None) -> dict of
    the new p, m, v, ema; asserts that the guards, g and the sumsq word are as they were."""
    n = host[0].size
    bufs = [Guarded(a, seed + i) for i, a in enumerate(host)]
    e = None if ema is None else Guarded(ema, seed + 9)
    ssq = torch.tensor([sumsq], dtype=torch.float32).cuda()
    keep, args = table_arrays(ends, ids, scales, decays)
    P, G, M, V = bufs
    L.call("ss_adamw_clip_groups", P.ptr, G.ptr, M.ptr, V.ptr, None if e is None else e.ptr, n, ssq.data_ptr(), *ADAM, step,
           0.0 if d is None else d, *args, L.stream())
    torch.cuda.synchronize()
    for b, name in zip(bufs + ([e] if e is not None else []), "pgmve"):
        b.check_guards(name)
    G.check_untouched("g")
    assert float(ssq[0]) == float(np.float32(sumsq))
    return dict(p=P.values(), m=M.values(), v=V.values(), ema=None if e is None else e.values())


def run_per_segment(L, host, ema, sumsq, step, d, ends, ids, scales, decays=None, plain_tail=False):
    """The oracle: one ``ss_adam_clip`` (``ss_adam_clip_ema`` with ``ema``) launch per segment on its sub-range, ``lr = lr_G`` as
    the entry point is specified to take it, the same sumsq word; with ``decays`` on p multiplied by ``decay_G`` in NumPy float32
    first.  ``plain_tail``: the last segment goes through ``ss_adam_clip`` even with ``ema``, whose range then stays as it was."""
    p, g, m, v = host
    if decays is not None:
        dec = AR.per_element(ends, ids, [AR.group_scalars(LR, s, w, step)["decay"] for s, w in zip(scales, decays)]).astype(np.float32)
        assert dec.dtype == np.float32 and p.dtype == np.float32
        p = p * dec  # float32 x float32 -> float32: one rounded product
    dev = [torch.from_numpy(a.copy()).cuda() for a in (p, g, m, v)] + ([] if ema is None else [torch.from_numpy(ema.copy()).cuda()])
    ssq = torch.tensor([sumsq], dtype=torch.float32).cuda()
    lo = 0
    for s, (hi, G) in enumerate(zip(ends, ids)):
        lr_g = AR.group_scalars(LR, scales[G], 0.0, step)["lr"]
        ptrs = [t.data_ptr() + 4 * lo for t in dev]
        if ema is None or (plain_tail and s == len(ends) - 1):
            L.call("ss_adam_clip", *ptrs[:4], hi - lo, ssq.data_ptr(), ADAM[0], ADAM[1], lr_g, *ADAM[3:], step, L.stream())
        else:
            L.call("ss_adam_clip_ema", *ptrs, hi - lo, ssq.data_ptr(), ADAM[0], ADAM[1], lr_g, *ADAM[3:], step, d, L.stream())
        lo = hi
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in dev]
    return dict(p=out[0], m=out[2], v=out[3], ema=None if ema is None else out[4])


def same_bits(got, want, keys, what, sl=slice(None)):
    for k in keys:
        a, b = got[k][sl].view(np.int32), want[k][sl].view(np.int32)
        assert np.array_equal(a, b), (what, k, int((a != b).sum()), int(np.flatnonzero(a != b)[0]))


def case(n, seed):
    p, g, m, v = FR.optimiser_case(n, seed)
    ema = np.random.default_rng(seed + 1).standard_normal(n).astype(np.float32)
    return (p, g, m, v), ema


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("n", NS)
def test_one_plain_segment_writes_the_bits_of_the_existing_kernels(L, n, with_ema):
    """One segment of a group {scale 1, decay 0}: p * 1.0f is exact and lr_G is lr, so p, m, v (and the average) are the bits of
    ``ss_adam_clip`` (``ss_adam_clip_ema``).  Steps 1 and 7 from nonzero moments, the second one clipped; sizes without a
    quad, with every ``n & 3``, on both sides of one sweep of the capped grid and just past four."""
    host, ema = case(n, 200 + n)
    ema = ema if with_ema else None
    d = 0.9 if with_ema else None
    for step, sumsq in ((1, 1e-3), (7, 4.0)):
        got = run_grouped(L, host, ema, sumsq, step, d, [n], [0], [1.0], [0.0], seed=step)
        want = run_per_segment(L, host, ema, sumsq, step, d, [n], [0], [1.0])
        same_bits(got, want, "pmv", (n, step))
        if with_ema:
            same_bits(got, want, ["ema"], (n, step))
        assert not np.array_equal(got["p"], host[0])  # (the step did something)
        host = (got["p"], host[1], got["m"], got["v"])
        ema = got["ema"]


SCALES = [1.0, 0.1, 0.0]
TABLES = {
    "a_64_quads": (256, [4 * (k + 1) for k in range(64)]),
    "b_inside_a_wave": (1031, [4, 8, 256, 260, 1024, 1028, 1031]),
    "c_around_the_sweep": (SWEEP + 7, [SWEEP - 4, SWEEP, SWEEP + 4, SWEEP + 7]),
    "d_quad_then_two_million": (4 + 2000000, [4, 4 + 2000000]),
    "e_last_is_a_quad_and_a_tail": (1030, [4, 512, 1024, 1030]),
}


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("name", list(TABLES))
def test_segment_edges_bit_for_bit(L, name, with_ema):
    """All decays 0, three groups with scales {1, 0.1, 0} dealt to the segments in turn: every segment gets the bits of one
    ``ss_adam_clip`` (``ss_adam_clip_ema``) launch on its sub-range.  (b) has a boundary inside one wave's span and a tail segment
    of ``n & 3 = 3`` elements of its own: that one is checked against ``ss_adam_clip`` for p, m, v and against
    ``optim_ref.ema_expected`` for the average.  (e) ends in a segment of one quad and
    ``n & 3 = 2`` elements, in the group of scale 1."""
    n, ends = TABLES[name]
    ids = [k % 3 for k in range(len(ends))]
    host, ema = case(n, 300 + len(ends))
    ema, d = (ema, 0.9) if with_ema else (None, None)
    tail3 = with_ema and name == "b_inside_a_wave"
    for step, sumsq in ((1, 1e-3), (7, 4.0)):
        got = run_grouped(L, host, ema, sumsq, step, d, ends, ids, SCALES, [0.0] * 3, seed=step)
        want = run_per_segment(L, host, ema, sumsq, step, d, ends, ids, SCALES, plain_tail=tail3)
        same_bits(got, want, "pmv", (name, step))
        if with_ema:
            body = slice(0, ends[-2]) if tail3 else slice(None)
            same_bits(got, want, ["ema"], (name, step), body)
            if tail3:
                t = slice(ends[-2], n)
                e_want, bound = OR.ema_expected(ema[t], got["p"][t], d)
                assert (np.abs(got["ema"][t].astype(np.float64) - e_want) <= bound).all() and not np.array_equal(got["ema"][t], ema[t])
        # scale 0 (group 2): p keeps its bits, m and v still move
        z = AR.per_element(ends, ids, [0, 0, 1]).astype(bool)
        assert z.any() == (len(ends) > 2)  # ((d) has two segments: groups 0 and 1 only)
        assert np.array_equal(got["p"][z].view(np.int32), host[0][z].view(np.int32))
        assert not z.any() or (not np.array_equal(got["m"][z], host[2][z]) and not np.array_equal(got["v"][z], host[3][z]))
        assert (got["p"][~z] != host[0][~z]).mean() > 0.5
        host = (got["p"], host[1], got["m"], got["v"])
        ema = got["ema"]


DECAYS = [0.0, 1e-3, 0.1]


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
def test_decay_is_one_rounded_product_in_front_of_the_update(L, with_ema):
    """Table (b), decays {0, 1e-3, 0.1}: the bits of ``ss_adam_clip`` per segment on ``p * decay_G`` taken on the host in float32.
    A product contracted into the update behind it (an fma on the unrounded p * decay) would differ in the last bit of many
    elements.  The same launch against float64 (``adamw_ref``: torch's decoupled AdamW) within the derived bounds.
    Scale 0 (the third group): ``p`` becomes ``float32(p * decay_G)`` with decay_G = 1 - 0 * 0.1 = 1 -- it keeps its bits up to the
    decay product, which here is exact --; m and v still move."""
    n, ends = TABLES["b_inside_a_wave"]
    ids = [k % 3 for k in range(len(ends))]
    host, ema = case(n, 77)
    ema, d = (ema, 0.9) if with_ema else (None, None)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, sumsq in ((1, 1e-3), (7, 4.0)):
        got = run_grouped(L, host, ema, sumsq, step, d, ends, ids, SCALES, DECAYS, seed=step)
        want = run_per_segment(L, host, None, sumsq, step, None, ends, ids, SCALES, decays=DECAYS)
        same_bits(got, want, "pmv", ("decay", step))
        want64, bound = AR.adamw_groups_expected(*host, np.float32(sumsq), step, ends, ids, SCALES, DECAYS, lr=LR, max_norm=ADAM[1],
                                                 beta1=ADAM[3], beta2=ADAM[4], eps=ADAM[5], grad_scale=ADAM[0])
        for k in "pmv":
            err = np.abs(got[k].astype(np.float64) - want64[k])
            worst[k] = max(worst[k], float((err / bound[k]).max()))
            assert (err <= bound[k]).all(), (k, step, worst[k])
        if with_ema:
            e_want, e_bound = OR.ema_expected(ema, got["p"], d)
            assert (np.abs(got["ema"].astype(np.float64) - e_want) <= e_bound).all()
        # the decay did act: group 1's weights differ from the undecayed step's, group 0's (decay 0) do not
        plain = run_per_segment(L, host, None, sumsq, step, None, ends, ids, SCALES)
        g0, g1 = (AR.per_element(ends, ids, sel).astype(bool) for sel in ([1, 0, 0], [0, 1, 0]))
        assert np.array_equal(got["p"][g0], plain["p"][g0]) and (got["p"][g1] != plain["p"][g1]).mean() > 0.1
        z = AR.per_element(ends, ids, [0, 0, 1]).astype(bool)
        assert AR.group_scalars(LR, 0.0, 0.1, step)["decay"] == 1.0 and np.array_equal(got["p"][z], host[0][z])
        assert not np.array_equal(got["m"][z], host[2][z])
        host = (got["p"], host[1], got["m"], got["v"])
        ema = got["ema"]
    print(f"adamw_clip_groups against float64: largest err / bound  m {worst['m']:.4f}  v {worst['v']:.4f}  p {worst['p']:.4f}")


def test_grouped_entry_point_refuses_bad_arguments_and_writes_nothing(L):
    """(tests/test_adamw_groups_cpu.py walks every case on host memory; here a few on device buffers, then the good call runs.)"""
    n = 1031
    host, ema = case(n, 5)
    bufs = [Guarded(a, i) for i, a in enumerate(host + (ema,))]
    ssq = torch.ones(1, device="cuda")
    lib = L.load()

    def status(ends, ids, scales, decays, p=bufs[0].ptr, e=bufs[4].ptr, n_=n):
        keep, args = table_arrays(ends, ids, scales, decays)
        return lib.ss_adamw_clip_groups(p, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, e, n_, ssq.data_ptr(), *ADAM, 1, 0.9, *args, L.stream())

    good = ([4, 1028, n], [0, 1, 0], [1.0, 0.5], [0.0, 0.1])
    assert status([4, 1026, n], *good[1:]) == -1 and status([4, 4, n], *good[1:]) == -1 and status([4, 1028, n - 1], *good[1:]) == -1
    assert status(good[0], [0, 2, 0], *good[2:]) == -1 and status(*good[:2], [1.0, -0.5], good[3]) == -1
    assert status(*good[:3], [0.0, float("nan")]) == -1 and status(*good, e=bufs[0].ptr) == -1 and status(*good, p=bufs[0].ptr + 4) == -1
    torch.cuda.synchronize()
    for b in bufs:
        b.check_untouched("a refused call wrote")
    assert status(*good) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(bufs[0].values(), host[0]) and not np.array_equal(bufs[4].values(), ema)
    for b in bufs:
        b.check_guards("the good call")


# ---------------------------------------------------------------------------------------------------------------- Trainer
WD = 1e-2


def groups_of(ss, frozen=False):
    return ([] if frozen else [ss.ParamGroup("roi_cnn.", lr_scale=0.1)]) + [ss.no_decay()]


def new_model(ss, sd):
    m = ss.BiGRUClassifier(84, 5, use_roi=True)
    m.load_state_dict(sd)
    return m.cuda().train()


def oracle_steps(ss, sd, inputs, groups, schedule, steps, frozen):
    """``oracle/model_ref.py`` stepped by ``clip_grad_norm_`` + ``torch.optim.AdamW`` with the same groups and the same per-step lr
    (dropout off).  ``frozen``: the ROI CNN has ``requires_grad=False`` -- no gradient, no part in the norm, no update.
    -> the state dict after every step."""
    X, Lh, R, y = inputs
    host_model = ss.BiGRUClassifier(84, 5, use_roi=True)
    n_cnn = host_model.cnn_param_range() if frozen else 0
    _, _, members = host_model.param_segments(groups, n_cnn)
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
    scales = [g.lr_scale for g in groups] + [1.0]
    decays = [WD if g.weight_decay is None else g.weight_decay for g in groups] + [WD]
    live = [(names, sc, wd) for names, sc, wd in zip(members, scales, decays) if names]
    opt = torch.optim.AdamW([dict(params=[params[k] for k in names], lr=LR * sc, weight_decay=wd) for names, sc, wd in live], lr=LR)
    out = []
    for step in range(1, steps + 1):
        _, _, grads = MR.loss_and_grads({k: p.detach() for k, p in params.items()}, X, Lh, R, y)
        trained = [k for names, _, _ in live for k in names]
        for k in trained:
            params[k].grad = grads[k].clone()
        torch.nn.utils.clip_grad_norm_([params[k] for k in trained], 1.0)
        for pg, (_, sc, _) in zip(opt.param_groups, live):
            pg["lr"] = LR * schedule(step) * sc
        opt.step()
        out.append({k: p.detach().clone() for k, p in params.items()})
    return out


def check_against_oracle(got_sd, want_sd, what):
    for k, v in got_sd.items():
        atol = 6.1e-4 if k == "pool.score.bias" else 3e-6  # tests/test_gpu_model.py, the parameters after Adam
        got, want = W.reduce_tensor(v.detach().cpu()), W.reduce_tensor(want_sd[k])
        print(f"{what} {k}: max |diff| {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, atol=atol, rtol=2e-5, err_msg=f"{what} {k}")


@pytest.fixture(scope="module")
def tiny():
    sd = W.make_state_dict(11, 84, 5, True)
    return sd, W.make_inputs(31, B_, T_, 84, 5, ROI)


def test_trainer_with_groups_decay_and_warmup_against_the_cpu_oracle(ss, tiny):
    """Three steps, dropout off: ``weight_decay=1e-2``, a tenth of the learning rate on the CNN, no decay on biases and LayerNorm,
    two warm-up steps -- against ``clip_grad_norm_`` + ``torch.optim.AdamW`` with the same groups on the CPU oracle."""
    sd, (X, Lh, R, y) = tiny
    sched = ss.LrSchedule(warmup_steps=2)
    want = oracle_steps(ss, sd, (X, Lh, R, y), groups_of(ss), sched, 3, frozen=False)
    model = new_model(ss, sd)
    tr = ss.Trainer(model, dropout=False, weight_decay=WD, param_groups=groups_of(ss), lr_schedule=sched)
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    for step in range(1, 4):
        tr.step(*dev)
        assert tr.current_lr() == LR * sched(step) and tr.step_count == step
        check_against_oracle(model.state_dict(), want[step - 1], f"step {step}")
    # the decay and the CNN's scale are visible: a plain Trainer ends elsewhere by far more than the tolerance
    plain = new_model(ss, sd)
    tp = ss.Trainer(plain, dropout=False, lr_schedule=sched)
    for _ in range(3):
        tp.step(*dev)
    a, b = plain.state_dict(), model.state_dict()
    assert float((a["gru.weight_hh_l0"] - b["gru.weight_hh_l0"]).abs().max()) > 3e-5
    assert float((a["roi_cnn.net.0.weight"] - b["roi_cnn.net.0.weight"]).abs().max()) > 3e-5


def test_frozen_trainer_with_groups_against_the_cpu_oracle(ss, tiny):
    """The same with ``freeze_cnn=True`` + ``step_embedded`` (the embeddings are the oracle's own): the CNN range keeps its exact
    bits, the rest matches the oracle with the CNN's ``requires_grad=False``."""
    sd, (X, Lh, R, y) = tiny
    sched = ss.LrSchedule(warmup_steps=2)
    want = oracle_steps(ss, sd, (X, Lh, R, y), groups_of(ss, True), sched, 3, frozen=True)
    with torch.no_grad():
        roi_e = MR.forward(sd, X, Lh, R, return_intermediates=True)[1]["roi_e"]
    Z = torch.cat([X, roi_e], dim=2).cuda()
    model = new_model(ss, sd)
    tr = ss.Trainer(model, dropout=False, freeze_cnn=True, weight_decay=WD, param_groups=groups_of(ss, True), lr_schedule=sched,
                    ema_decay=0.9)
    n_cnn = model.cnn_param_range()
    p0 = model.flat_params.clone()
    assert tr.table.n == model.flat_params.numel() - n_cnn
    for step in range(1, 4):
        tr.step_embedded(Z, Lh.cuda(), y.cuda())
        check_against_oracle(model.state_dict(), want[step - 1], f"frozen step {step}")
    assert torch.equal(bits(model.flat_params[:n_cnn]), bits(p0[:n_cnn])) and torch.equal(bits(tr.ema[:n_cnn]), bits(p0[:n_cnn]))
    assert not torch.equal(model.flat_params[n_cnn:], p0[n_cnn:]) and not torch.equal(tr.ema[n_cnn:], model.flat_params[n_cnn:])
    assert all(torch.equal(want[-1][k], sd[k]) for k in sd if k.startswith("roi_cnn."))
    with pytest.raises(ValueError, match="frozen ROI CNN"):
        ss.Trainer(new_model(ss, sd), freeze_cnn=True, param_groups=groups_of(ss))


def test_launch_list_with_and_without_groups(ss, tiny):
    """With groups a step's launches are the plain step's with ``ss_adam_clip`` replaced by ONE ``ss_adamw_clip_groups`` whose n is
    the trainable range; with ``ema_decay`` it replaces ``ss_adam_clip_ema``.  Without the new arguments -- and with a schedule
    alone -- the list is the plain one (tests/test_gpu_launch_trace.py pins that one to the recorded parent)."""
    sd, (X, Lh, R, y) = tiny
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    mp = pytest.MonkeyPatch()

    def trace(**kw):
        model = new_model(ss, sd)
        tr = ss.Trainer(model, **kw)
        tr.step(*dev)
        return LT.launches(LT.traced(mp, model, lambda: tr.step(*dev))), model

    def shape(log):  # entry point, tag, stream -- and the arguments of everything but the optimiser's launch
        return [(e[1], e[2], e[3], None if e[1].startswith("ss_adam") else e[4]) for e in log]

    plain, model = trace()
    n = model.flat_params.numel()
    names = [e[1] for e in plain]
    assert names.count("ss_adam_clip") == 1 and names[-1] == "ss_adam_clip" and "ss_adamw_clip_groups" not in names
    sched, _ = trace(lr_schedule=ss.LrSchedule(warmup_steps=5))
    assert shape(sched) == shape(plain) and [e[4][:8] for e in sched[-1:]] == [plain[-1][4][:8]]
    assert sched[-1][4][8] == LR * 1.0 * 0.4 != plain[-1][4][8] == LR  # the lr of step 2 of a five-step warm-up
    grouped, _ = trace(weight_decay=WD, param_groups=groups_of(ss))
    want = [("ss_adamw_clip_groups", "ss_adamw_clip_groups") + s[2:] if s[0] == "ss_adam_clip" else s for s in shape(plain)]
    assert shape(grouped) == want
    a = grouped[-1][4]
    assert a[4] == "null" and a[5] == n and a[17] == 15 and a[20] == 3 and a[15:17] == ["ptr", "ptr"] and a[18:20] == ["ptr", "ptr"]
    decay_only, _ = trace(weight_decay=WD)
    assert shape(decay_only) == want and decay_only[-1][4][17] == 1 and decay_only[-1][4][20] == 1
    ema_plain, _ = trace(ema_decay=0.9)
    ema_grouped, _ = trace(ema_decay=0.9, param_groups=[ss.no_decay()])
    assert [e[1] for e in ema_plain][-1] == "ss_adam_clip_ema"
    assert shape(ema_grouped) == [("ss_adamw_clip_groups", "ss_adamw_clip_groups") + s[2:] if s[0] == "ss_adam_clip_ema" else s
                                  for s in shape(ema_plain)]
    assert ema_grouped[-1][4][4] == "ptr" and ema_grouped[-1][4][14] == ema_plain[-1][4][14]  # the average, the step's decay


def test_trainer_state_keys_and_round_trip(ss, tiny):
    sd, (X, Lh, R, y) = tiny
    dev = (X.cuda(), Lh.cuda(), R.cuda(), y.cuda())
    old_keys = {"m", "v", "ema", "step_count", "ema_decay", "ema_warmup", "betas", "eps", "lr", "max_norm", "numel"}
    assert set(ss.Trainer(new_model(ss, sd)).state_dict()) == old_keys  # unchanged without the new arguments
    sched = ss.LrSchedule(warmup_steps=2, decay="cosine", total_steps=10)
    kw = dict(dropout=False, weight_decay=WD, param_groups=groups_of(ss), lr_schedule=sched)
    m1 = new_model(ss, sd)
    t1 = ss.Trainer(m1, **kw)
    t1.lr_scale = 0.5  # (as a plateau would have set it)
    for _ in range(2):
        t1.step(*dev)
    state = t1.state_dict()
    assert set(state) == old_keys | {"weight_decay", "param_groups", "lr_schedule", "lr_scale"}
    assert state["weight_decay"] == WD and state["lr_scale"] == 0.5 and state["lr_schedule"] == sched.plain()
    assert state["param_groups"] == t1.table.plain() and len(state["param_groups"]["seg_end"]) == 15
    from silent_speech_amd import checkpoint as Ck

    m2 = new_model(ss, {k: v.cpu() for k, v in m1.state_dict().items()})
    t2 = ss.Trainer(m2, **kw)
    t2.load_state_dict(Ck._plain(state))  # (as read from a file: lists for tuples, CPU tensors)
    assert t2.lr_scale == 0.5 and t2.step_count == 2 and t2.current_lr(3) == t1.current_lr(3) == LR * 0.5 * sched(3)
    l1, l2 = float(t1.step(*dev)[0]), float(t2.step(*dev)[0])
    assert abs(l1 - l2) <= LOSS_BOUND
    assert float((m1.flat_params - m2.flat_params).abs().max()) <= 1e-6
    # another table -- other groups, another decay, none at all -- is refused, in both directions
    for other in (dict(kw, weight_decay=1e-3), dict(kw, param_groups=[ss.no_decay()]), dict(dropout=False)):
        with pytest.raises(ValueError, match="param_groups"):
            ss.Trainer(new_model(ss, sd), **other).load_state_dict(state)
    with pytest.raises(ValueError, match="param_groups"):
        t2.load_state_dict(ss.Trainer(new_model(ss, sd)).state_dict())


# -------------------------------------------------------------------------------------------------------------------- fit
def test_fit_lr_follows_the_schedules_and_a_resumed_run_reproduces_it(ss, tmp_path):
    """Four epochs with a plateau of patience 0 (every epoch that does not improve the validation accuracy halves the rate) and a
    schedule with warm-up and a cosine decay: uninterrupted (``total_steps=None``: ``fit`` fills in 4 epochs x 3 batches), and
    stopped after epoch 2 and resumed (``total_steps=12`` spelled out, since the first leg is asked for two epochs only)."""
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    d = tmp_path
    clips = write_clips(str(d / "clips_npz"), WORDS)
    quiet = lambda *a, **k: None  # noqa: E731
    kw = dict(FIT, epochs=4, patience=9, weight_decay=WD, param_groups=[ss.no_decay()], log=quiet)
    total = ss.LrSchedule(warmup_steps=4, decay="cosine", final_frac=0.1, total_steps=12)
    hu, h1, h2, logs = [], [], [], []
    Hn.fit(clips, str(d / "u.pt"), state_path=str(d / "u_state.pt"), history=hu, **dict(kw, log=logs.append),
           lr_plateau=ss.PlateauSchedule(patience=0), lr_schedule=ss.LrSchedule(warmup_steps=4, decay="cosine", final_frac=0.1))
    S = str(d / "r_state.pt")
    Hn.fit(clips, str(d / "r.pt"), state_path=S, history=h1, **dict(kw, epochs=2), lr_plateau=ss.PlateauSchedule(patience=0), lr_schedule=total)
    mid = Ck.load_train_state(S)
    Hn.fit(clips, str(d / "r.pt"), state_path=S, resume=True, history=h2, **kw, lr_plateau=ss.PlateauSchedule(patience=0), lr_schedule=total)
    assert [h["epoch"] for h in hu] == [1, 2, 3, 4] and [h["epoch"] for h in h1] == [1, 2] and [h["epoch"] for h in h2] == [3, 4]
    # 38 training clips in batches of 16: three steps per epoch
    assert Ck.load_train_state(str(d / "u_state.pt"))["trainer"]["step_count"] == 12
    # the two rules: lr of the epoch's last step = base x plateau scale during the epoch x schedule(step count)
    plateau, scale, reductions = ss.PlateauSchedule(patience=0), 1.0, 0
    for h in hu:
        want = FIT["lr"] * scale * total(3 * h["epoch"])
        print(f"epoch {h['epoch']}: lr {h['lr']:.9e} (plateau scale {scale:g}), val_acc {h['val_acc']:.3f}")
        assert h["lr"] == want, (h, want)
        reductions += plateau.step(h["val_acc"])
        scale = plateau.scale
    assert hu[0]["lr"] == FIT["lr"] * 0.75  # still warming up at the end of epoch 1: step 3 of 4
    assert sum("lr plateau" in str(line) for line in logs) == reductions
    # resumed: the lr of every epoch exactly, the losses within the atomic-order noise
    for a, b in zip(hu, h1 + h2):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {a['epoch']} {key}: uninterrupted {a[key]:.9f} resumed {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
    for a, b in zip(hu, h1 + h2):
        assert a["lr"] == b["lr"], (a, b)
        assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
    # the file carries the plateau's state and the fingerprint the four settings
    assert set(mid["plateau"]) == {"best", "bad", "scale"} and mid["epoch"] == 2 and mid["trainer"]["lr_scale"] == mid["plateau"]["scale"]
    fp = mid["fingerprint"]
    assert fp["weight_decay"] == WD and fp["lr_plateau"]["patience"] == 0 and fp["lr_schedule"]["total_steps"] == 12
    assert fp["param_groups"] == [dict(match=["*bias", "gru.bias_", "head.0."], lr_scale=1.0, weight_decay=0.0)]
    assert Ck.load_train_state(str(d / "u_state.pt"))["fingerprint"]["lr_schedule"]["total_steps"] is None
    # another weight_decay cannot resume the run
    with pytest.raises(ValueError, match="weight_decay"):
        Hn.fit(clips, str(d / "never.pt"), state_path=S, resume=True, **dict(kw, weight_decay=1e-3),
               lr_plateau=ss.PlateauSchedule(patience=0), lr_schedule=total)
    # a run without the new arguments has neither the keys nor history["lr"]
    plain_h, Sp = [], str(d / "p_state.pt")
    Hn.fit(clips, str(d / "p.pt"), state_path=Sp, history=plain_h, **dict(FIT, epochs=1, log=quiet))
    plain = Ck.load_train_state(Sp)
    assert "plateau" not in plain and set(plain["fingerprint"]) == set(Ck.FINGERPRINT_FIELDS) and "lr" not in plain_h[0]
    assert "lr_scale" not in plain["trainer"] and "param_groups" not in plain["trainer"]
