"""CPU: the host side of the grouped AdamW step and of the learning-rate schedules -- the NumPy restatement
(tests/adamw_ref.py) against ``clip_grad_norm_`` + ``torch.optim.AdamW`` with real param groups; the segment tables of real
models; ``LrSchedule`` values; ``PlateauSchedule`` against ``torch.optim.lr_scheduler.ReduceLROnPlateau``; the run fingerprint;
the ABI of ``ss_adamw_clip_groups`` and the argument checks that return before any launch.  No device is touched.
(``Trainer`` needs a device to exist: its ``state_dict`` is checked in tests/test_gpu_adamw_groups.py.)"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import adamw_ref as AR
import flat_ref as FR
import optim_ref as OR
from test_ema_resume_cpu import declared_arguments


# ------------------------------------------------------------------------------------------------------------ the reference
def test_adamw_ref_against_torch_clip_and_adamw_param_groups():
    """Three steps of ``adamw_ref.adamw_groups_step`` (float64) against ``clip_grad_norm_`` + ``torch.optim.AdamW`` with two real
    param groups of different lr and decay, from nonzero moments: the same arithmetic in another order, 1e-12 relative (the
    round-off tests/test_ema_resume_cpu.py allows plain Adam).  The two groups interleave: three segments."""
    rng = np.random.default_rng(11)
    lr, scales, decays = 3e-4, [1.0, 0.1], [1e-2, 0.3]
    seg_end, seg_group = [400, 700, 1000], [0, 1, 0]
    p0, _, m0, v0 = (a.astype(np.float64) for a in FR.optimiser_case(1000, 4))
    grads = [rng.normal(size=1000) * s for s in (0.2, 0.001, 3.0)]  # clipped, not clipped (norm 0.03), clipped hard
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    idx = [np.r_[0:400, 700:1000], np.r_[400:700]]
    tps = [torch.nn.Parameter(torch.from_numpy(p0[i].copy())) for i in idx]
    opt = torch.optim.AdamW([dict(params=[tp], lr=lr * sc, weight_decay=wd) for tp, sc, wd in zip(tps, scales, decays)], lr=lr)
    for tp, i in zip(tps, idx):  # (nonzero moments: as if three steps had been taken; the step numbers below carry on from there)
        opt.state[tp] = dict(step=torch.tensor(3.0), exp_avg=torch.from_numpy(m0[i].copy()), exp_avg_sq=torch.from_numpy(v0[i].copy()))
    for step, g in enumerate(grads, 4):
        total = AR.adamw_groups_step(p, g.copy(), m, v, step, seg_end, seg_group, scales, decays, lr=lr)
        for tp, i in zip(tps, idx):
            tp.grad = torch.from_numpy(g[i].copy())
        t_total = torch.nn.utils.clip_grad_norm_(tps, 1.0)
        opt.step()
        assert abs(total - float(t_total)) <= 1e-12 * total
        for tp, i in zip(tps, idx):
            assert np.abs(p[i] - tp.detach().numpy()).max() <= 1e-12 * np.abs(p).max()
            assert np.abs(m[i] - opt.state[tp]["exp_avg"].numpy()).max() <= 1e-12 * np.abs(m).max()
            assert np.abs(v[i] - opt.state[tp]["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(v).max()
    # the steps moved the weights, the decay is visible (0.3 * 3e-5 * 3 steps of |p| ~ 1 against Adam's ~3e-5 per step), and the
    # groups differ
    assert np.abs(p - p0).max() > 1e-4
    q, mq, vq = p0.copy(), m0.copy(), v0.copy()
    for step, g in enumerate(grads, 4):
        AR.adamw_groups_step(q, g.copy(), mq, vq, step, seg_end, seg_group, scales, [0.0, 0.0], lr=lr)
    assert np.abs(p - q)[idx[1]].max() > 1e-5 and np.array_equal(m, mq) and np.array_equal(v, vq)  # decay is no part of the gradient


def test_adamw_expected_is_the_step_with_float32_scalars_and_bounds_a_few_ulp():
    """``adamw_groups_expected`` (the scalars as the kernel gets them, float32) against ``adamw_groups_step`` (unrounded): what
    differs is a handful of scalars each off by at most 2**-24 relatively -- 1e-6 of the largest m, v and of the largest move of a
    weight, the margin tests/test_flat_ref_cpu.py gives plain Adam.  With one group {1, 0} it IS ``flat_ref.adam_clip_expected``,
    whose bound on p it exceeds by exactly one ulp of the larger operand."""
    n, lr = 1000, 3e-4
    p, g, m, v = FR.optimiser_case(n, 3)
    sumsq = np.float32(np.sum(g.astype(np.float64) ** 2))
    seg_end, seg_group, scales, decays = [4, 8, 256, 260, 1000], [0, 1, 2, 0, 1], [1.0, 0.1, 0.0], [0.0, 1e-3, 0.1]
    f32 = dict(beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))  # (as the kernel is fed them)
    for step in (1, 7):
        want, bound = AR.adamw_groups_expected(p, g, m, v, sumsq, step, seg_end, seg_group, scales, decays, lr=lr)
        q, mq, vq = (a.astype(np.float64) for a in (p, m, v))
        AR.adamw_groups_step(q, g.astype(np.float64), mq, vq, step, seg_end, seg_group, scales, decays, lr=lr, **f32)
        moved = np.abs(q - p).max()
        # (and decay_G, a number next to 1 rounded to float32, is off by up to 2**-24 absolutely: that times |p|)
        assert np.abs(want["p"] - q).max() <= 1e-6 * moved + 2.0 ** -24 * np.abs(p).max() and 1e-5 < moved
        assert np.abs(want["m"] - mq).max() <= 1e-6 * np.abs(mq).max() and np.abs(want["v"] - vq).max() <= 1e-6 * vq.max()
        for k, size in (("m", np.abs(m)), ("v", v), ("p", np.abs(p))):
            assert (bound[k] > 0).all() and (bound[k] <= 64 * OR.f32_ulp(np.maximum(size, np.abs(want[k])))).all(), (k, step)
        # scale 0: the weight only decays -- exactly p * decay_G -- while m and v still move
        z = AR.per_element(seg_end, seg_group, [0, 0, 1]).astype(bool)
        d2 = AR.group_scalars(lr, 0.0, 0.1, step)
        assert d2 == dict(lr=0.0, step_size=0.0, decay=1.0)
        assert np.array_equal(want["p"][z], p[z].astype(np.float64)) and not np.array_equal(want["m"][z], m[z])
        one, b_one = AR.adamw_groups_expected(p, g, m, v, sumsq, step, [n], [0], [1.0], [0.0], lr=lr)
        ref, b_ref = FR.adam_clip_expected(p, g, m, v, sumsq, step, lr=lr)
        assert all(np.array_equal(one[k], ref[k]) for k in "pmv") and all(np.array_equal(b_one[k], b_ref[k]) for k in "mv")
        t = np.abs(ref["p"] - p)
        assert np.allclose(b_one["p"] - b_ref["p"], OR.f32_ulp(np.maximum(np.abs(p), t)), rtol=1e-9, atol=0)
    s = AR.group_scalars(3e-4, 0.1, 1e-2, 7)
    lr_g = float(np.float32(float(np.float32(3e-4)) * float(np.float32(0.1))))
    assert s["lr"] == lr_g and s["decay"] == float(np.float32(1.0 - lr_g * float(np.float32(1e-2)))) < 1.0
    assert s["step_size"] == float(np.float32(lr_g / (1.0 - float(np.float32(0.9)) ** 7)))


# --------------------------------------------------------------------------------------------------- the segment tables
def models():
    import silent_speech_amd as ss

    return {"landmarks": (ss.BiGRUClassifier(84, 5), 0), "roi": (ss.BiGRUClassifier(84, 5, use_roi=True), 0),
            "roi_one_layer": (ss.BiGRUClassifier(84, 5, use_roi=True, gru_layers=1), 0),
            "roi_frozen": (ss.BiGRUClassifier(84, 5, use_roi=True), None)}


@pytest.mark.parametrize("name", ["landmarks", "roi", "roi_one_layer", "roi_frozen"])
def test_segment_table_of_real_models(name):
    import silent_speech_amd as ss
    from silent_speech_amd.train import SegmentTable

    model, lo = models()[name]
    lo = model.cnn_param_range() if lo is None else lo
    lay, total = model._layout()
    groups = [ss.ParamGroup("gru.weight_hh", lr_scale=0.5), ss.no_decay(), ss.ParamGroup(("gru.", "head."), lr_scale=0.25, weight_decay=0.3)]
    ends, ids, members = model.param_segments(groups, lo)
    table = SegmentTable(model, groups, 1e-2, lo)
    assert table.seg_end == ends and table.seg_group == ids and table.n == total - lo
    # ends: multiples of 4, strictly increasing, the last the range length; the segments tile [lo, n) and follow the layout
    assert all(e % 4 == 0 for e in ends) and all(a < b for a, b in zip([0] + ends, ends)) and ends[-1] == total - lo
    assert len(ends) <= 64 and all(0 <= g <= len(groups) for g in ids)
    live = [(n_, off - lo, cnt) for n_, off, cnt, _ in lay if off >= lo]
    assert len(live) == len(lay) - (8 if name == "roi_frozen" else 0) and (lo > 0) == (name == "roi_frozen")
    starts = [0] + ends[:-1]
    want_group = {}
    for n_, off, cnt in live:  # every tensor lies inside exactly one segment, which is its group's
        s = next(k for k, (a, b) in enumerate(zip(starts, ends)) if a <= off and off + cnt <= b)
        want_group[n_] = ids[s]
    first = lambda n_: next((i for i, g in enumerate(groups) if g.matches(n_)), len(groups))  # noqa: E731
    assert want_group == {n_: first(n_) for n_, _, _ in live}
    assert sorted(sum(members, [])) == sorted(want_group) and all(want_group[n_] == g for g, ms in enumerate(members) for n_ in ms)
    # adjacent tensors of one group are merged: neighbouring segments differ, and there are as many segments as group changes
    assert all(a != b for a, b in zip(ids, ids[1:]))
    order = [want_group[n_] for n_, _, _ in live]
    assert len(ends) == 1 + sum(a != b for a, b in zip(order, order[1:]))
    # first match wins: gru.weight_hh_* is in group 0 although group 2 matches it too, the GRU biases in no_decay()'s (1) although
    # "gru." matches them; no_decay() holds exactly the biases and the LayerNorm
    assert all(want_group[n_] == 0 for n_ in want_group if n_.startswith("gru.weight_hh"))
    assert members[1] == [n_ for n_, _, _ in live if "bias" in n_ or n_.startswith("head.0.")]
    assert any(n_.startswith("gru.bias_") for n_ in members[1]) and "head.0.weight" in members[1] and "pool.score.bias" in members[1]
    assert members[2] == [n_ for n_, _, _ in live if n_.startswith(("gru.weight_ih", "head.1.weight", "head.4.weight"))]
    assert members[3] == [n_ for n_, _, _ in live if n_ == "pool.score.weight" or (n_.startswith("roi_cnn.") and "bias" not in n_)]
    # scales and decays per group: None inherits the trainer's decay, the default group is last
    assert table.lr_scale == [0.5, 1.0, 0.25, 1.0] and table.weight_decay == [1e-2, 0.0, 0.3, 1e-2]
    plain = table.plain()
    assert plain["seg_end"] == ends and plain["seg_group"] == ids and plain["match"][-1] == [] and len(plain["match"]) == 4
    assert table.args[2] == len(ends) and table.args[5] == 4
    # no groups at all: one segment, the default group
    assert model.param_segments((), lo)[:2] == ([total - lo], [0])


def test_the_no_decay_table_of_the_shipped_model_has_fifteen_segments():
    import silent_speech_amd as ss

    model = ss.BiGRUClassifier(180, 10, use_roi=True)
    ends, ids, members = model.param_segments([ss.ParamGroup("roi_cnn.", lr_scale=0.1), ss.no_decay()])
    # the CNN (its biases too: the first match wins), then weights and biases in turn
    assert len(ends) == 15 and ids == [0] + [2, 1] * 7 and ends[0] == model.cnn_param_range() and ends[-1] == model._layout()[1]
    assert all(n.startswith("roi_cnn.") for n in members[0]) and len(members[0]) == 8


def test_group_limits_and_frozen_cnn_groups_raise():
    import silent_speech_amd as ss

    model = ss.BiGRUClassifier(84, 5, use_roi=True)
    seven = [ss.ParamGroup("gru.weight_ih_l%d" % k) for k in range(7)]
    assert len(model.param_segments(seven)[2]) == 8  # seven and the default one: the most one launch takes
    with pytest.raises(ValueError, match="at most 8 groups"):
        model.param_segments(seven + [ss.ParamGroup("head.")])
    with pytest.raises(ValueError, match="at most 8 groups"):
        ss.Trainer(model, param_groups=seven + [ss.ParamGroup("head.")])  # (before the device check)
    n_cnn = model.cnn_param_range()
    with pytest.raises(ValueError, match="frozen ROI CNN"):
        model.param_segments([ss.ParamGroup("roi_cnn.", lr_scale=0.1), ss.no_decay()], n_cnn)
    with pytest.raises(ValueError, match="frozen ROI CNN"):
        model.param_segments([ss.ParamGroup(("gru.", "roi_cnn.fc."))], n_cnn)
    with pytest.raises(ValueError, match="frozen ROI CNN"):
        ss.Trainer(model, freeze_cnn=True, param_groups=[ss.ParamGroup("roi_cnn.")])
    model.param_segments([ss.no_decay()], n_cnn)  # "*bias" matches CNN biases as well: a suffix names no module
    # more than 64 segments: a deep GRU whose weights and biases alternate
    deep = ss.BiGRUClassifier(84, 5, gru_layers=17)
    with pytest.raises(ValueError, match="at most 64"):
        deep.param_segments([ss.no_decay()])
    assert len(deep.param_segments(())[0]) == 1
    for bad in (dict(match=""), dict(match=()), dict(match="*"), dict(match="gru.", lr_scale=-1.0), dict(match="gru.", lr_scale=float("nan")),
                dict(match="gru.", weight_decay=-0.1), dict(match="gru.", weight_decay=float("inf"))):
        with pytest.raises(ValueError, match="ParamGroup"):
            ss.ParamGroup(**bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            ss.Trainer(model, weight_decay=bad)
    with pytest.raises(RuntimeError, match="HIP device"):  # good groups get as far as the device check
        ss.Trainer(model, weight_decay=1e-2, param_groups=[ss.no_decay()])


# ------------------------------------------------------------------------------------------------------------ the schedules
def test_lr_schedule_values():
    import silent_speech_amd as ss

    lin = ss.LrSchedule(warmup_steps=4, decay="linear", total_steps=24, final_frac=0.1)
    assert lin(1) == 0.25 and lin(4) == 1.0                      # step 1, the last warm-up step
    assert lin(5) == 1.0 - 0.9 * (1.0 / 20.0)                    # the first decay step
    assert lin(24) == 0.1 and lin(25) == 0.1 and lin(10 ** 6) == 0.1  # total_steps and beyond: held at final_frac
    assert lin(14) == 1.0 - 0.9 * 0.5
    cos = ss.LrSchedule(warmup_steps=4, decay="cosine", total_steps=24, final_frac=0.1)
    assert cos(1) == 0.25 and cos(4) == 1.0
    assert cos(5) == 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi / 20.0)) and 0.99 < cos(5) < 1.0
    assert abs(cos(14) - 0.55) < 1e-15 and cos(24) == 0.1 and cos(1000) == 0.1
    assert all(cos(k) > cos(k + 1) for k in range(4, 24)) and all(lin(k) > lin(k + 1) for k in range(4, 24))
    flat = ss.LrSchedule(warmup_steps=2)
    assert [flat(k) for k in (1, 2, 3, 1000)] == [0.5, 1.0, 1.0, 1.0]
    plain = ss.LrSchedule()
    assert [plain(k) for k in (1, 2, 10 ** 9)] == [1.0, 1.0, 1.0]
    nowarm = ss.LrSchedule(decay="linear", total_steps=10)
    assert nowarm(1) == 0.9 and nowarm(10) == 0.0 and nowarm(11) == 0.0
    with pytest.raises(ValueError, match="total_steps"):
        ss.LrSchedule(decay="cosine")(3)
    assert ss.LrSchedule(warmup_steps=5, decay="cosine")(3) == 0.6  # (the warm-up needs no total)
    for bad in (dict(decay="exp"), dict(warmup_steps=-1), dict(warmup_steps=4, total_steps=4), dict(final_frac=1.5),
                dict(final_frac=float("nan"))):
        with pytest.raises(ValueError, match="LrSchedule"):
            ss.LrSchedule(**bad)
    assert lin.plain() == dict(warmup_steps=4, decay="linear", total_steps=24, final_frac=0.1)


# 40 values: improvements, exact ties, improvements below the relative threshold of 1e-2 (0.5 -> 0.504), dips
METRICS = [0.30, 0.50, 0.50, 0.504, 0.50, 0.49, 0.51, 0.51, 0.5149, 0.52, 0.52, 0.52, 0.52, 0.60, 0.60, 0.605, 0.59, 0.58, 0.61, 0.61,
           0.61, 0.61, 0.61, 0.6159, 0.6161, 0.70, 0.70, 0.69, 0.70, 0.706, 0.71, 0.71, 0.71, 0.71, 0.71, 0.71, 0.80, 0.80, 0.80, 0.80]


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("patience", [0, 2])
def test_plateau_schedule_is_torchs_reduce_on_plateau(mode, patience):
    import silent_speech_amd as ss

    assert len(METRICS) == 40
    values = METRICS if mode == "max" else [1.0 - x for x in METRICS]
    tp = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([tp], lr=1.0)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode=mode, factor=0.5, patience=patience, threshold=1e-2, eps=0.0)
    mine = ss.PlateauSchedule(mode=mode, factor=0.5, patience=patience, threshold=1e-2)
    scales = []
    for k, x in enumerate(values):
        ref.step(x)
        moved = mine.step(x)
        assert mine.scale == opt.param_groups[0]["lr"], (k, x, mine.scale, opt.param_groups[0]["lr"])
        assert mine.best == ref.best and mine.bad == ref.num_bad_epochs, (k, mine.best, ref.best, mine.bad, ref.num_bad_epochs)
        assert moved == (mine.scale != (scales[-1] if scales else 1.0))
        scales.append(mine.scale)
    assert 1.0 > scales[-1] >= 2.0 ** -40 and scales[0] == 1.0  # it did reduce, by powers of two (exact in float64)
    # the state is three numbers and restores the sequence; reset() starts over
    half = ss.PlateauSchedule(mode=mode, factor=0.5, patience=patience, threshold=1e-2)
    for x in values[:17]:
        half.step(x)
    state = half.state_dict()
    assert set(state) == {"best", "bad", "scale"}
    other = ss.PlateauSchedule(mode=mode, factor=0.5, patience=patience, threshold=1e-2)
    other.load_state_dict(state)
    for x in values[17:]:
        other.step(x)
    assert other.state_dict() == mine.state_dict()
    mine.reset()
    assert mine.state_dict() == dict(best=-math.inf if mode == "max" else math.inf, bad=0, scale=1.0)


def test_plateau_defaults_and_floor():
    import silent_speech_amd as ss

    d = ss.PlateauSchedule()
    assert d.plain() == dict(mode="max", factor=0.5, patience=10, threshold=1e-4, min_scale=0.0)
    f = ss.PlateauSchedule(patience=0, min_scale=0.2)
    f.step(1.0)
    assert [f.step(0.5) for _ in range(4)] == [True, True, True, False] and f.scale == 0.2
    for bad in (dict(mode="up"), dict(factor=1.0), dict(factor=0.0), dict(patience=-1), dict(min_scale=2.0), dict(threshold=-1.0)):
        with pytest.raises(ValueError, match="PlateauSchedule"):
            ss.PlateauSchedule(**bad)


# ---------------------------------------------------------------------------------------------------------- the fingerprint
FIELDS = dict(seed=42, batch_size=16, world_size=1, max_t=90, lr=3e-4, labels=["a", "b"], x_dim=84, use_roi=True, n_train=10, n_val=2,
              class_weights=None, augment_policy=None, ema_decay=None)


def test_run_fingerprint_is_unchanged_without_the_new_arguments_and_names_them_when_they_differ(tmp_path):
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    assert Hn.run_fingerprint(**FIELDS) == FIELDS
    assert Hn.run_fingerprint(**FIELDS, weight_decay=0.0, param_groups=None, lr_schedule=None, lr_plateau=None) == FIELDS
    assert list(Hn.run_fingerprint(**FIELDS)) == list(Ck.FINGERPRINT_FIELDS)
    new = dict(weight_decay=1e-2, param_groups=[ss.ParamGroup("roi_cnn.", lr_scale=0.1), ss.no_decay()],
               lr_schedule=ss.LrSchedule(warmup_steps=2, decay="cosine"), lr_plateau=ss.PlateauSchedule(patience=0))
    full = Hn.run_fingerprint(**FIELDS, **new)
    assert full == dict(FIELDS, weight_decay=1e-2,
                        param_groups=[dict(match=["roi_cnn."], lr_scale=0.1, weight_decay=None),
                                      dict(match=["*bias", "gru.bias_", "head.0."], lr_scale=1.0, weight_decay=0.0)],
                        lr_schedule=dict(warmup_steps=2, decay="cosine", total_steps=None, final_frac=0.0),
                        lr_plateau=dict(mode="max", factor=0.5, patience=0, threshold=1e-4, min_scale=0.0))
    for name, value in new.items():  # each alone is one more entry, and the one the comparison names
        one = Hn.run_fingerprint(**FIELDS, **{name: value})
        assert set(one) == set(FIELDS) | {name}
        assert Ck.fingerprint_difference(FIELDS, one) == name and Ck.fingerprint_difference(one, one) is None
    other = dict(weight_decay=1e-3, param_groups=[ss.no_decay()], lr_schedule=ss.LrSchedule(warmup_steps=3, decay="cosine"),
                 lr_plateau=ss.PlateauSchedule(patience=1))
    for name, value in other.items():
        assert Ck.fingerprint_difference(full, Hn.run_fingerprint(**FIELDS, **dict(new, **{name: value}))) == name
    # through a file: lists for tuples, None stays None
    path = str(tmp_path / "s.pt")
    Ck.save_train_state(path, dict(format=Ck.TRAIN_STATE_FORMAT, fingerprint=full, plateau=ss.PlateauSchedule(mode="min").state_dict()))
    back = Ck.load_train_state(path)
    assert Ck.fingerprint_difference(back["fingerprint"], full) is None and back["plateau"] == dict(best=math.inf, bad=0, scale=1.0)


def test_fit_checks_the_new_arguments_before_anything_else(tmp_path, monkeypatch):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    def never(*a, **k):
        raise AssertionError("fit went past its argument checks")

    monkeypatch.setattr(Hn, "scan_clips", never)
    out = str(tmp_path / "o.pt")
    with pytest.raises(ValueError, match="weight_decay"):
        Hn.fit(str(tmp_path), out, weight_decay=-1.0)
    with pytest.raises(TypeError, match="LrSchedule"):
        Hn.fit(str(tmp_path), out, lr_schedule="cosine")
    with pytest.raises(TypeError, match="PlateauSchedule"):
        Hn.fit(str(tmp_path), out, lr_plateau=0.5)
    with pytest.raises(TypeError, match="ParamGroup"):
        Hn.fit(str(tmp_path), out, param_groups=["gru."])


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_library_and_ctypes_table_agree_on_the_grouped_entry_point():
    from silent_speech_amd import _lib

    lib = _lib.load()
    assert declared_arguments("ss_adam_clip_ema") == 16  # (the parser, on an entry point that was there before)
    assert declared_arguments("ss_adamw_clip_groups") == 22
    assert hasattr(lib, "ss_adamw_clip_groups") and len(_lib.SIGNATURES["ss_adamw_clip_groups"]) == 22
    assert lib.ss_adamw_clip_groups.argtypes == _lib.SIGNATURES["ss_adamw_clip_groups"]
    # ss_adam_clip_ema + the two segment arrays and their count + the two group arrays and their count, in front of the stream
    e, w = _lib.SIGNATURES["ss_adam_clip_ema"], _lib.SIGNATURES["ss_adamw_clip_groups"]
    assert w == e[:-1] + [_lib._vp, _lib._vp, _lib._i, _lib._vp, _lib._vp, _lib._i] + e[-1:]
    assert lib.ss_abi_version() == 3  # additive
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ss_hotpath.h")).read()
    assert "HOST arrays" in hdr


def test_grouped_entry_point_refuses_bad_arguments_before_any_launch():
    """Every SS_ERR_ARG case returns before a launch: the 'device' pointers below are host memory that nothing dereferences (and
    that stays as it is), the four host arrays are real."""
    from silent_speech_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15  # 16-byte aligned
    P, G, M, V, E, S = (base + 2048 * k for k in range(6))
    n = 256

    def status(p=P, g=G, m=M, v=V, ema=E, n_=n, ends=(4, 8, n), ids=(0, 1, 2), scales=(1.0, 0.1, 0.0), decays=(0.0, 1e-3, 0.1),
               n_seg=None, n_groups=None, step=1, ema_decay=0.9, null=None):
        arrs = dict(ends=(ctypes.c_long * max(len(ends), 1))(*ends), ids=(ctypes.c_int * max(len(ids), 1))(*ids),
                    scales=(ctypes.c_float * max(len(scales), 1))(*scales), decays=(ctypes.c_float * max(len(decays), 1))(*decays))
        ptr = {k: (None if k == null else ctypes.addressof(a)) for k, a in arrs.items()}
        return lib.ss_adamw_clip_groups(p, g, m, v, ema, n_, S, 1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8, step, ema_decay, ptr["ends"], ptr["ids"],
                                        len(ends) if n_seg is None else n_seg, ptr["scales"], ptr["decays"],
                                        len(scales) if n_groups is None else n_groups, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(p=P + 4), dict(g=G + 8), dict(m=M + 4), dict(v=V + 12), dict(ema=E + 4),           # an unaligned pointer
           dict(ema=P), dict(ema=P + 16), dict(ema=P - 16),                                         # ema overlapping p
           dict(ends=(8, 8, n)), dict(ends=(8, 4, n)), dict(ends=(0, 8, n)), dict(ends=(-4, 8, n)),  # seg_end not increasing
           dict(ends=(4, 6, n)), dict(ends=(3, 8, n)),                                              # an interior end off a quad
           dict(ends=(4, 8, n - 4)), dict(ends=(4, 8, n + 4)), dict(n_=n - 1),                      # a last end that is not n
           dict(ids=(0, 3, 2)), dict(ids=(0, -1, 2)), dict(ids=(0, 1, 2), n_groups=2),              # a group id out of range
           dict(scales=(1.0, -0.1, 0.0)), dict(scales=(nan, 0.1, 0.0)), dict(scales=(1.0, inf, 0.0)),
           dict(decays=(0.0, -1e-3, 0.1)), dict(decays=(0.0, 1e-3, nan)), dict(decays=(inf, 1e-3, 0.1)),
           dict(ends=tuple(range(4, 4 * 66, 4)), ids=(0,) * 65, n_=4 * 65),                         # n_seg > 64
           dict(scales=(1.0,) * 9, decays=(0.0,) * 9), dict(n_seg=0), dict(n_groups=0),             # n_groups > 8; none at all
           dict(p=None), dict(g=None), dict(n_=0), dict(step=0), dict(ema_decay=1.0), dict(ema_decay=nan), dict(ema_decay=-0.5),
           dict(null="ends"), dict(null="ids"), dict(null="scales"), dict(null="decays")]
    for case in bad:
        assert status(**case) == -1, case
    assert not any(buf)
