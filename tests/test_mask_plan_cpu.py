"""CPU: the masking augmentations of the device-planned path as tests/mask_plan_ref.py restates them (no GPU) -- the policy's
validation and fingerprint rule, masks off, runs inside [1, n), bands and rectangles inside the row and the frame, and the
distribution of every draw (20 000 draws, five binomial standard deviations of the stated probability)."""
import dataclasses

import numpy as np
import pytest

import batch_plan_ref as P
import mask_plan_ref as M

SEED = 0x1234567890ABCDEF
N_DRAWS = 20000


def _sigma(p, n):
    return np.sqrt(p * (1 - p) / n)


def _uniform(values, lo, hi, what):
    """Every integer of [lo, hi] equally likely among ``values``: each count within five binomial standard deviations."""
    values = np.asarray(values)
    k, n = hi - lo + 1, len(values)
    assert values.min() >= lo and values.max() <= hi, (what, values.min(), values.max())
    for v in range(lo, hi + 1):
        assert abs((values == v).mean() - 1 / k) < 5 * _sigma(1 / k, n), (what, v, (values == v).mean(), 1 / k)


def _maps(lens, max_t, roi=True, noisy=True):
    """Maps as a planner leaves them for clips of the given planned lengths: store rows 100 b + t, -1 behind the length."""
    lens = np.asarray(lens, np.int64)
    t = np.arange(max_t)[None, :]
    inside = t < lens[:, None]
    xmap = np.where(inside, 100 * np.arange(len(lens))[:, None] + t, -1).astype(np.int32)
    nmap = np.where(inside & noisy, 0, -1).astype(np.int32)
    rmap = np.where(inside, 5000 + xmap, -1).astype(np.int32) if roi else None
    return xmap, nmap, rmap, lens


# ------------------------------------------------------------------------------------------------ the policy
def test_policy_defaults_and_validation():
    import silent_speech_amd as ss

    p = ss.AugmentPolicy()
    assert (p.time_mask_prob, p.time_mask_max, p.time_mask_streams, p.time_mask_fill) == (0.0, 0, "both", "zero")
    assert (p.feat_mask_prob, p.feat_mask_max, p.cutout_prob, p.cutout_max, p.cutout_fill) == (0.0, 0, 0.0, (0, 0), 128)
    assert not (p.time_mask_on or p.feat_mask_on or p.cutout_on)
    # on = probability > 0 and maximum >= 1
    assert not ss.AugmentPolicy(time_mask_prob=1.0).time_mask_on and not ss.AugmentPolicy(time_mask_max=3).time_mask_on
    assert ss.AugmentPolicy(time_mask_prob=0.1, time_mask_max=1).time_mask_on
    assert ss.AugmentPolicy(feat_mask_prob=0.1, feat_mask_max=1).feat_mask_on and not ss.AugmentPolicy(feat_mask_prob=0.1).feat_mask_on
    assert ss.AugmentPolicy(cutout_prob=0.5, cutout_max=(1, 1)).cutout_on
    assert not ss.AugmentPolicy(cutout_prob=0.5, cutout_max=(4, 0)).cutout_on
    assert ss.AugmentPolicy(cutout_max=[3, 2]).cutout_max == (3, 2)
    bad = (dict(time_mask_prob=1.5), dict(time_mask_prob=-0.1), dict(feat_mask_prob=2), dict(cutout_prob=float("nan")),
           dict(time_mask_max=-1), dict(time_mask_max=2.5), dict(feat_mask_max=-3), dict(feat_mask_max="4"), dict(cutout_max=(1,)),
           dict(cutout_max=(-1, 2)), dict(cutout_max=(1.5, 2)), dict(cutout_fill=256), dict(cutout_fill=-1), dict(cutout_fill=1.5),
           dict(time_mask_streams="audio"), dict(time_mask_fill="mean"))
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            ss.AugmentPolicy(**kw)
    # lineage() is what it was
    lin = ss.AugmentPolicy.lineage()
    assert lin == ss.AugmentPolicy(time_warp_prob=0.5, time_warp_range=(0.8, 1.2), scale_prob=0.3, scale_range=(0.95, 1.05))
    assert not (lin.time_mask_on or lin.feat_mask_on or lin.cutout_on)
    assert ss.AugmentPolicy.lineage(time_mask_prob=0.5, time_mask_max=4).time_mask_on


def test_fingerprint_carries_the_mask_fields_only_off_their_defaults():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    base = dict(seed=42, batch_size=16, world_size=1, max_t=24, lr=3e-3, labels=["aura", "no"], x_dim=20, use_roi=True, n_train=38,
                n_val=7, class_weights=None, ema_decay=None)
    old_keys = {"time_warp_prob", "time_warp_range", "scale_prob", "scale_range", "roi_shift_prob", "roi_shift_max"}
    lin = ss.AugmentPolicy.lineage()
    fp = Hn.run_fingerprint(**base, augment_policy=lin)
    assert set(fp["augment_policy"]) == old_keys
    assert fp["augment_policy"] == dict(time_warp_prob=0.5, time_warp_range=[0.8, 1.2], scale_prob=0.3, scale_range=[0.95, 1.05],
                                        roi_shift_prob=0.0, roi_shift_max=[0, 0])
    # fields spelled out at their defaults change nothing either
    same = ss.AugmentPolicy.lineage(time_mask_streams="both", cutout_fill=128, cutout_max=(0, 0), time_mask_max=0)
    assert Ck.fingerprint_difference(fp, Hn.run_fingerprint(**base, augment_policy=same)) is None
    masked = ss.AugmentPolicy.lineage(time_mask_prob=0.5, time_mask_max=4, time_mask_fill="hold", cutout_prob=0.25, cutout_max=(8, 6))
    fm = Hn.run_fingerprint(**base, augment_policy=masked)
    assert set(fm["augment_policy"]) == old_keys | {"time_mask_prob", "time_mask_max", "time_mask_fill", "cutout_prob", "cutout_max"}
    assert fm["augment_policy"]["cutout_max"] == [8, 6] and fm["augment_policy"]["time_mask_fill"] == "hold"
    assert Ck.fingerprint_difference(fp, fm) == "augment_policy"
    for name in ss.device_data.MASK_FIELDS:  # every single field off its default is seen
        default = getattr(lin, name)
        other = {str: {"both": "roi", "zero": "hold"}.get(default), float: 0.5, int: 7, tuple: (3, 3)}[type(default)]
        one = Hn.run_fingerprint(**base, augment_policy=dataclasses.replace(lin, **{name: other}))
        assert set(one["augment_policy"]) == old_keys | {name} and Ck.fingerprint_difference(fp, one) == "augment_policy"


# ------------------------------------------------------------------------------------------------ the restatement
def test_masks_off_return_the_inputs_and_a_zero_table():
    xmap, nmap, rmap, lens = _maps([0, 3, 8, 24, 24, 17], 24)
    on = dict(time_mask_prob=1.0, time_mask_max=5, feat_mask_prob=1.0, feat_mask_max=9, cutout_prob=1.0, cutout_max=(8, 8))
    cases = [dict(), dict(on, augment=False), dict(on, time_mask_prob=0.0, feat_mask_prob=0.0, cutout_prob=0.0),
             dict(on, time_mask_max=0, feat_mask_max=0, cutout_max=(0, 8)), dict(on, time_mask_max=0, feat_mask_max=0, cutout_max=(8, 0))]
    for kw in cases:
        gx, gn, gr, gl, table = M.plan_mask(xmap, nmap, rmap, lens, 11, SEED, 84, 64, 64, **kw)
        assert np.array_equal(gx, xmap) and np.array_equal(gn, nmap) and np.array_equal(gr, rmap) and np.array_equal(gl, lens)
        assert table.shape == (6, 8) and table.dtype == np.int32 and not table.any()
    # ... and with everything on the inputs themselves are left alone (copies are edited)
    keep = xmap.copy()
    gx = M.plan_mask(xmap, nmap, rmap, lens, 11, SEED, 84, 64, 64, **on)[0]
    assert np.array_equal(xmap, keep) and not np.array_equal(gx, keep)


@pytest.mark.parametrize("fill", M.FILLS)
@pytest.mark.parametrize("streams", M.STREAMS)
def test_runs_stay_inside_the_clip_for_every_length(streams, fill):
    """n = 0 .. 40, 200 draws each, probability 1: the run lies in [1, n), lens is unchanged, n < 8 is never masked, the maps
    differ from the planner's inside the run of the selected streams only, and "hold" rows equal row t0 - 1."""
    reps, max_t = 200, 40
    lens = np.repeat(np.arange(41), reps)
    xmap, nmap, rmap, lens = _maps(lens, max_t)
    gx, gn, gr, gl, table = M.plan_mask(xmap, nmap, rmap, lens, 0, SEED, 84, 64, 64, time_mask_prob=1.0, time_mask_max=6,
                                        time_mask_streams=streams, time_mask_fill=fill)
    t0, tw = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64)
    assert np.array_equal(gl, lens) and not table[:, 2:].any()
    assert not tw[lens < 8].any() and not t0[lens < 8].any() and np.all(tw[lens >= 8] >= 1)
    act = tw > 0
    assert np.all(t0[act] >= 1) and np.all(t0[act] + tw[act] <= lens[act]) and np.all(tw[act] <= np.minimum(6, lens[act] // 4))
    t = np.arange(max_t)[None, :]
    run = act[:, None] & (t >= t0[:, None]) & (t < (t0 + tw)[:, None])
    feat, roi = streams != "roi", streams != "features"
    src = np.maximum(t0 - 1, 0)[:, None]
    if fill == "zero":
        want_x = np.where(run & feat, -1, xmap)
        want_n = np.where(run & feat, -1, nmap)
        want_r = np.where(run & roi, -1, rmap)
    else:
        want_x = np.where(run & feat, np.take_along_axis(xmap, src, 1), xmap)
        want_n = nmap
        want_r = np.where(run & roi, np.take_along_axis(rmap, src, 1), rmap)
        assert np.all(want_x[run] >= 0) and np.all(want_r[run] >= 0)
    assert np.array_equal(gx, want_x) and np.array_equal(gn, want_n) and np.array_equal(gr, want_r)
    assert np.array_equal(gx[:, 0], xmap[:, 0]) and np.array_equal(gr[:, 0], rmap[:, 0])  # frame 0 is never masked
    # both ends of the clip are reached: a run that starts at 1, one that ends at n
    big = lens == 40
    assert (t0[big] == 1).any() and (t0[big] + tw[big] == 40).any()
    # a store without ROI frames: "roi" edits nothing
    gx2, gn2, gr2, _, table2 = M.plan_mask(xmap, nmap, None, lens, 0, SEED, 84, time_mask_prob=1.0, time_mask_max=6,
                                           time_mask_streams=streams, time_mask_fill=fill)
    assert gr2 is None and np.array_equal(table2, table) and np.array_equal(gx2, want_x) and np.array_equal(gn2, want_n)


@pytest.mark.parametrize("D,H,W", [(84, 64, 64), (83, 12, 20), (1, 1, 1)])
def test_bands_and_rectangles_stay_inside_for_maxima_below_at_and_above(D, H, W):
    n = np.full(4000, 24)
    top = 2 ** 31 - 1
    for fm, cm in ((max(1, D // 3), (max(1, W // 3), max(1, H // 3))), (D, (W, H)), (D + 50, (W + 9, H + 100)), (top, (top, top))):
        table = M.decisions(n, True, 5, SEED, D, H, W, feat_mask_prob=1.0, feat_mask_max=fm, cutout_prob=1.0, cutout_max=cm).astype(np.int64)
        _, _, col0, cw, x0, y0, rw, rh = table.T
        assert np.all(cw >= 1) and np.all(cw <= min(fm, D)) and np.all(col0 >= 0) and np.all(col0 + cw <= D)
        assert np.all(rw >= 1) and np.all(rw <= min(cm[0], W)) and np.all(x0 >= 0) and np.all(x0 + rw <= W)
        assert np.all(rh >= 1) and np.all(rh <= min(cm[1], H)) and np.all(y0 >= 0) and np.all(y0 + rh <= H)
        if fm >= D:
            assert (cw == D).any() and np.all(col0[cw == D] == 0)
        if cm[0] >= W and cm[1] >= H and W * H <= 240:  # (one draw in W * H is the full frame: 4000 draws reach it there)
            full = (rw == W) & (rh == H)
            assert full.any() and not x0[full].any() and not y0[full].any()


def test_apply_restates_band_and_rectangle():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(3, 5, 9)).astype(np.float32)
    R = rng.integers(1, 256, (3, 5, 6, 8), dtype=np.uint8)
    rmap = np.array([[0, 1, 2, -1, -1], [-1] * 5, [3, 4, 5, 6, 7]], np.int32)
    R[rmap < 0] = 0
    table = np.array([[0, 0, 2, 3, 1, 2, 4, 3], [2, 1, 0, 9, 0, 0, 0, 0], [0, 0, 0, 0, 7, 5, 1, 1]], np.int32)
    gX, gR = M.apply(X, R, rmap, table, 200)
    assert not gX[0, :, 2:5].any() and np.array_equal(gX[0, :, :2], X[0, :, :2]) and np.array_equal(gX[0, :, 5:], X[0, :, 5:])
    assert not gX[1].any() and np.array_equal(gX[2], X[2])
    assert np.all(gR[0, :3, 2:5, 1:5] == 200) and not gR[0, 3:].any() and not gR[1].any()
    assert np.all(gR[2, :, 5, 7] == 200)
    changed = gR != R
    assert changed[0, :3, 2:5, 1:5].sum() + changed[2, :, 5, 7].sum() == changed.sum()
    assert M.apply(None, R, rmap, table, 1)[0] is None and M.apply(X, None, None, table, 1)[1] is None


# ------------------------------------------------------------------------------------------------ distributions
def test_mask_draws_have_the_stated_distributions():
    """20 000 draws of a clip of n = 40 planned frames with ROI frames, D = 84, 64 x 64 pixels."""
    n, N = 40, N_DRAWS
    kw = dict(time_mask_prob=0.4, time_mask_max=6, feat_mask_prob=0.3, feat_mask_max=10, cutout_prob=0.6, cutout_max=(16, 12))
    tab = M.decisions(np.full(N, n), True, 0, SEED, 84, 64, 64, **kw).astype(np.int64)
    t0, tw, col0, cw, x0, y0, rw, rh = tab.T
    timed, band, cut = tw > 0, cw > 0, rw > 0
    assert np.array_equal(cut, rh > 0)
    for name, got, p in (("time", timed, 0.4), ("band", band, 0.3), ("cutout", cut, 0.6)):
        assert abs(got.mean() - p) < 5 * _sigma(p, N), (name, got.mean())
    # independent of each other, and of the planner's own sub-draw 0 (noise with probability 0.7)
    assert abs((timed & band).mean() - 0.12) < 5 * _sigma(0.12, N)
    assert abs((timed & cut).mean() - 0.24) < 5 * _sigma(0.24, N)
    assert abs((band & cut).mean() - 0.18) < 5 * _sigma(0.18, N)
    noisy = P.decisions(np.full(N, n), 0, SEED)[0]
    assert abs((timed & noisy).mean() - 0.28) < 5 * _sigma(0.28, N)
    # widths uniform over 1 .. cap; cap = min(6, 40 // 4) = 6, and min(12, 40 // 4) = 10 when the maximum is above n / 4
    _uniform(tw[timed], 1, 6, "tw")
    wide = M.decisions(np.full(N, n), True, 0, SEED, 84, time_mask_prob=1.0, time_mask_max=12).astype(np.int64)
    _uniform(wide[:, 1], 1, 10, "tw capped at n / 4")
    # the start uniform over 1 .. n - tw, for one width at a time
    one = M.decisions(np.full(N, n), True, 0, SEED, 84, time_mask_prob=1.0, time_mask_max=1).astype(np.int64)
    assert np.all(one[:, 1] == 1)
    _uniform(one[:, 0], 1, n - 1, "t0 (tw = 1)")
    w6 = wide[wide[:, 1] == 6]
    assert len(w6) > 1500
    _uniform(w6[:, 0], 1, n - 6, "t0 (tw = 6)")
    # band
    _uniform(cw[band], 1, 10, "cw")
    b1 = M.decisions(np.full(N, n), True, 0, SEED, 84, feat_mask_prob=1.0, feat_mask_max=1).astype(np.int64)
    _uniform(b1[:, 2], 0, 83, "col0 (cw = 1)")
    # rectangle: sizes uniform, the position uniform at both extremes -- a 1 x 1 rectangle anywhere, the largest one
    _uniform(rw[cut], 1, 16, "rw")
    _uniform(rh[cut], 1, 12, "rh")
    small = M.decisions(np.full(N, n), True, 0, SEED, 84, 12, 20, cutout_prob=1.0, cutout_max=(1, 1)).astype(np.int64)
    assert np.all(small[:, 6:] == 1)
    _uniform(small[:, 4], 0, 19, "x0 (1 x 1)")
    _uniform(small[:, 5], 0, 11, "y0 (1 x 1)")
    big = M.decisions(np.full(8 * N, n), True, 0, SEED, 84, 12, 20, cutout_prob=1.0, cutout_max=(16, 8)).astype(np.int64)
    big = big[(big[:, 6] == 16) & (big[:, 7] == 8)]
    assert len(big) > 1000
    _uniform(big[:, 4], 0, 4, "x0 (16 x 8 of 20 x 12)")
    _uniform(big[:, 5], 0, 4, "y0 (16 x 8 of 20 x 12)")
    # a clip without ROI frames is never cut, no augmentation draws nothing, an empty row is eight zeros
    assert not M.decisions(np.full(500, n), False, 0, SEED, 84, 64, 64, cutout_prob=1.0, cutout_max=(8, 8))[:, 4:].any()
    assert not M.decisions(np.full(500, n), True, 0, SEED, 84, 64, 64, augment=False, **dict(kw, time_mask_prob=1.0)).any()
    assert not M.decisions(np.zeros(500, np.int64), True, 0, SEED, 84, 64, 64, **dict(kw, feat_mask_prob=1.0)).any()


def test_decisions_are_keyed_by_the_draw_index():
    """Rows [lo, hi) of a batch drawn from first_row + lo equal those rows of the whole batch: shards stay bit-equal."""
    kw = dict(time_mask_prob=0.5, time_mask_max=5, feat_mask_prob=0.5, feat_mask_max=12, cutout_prob=0.5, cutout_max=(9, 7))
    n = np.arange(70) % 41
    for base in (0, 2 ** 32 - 8, 2 ** 63 + 3):
        whole = M.decisions(n, n % 3 > 0, base, SEED, 83, 12, 20, **kw)
        for lo, hi in ((0, 6), (6, 33), (33, 70)):
            assert np.array_equal(M.decisions(n[lo:hi], n[lo:hi] % 3 > 0, base + lo, SEED, 83, 12, 20, **kw), whole[lo:hi])
    assert not np.array_equal(M.decisions(n, True, 0, SEED, 83, 12, 20, **kw), M.decisions(n, True, 0, SEED + 1, 83, 12, 20, **kw))
