"""CPU: the augmentation policy of the device-planned path as restated in tests/aug_plan_ref.py -- the policy switched off is
tests/batch_plan_ref.py's plan, the integer warp against np.linspace, the closed form of the ROI length against counting, map
entries inside their clips, the distributions of every new draw, and the Python surface (AugmentPolicy, batch, fit).

The GPU suite (tests/test_gpu_aug_plan.py) compares the kernels with this restatement exactly."""
import os
import re

import numpy as np
import pytest

import aug_plan_ref as A
import batch_plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567890ABCDEF
N_DRAWS = 20000
ALL_ON = dict(warp_prob=1.0, scale_prob=1.0, shift_prob=1.0, shift_max=(4, 2))


def _sigma(p, n):
    return np.sqrt(p * (1 - p) / n)


def _store(rng, n=40):
    clips = []
    for k in range(n):
        T = int(rng.integers(1, 121))
        Tr = None if k % 5 == 3 else max(0, T + int(rng.integers(-3, 4)))
        clips.append((T, Tr))
    return clips


def test_policy_off_is_the_plain_plan():
    """All three probabilities 0 (and the policy's sub-draws therefore unused): maps, lengths, labels == batch_plan_ref.plan."""
    rng = np.random.default_rng(3)
    clips = _store(rng)
    x_off, x_len, r_off, r_len = P.store_tables(clips)
    y = rng.integers(0, 7, len(clips))
    for tables in ((x_off, x_len, r_off, r_len), (x_off, x_len, None, None)):
        for max_t in (16, 90):
            for augment in (True, False):
                for first_row in (0, 2 ** 32 - 100, 2 ** 63 + 11):
                    idx = rng.integers(-1, len(clips) + 1, 300)
                    ref = P.plan(idx, *tables, y, max_t, augment, first_row, SEED)
                    got = A.plan(idx, *tables, y, max_t, augment, first_row, SEED, shift_max=(4, 2))
                    for key in ("xmap", "nmap", "rmap", "lens", "y_out", "noisy", "k"):
                        assert (got[key] is None and ref[key] is None) or np.array_equal(got[key], ref[key]), key
                    assert got["bad"] == ref["bad"]
                    assert np.all(got["row_scale"] == 1) and not got["row_shift"].any()
    # augment off switches the policy off as well
    got = A.plan(np.arange(len(clips)), x_off, x_len, r_off, r_len, y, 90, False, 0, SEED, **ALL_ON)
    ref = P.plan(np.arange(len(clips)), x_off, x_len, r_off, r_len, y, 90, False, 0, SEED)
    assert np.array_equal(got["xmap"], ref["xmap"]) and np.array_equal(got["rmap"], ref["rmap"])
    assert np.all(got["row_scale"] == 1) and not got["row_shift"].any()


def test_integer_warp_against_linspace():
    """Wp(j) = j (T-1) // (L-1) is np.linspace(0, T-1, L).astype(int) without linspace's float rounding: over T = 11..200 and
    every permille factor in 800..1200 the two never differ by more than one frame, and differ at all on at most 2 % of the
    (T, factor) pairs (measured: 1 181 of 76 190)."""
    pairs = differing = 0
    worst = 0
    for T in range(11, 201):
        for f in range(800, 1201):
            L = int(A.warp_len(T, f))
            assert L == max(5, T * f // 1000)
            mine = A.warp_src(np.arange(L), T, L)
            lin = np.linspace(0, T - 1, L).astype(int)
            d = int(np.abs(mine - lin).max())
            worst = max(worst, d)
            differing += d > 0
            pairs += 1
            assert mine[0] == 0 and mine[-1] == T - 1 and np.all(np.diff(mine) >= 0)
    print(f"linspace differs on {differing} of {pairs} (T, factor) pairs, by at most {worst} frame(s)")
    assert pairs == 190 * 401 and worst <= 1
    assert differing <= 0.02 * pairs
    # no warp: the identity, also for a clip of one frame
    for T in (1, 2, 10, 50):
        assert np.array_equal(A.warp_src(np.arange(T), T, T), np.arange(T))


def test_roi_length_closed_form_against_counting():
    for T in list(range(11, 60)) + [108, 200]:
        for f in (800, 873, 999, 1000, 1001, 1200, 2500, 4000, 100):
            L = int(A.warp_len(T, f))
            src = A.warp_src(np.arange(L), T, L)
            for Tr in (0, 1, 2, T - 3, T - 1, T, T + 3):
                assert int(A.roi_positions(T, Tr, L)) == int((src < Tr).sum()), (T, f, Tr)
    # unwarped: min(T, Tr), the reference's rule (also for T = 1)
    for T in range(1, 30):
        for Tr in range(0, T + 3):
            assert int(A.roi_positions(T, Tr, T)) == min(T, Tr)


@pytest.mark.parametrize("max_t", [16, 90])
def test_maps_stay_inside_their_clips(max_t):
    """Every policy on, 2000 rows per clip shape: map entries inside the clip, lengths <= max_t and consistent with the padding,
    feature frames non-decreasing with first and last kept, ROI frames only where the track has them."""
    n_rows = 2000
    warped = dropped = 0
    for T in (3, 10, 11, 12, 13, 14, 40, 64, 65, 90, 108):
        for Tr in (None, 0, T - 3, T, T + 3):
            if Tr is not None and Tr < 0:
                continue
            x_off, x_len, r_off, r_len = P.store_tables([(5, 5), (T, Tr), (7, None)])
            pl = A.plan(np.ones(n_rows, np.int64), x_off, x_len, r_off, r_len, [3, 1, 4], max_t, True, 2 ** 32 - 1000, SEED,
                        warp_prob=0.5, warp_lo_pm=800, warp_hi_pm=1200, scale_prob=0.3, scale_lo=0.95, scale_span=0.1,
                        shift_prob=0.5, shift_max=(4, 2))
            lens, L, k = pl["lens"], pl["L"], pl["k"]
            assert lens.max() <= max_t and lens.min() >= 0 and not pl["bad"]
            inside = np.arange(max_t)[None, :] < lens[:, None]
            for m in (pl["xmap"], pl["nmap"], pl["rmap"]):
                assert np.all(m[~inside] == -1)
            src = pl["xmap"] - x_off[1]
            assert np.all(src[inside] >= 0) and np.all(src[inside] < T)
            assert np.all((np.diff(src, axis=1) >= 0)[inside[:, 1:]])
            assert np.all(src[lens > 0, 0] == 0)
            whole = (lens == L - k) & (lens > 0)        # neither trimmed nor cut by the ROI track: the last frame is kept
            assert np.all(src[whole, lens[whole] - 1] == T - 1)
            if T <= 10:
                assert np.all(L == T) and not pl["warped"].any()
            else:
                assert np.all(L[pl["warped"]] >= max(5, T * 800 // 1000)) and np.all(L <= T * 1200 // 1000)
            assert not k[L <= 12].any()
            if Tr is None:
                assert np.all(pl["rmap"] == -1) and not pl["row_shift"].any()
            else:
                rs = pl["rmap"] - r_off[1]
                assert np.all(rs[inside] >= 0) and np.all(rs[inside] < Tr)
                want = np.minimum(np.minimum(L - k, max_t), A.roi_positions(T, Tr, L))
                assert np.array_equal(lens, want)
                assert np.abs(pl["row_shift"][:, 0]).max() <= 4 and np.abs(pl["row_shift"][:, 1]).max() <= 2
            assert pl["row_scale"].dtype == np.float32 and pl["row_scale"].min() >= np.float32(0.95)
            assert pl["row_scale"].max() <= np.float32(np.float32(0.95) + np.float32(0.1))
            warped += int(pl["warped"].sum())
            dropped += int(k.sum())
    assert warped > 0 and dropped > 0


def test_new_draws_have_the_stated_distributions():
    """20 000 draws of a T = 40 clip with ROI frames; bounds: five binomial standard deviations of the stated probability."""
    T, n = 40, N_DRAWS
    d = A.decisions(np.full(n, T), True, 0, SEED, warp_prob=0.5, scale_prob=0.3, shift_prob=0.5, shift_max=(4, 2))
    for name, p in (("warped", 0.5), ("scaled", 0.3), ("shifted", 0.5)):
        assert abs(d[name].mean() - p) < 5 * _sigma(p, n), (name, d[name].mean())
    # the three are independent of each other and of the reference's two
    assert abs((d["warped"] & d["scaled"]).mean() - 0.15) < 5 * _sigma(0.15, n)
    assert abs((d["warped"] & d["shifted"]).mean() - 0.25) < 5 * _sigma(0.25, n)
    assert abs((d["warped"] & d["noisy"]).mean() - 0.35) < 5 * _sigma(0.35, n)
    # every permille factor equally likely -> P(L) = (number of factors that give L) / 401
    nw = int(d["warped"].sum())
    Ls = d["L"][d["warped"]]
    factors = np.arange(800, 1201)
    L_of_f = np.maximum(5, T * factors // 1000)
    assert Ls.min() == 32 and Ls.max() == 48 and np.all(d["L"][~d["warped"]] == T)
    for L in range(32, 49):
        p = (L_of_f == L).sum() / 401.0
        assert p > 0 and abs((Ls == L).sum() - nw * p) < 5 * np.sqrt(nw * p * (1 - p)), L
    # every (dx, dy) of the box equally likely
    ns = int(d["shifted"].sum())
    sh = d["shift"][d["shifted"]]
    assert not d["shift"][~d["shifted"]].any()
    p = 1.0 / 45
    for dx in range(-4, 5):
        for dy in range(-2, 3):
            c = int(((sh[:, 0] == dx) & (sh[:, 1] == dy)).sum())
            assert abs(c - ns * p) < 5 * np.sqrt(ns * p * (1 - p)), (dx, dy, c)
    assert np.abs(sh[:, 0]).max() == 4 and np.abs(sh[:, 1]).max() == 2
    # the scale factor: uniform in [lo, lo + span), exactly 1 where not drawn
    sc = d["scale"][d["scaled"]]
    assert np.all(d["scale"][~d["scaled"]] == 1) and sc.min() >= np.float32(0.95) and sc.max() <= np.float32(1.05) + np.float32(1e-7)
    assert abs(sc.mean() - 1.0) < 5 * (0.1 / np.sqrt(12)) / np.sqrt(len(sc))
    assert abs((sc < 1.0).mean() - 0.5) < 5 * _sigma(0.5, len(sc))
    # a clip without ROI frames is never shifted, a clip of 10 frames never warped, no augmentation draws nothing
    assert not A.decisions(np.full(500, T), False, 0, SEED, shift_prob=1.0, shift_max=(4, 2))["shift"].any()
    assert not A.decisions(np.full(500, 10), True, 0, SEED, warp_prob=1.0)["warped"].any()
    off = A.decisions(np.full(500, T), True, 0, SEED, augment=False, **ALL_ON)
    assert not off["warped"].any() and not off["shift"].any() and np.all(off["scale"] == 1)
    # sub-draws 0 and 1 keep their meaning: an unwarped row decides noise and drop as batch_plan_ref does
    noisy, k, d0, d1 = P.decisions(np.full(n, T), 0, SEED)
    u = ~d["warped"]
    assert np.array_equal(d["noisy"], noisy) and all(np.array_equal(d[key][u], v[u]) for key, v in (("k", k), ("d0", d0), ("d1", d1)))


def test_shifted_and_scaled_gathers_restated():
    """The two gather restatements on a hand-made store: shift (0, 0) and scale 1 are the plain gather; a shift moves the image
    and replicates the edge."""
    rng = np.random.default_rng(1)
    Rs = rng.integers(0, 256, (6, 5, 8), dtype=np.uint8)
    fmap = np.array([[0, 1, -1], [5, -1, -1]], np.int32)
    assert np.array_equal(A.gather_shifted(Rs, fmap, np.zeros((2, 2), np.int32)), P.gather(Rs, fmap, (5, 8)))
    out = A.gather_shifted(Rs, fmap, np.array([[2, -1], [-9, 9]], np.int32))
    assert np.array_equal(out[0, 0, :4, 2:], Rs[0, 1:, :6]) and np.array_equal(out[0, 0, :, 0], out[0, 0, :, 2])
    assert np.array_equal(out[0, 0, 4], out[0, 0, 3]) and not out[0, 2].any() and not out[1, 1:].any()
    assert np.all(out[1, 0] == Rs[5, 0, 7])                                     # past both extremes: one corner pixel
    Xs = rng.normal(size=(6, 3)).astype(np.float32)
    assert np.array_equal(A.gather_scaled(Xs, fmap, np.ones(2, np.float32)), P.gather(Xs, fmap, (3,)))
    s = np.array([0.97, 1.03], np.float32)
    got = A.gather_scaled(Xs, fmap, s)
    assert got.dtype == np.float32 and np.array_equal(got[1, 0], Xs[5] * s[1]) and not got[1, 1:].any()


def test_augment_policy_validates():
    import silent_speech_amd as ss
    from silent_speech_amd.device_data import AugmentPolicy

    assert ss.AugmentPolicy is AugmentPolicy and "AugmentPolicy" in ss.__all__
    p = AugmentPolicy()
    assert (p.time_warp_prob, p.time_warp_range, p.scale_prob, p.scale_range, p.roi_shift_prob, p.roi_shift_max) == \
        (0.0, (0.8, 1.2), 0.0, (0.95, 1.05), 0.0, (0, 0))
    lin = AugmentPolicy.lineage()
    assert (lin.time_warp_prob, lin.time_warp_range, lin.scale_prob, lin.scale_range, lin.roi_shift_prob, lin.roi_shift_max) == \
        (0.5, (0.8, 1.2), 0.3, (0.95, 1.05), 0.0, (0, 0))
    both = AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(4, 2))
    assert both.roi_shift_max == (4, 2) and both.time_warp_prob == 0.5
    assert lin.warp_permille() == (800, 1200)
    lo, span = lin.scale_lo_span()
    assert lo == float(np.float32(0.95)) and span == float(np.float32(1.05 - 0.95))
    assert A.policy_kwargs(both)["shift_max"] == (4, 2) and A.policy_kwargs(both)["warp_hi_pm"] == 1200
    with pytest.raises(Exception):  # frozen
        p.scale_prob = 0.5
    for bad in (dict(time_warp_prob=-0.1), dict(time_warp_prob=1.01), dict(scale_prob=2), dict(roi_shift_prob=float("nan")),
                dict(time_warp_range=(0.0, 1.2)), dict(time_warp_range=(1.2, 0.8)), dict(time_warp_range=(0.8, 4.5)),
                dict(time_warp_range=(0.8,)), dict(scale_range=(0.0, 1.0)), dict(scale_range=(1.05, 0.95)),
                dict(scale_range=(-1.0, 1.0)), dict(roi_shift_max=(-1, 0)), dict(roi_shift_max=(1.5, 0)), dict(roi_shift_max=3)):
        with pytest.raises(ValueError):
            AugmentPolicy(**bad)


def test_the_library_declares_and_exports_the_three_entry_points():
    """Header, ctypes table and built library carry the new symbols; their argument checks are host code and answer without a
    GPU (nothing is launched)."""
    from silent_speech_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ss_hotpath.h")).read(), flags=re.S)
    for name, n_args in (("ss_batch_plan_aug", 33), ("ss_batch_gather_f32_aug", 12), ("ss_batch_gather_u8_shift", 11)):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert len(_lib.SIGNATURES[name]) == n_args
        assert hasattr(_lib.load(), name)
    lib, one = _lib.load(), 1 << 20  # any non-NULL address: refused before it is used

    def plan_status(noise=0.7, drop=0.35, drop_max=2, warp=0.5, lo_pm=800, hi_pm=1200, scale=0.3, s_lo=0.95, s_span=0.1, shift=0.5,
                    mx=4, my=2, row_scale=one):
        return lib.ss_batch_plan_aug(one, 4, one, one, None, None, one, 6, 24, 1, 0, 0, noise, drop, drop_max, warp, lo_pm, hi_pm,
                                     scale, s_lo, s_span, shift, mx, my, one, one, None, one, one, row_scale, one, one, None)

    for kw in (dict(warp=1.5), dict(warp=-0.1), dict(scale=1.01), dict(shift=-1e-9), dict(noise=2.0), dict(lo_pm=0),
               dict(lo_pm=1201), dict(hi_pm=4001), dict(s_lo=0.0), dict(s_span=-0.1), dict(mx=-1), dict(my=-1), dict(row_scale=None)):
        assert plan_status(**kw) == -1, kw
    assert plan_status(drop_max=3) == -3
    assert lib.ss_batch_gather_u8_shift(one, 32, 32, one, 16, one, 16, 32, 0, one, None) == -1      # mx >= W
    assert lib.ss_batch_gather_u8_shift(one, 32, 32, one, 16, one, 16, 0, 32, one, None) == -1      # my >= H
    assert lib.ss_batch_gather_u8_shift(one, 32, 32, one, 16, one, 16, -1, 0, one, None) == -1
    assert lib.ss_batch_gather_u8_shift(one, 32, 32, one, 16, None, 16, 4, 2, one, None) == -1
    assert lib.ss_batch_gather_u8_shift(one, 32, 32, one, 15, one, 16, 4, 2, one, None) == -1       # rows not whole clips
    assert lib.ss_batch_gather_u8_shift(one, 5, 7, one, 16, one, 16, 4, 2, one, None) == -3         # H * W % 16
    assert lib.ss_batch_gather_f32_aug(one, 20, one, 16, one, 0.01, 0, 0, None, 16, one, None) == -1
    assert lib.ss_batch_gather_f32_aug(one, 20, one, 16, one, 0.01, 0, 0, one, 0, one, None) == -1


def test_fit_and_batch_refuse_the_policy_outside_the_device_plan(tmp_path):
    """Both raise before anything is read or launched."""
    import silent_speech_amd as ss
    from silent_speech_amd import data as Dm
    from silent_speech_amd import harness as Hn

    pol = ss.AugmentPolicy.lineage()
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(tmp_path / "nothing_here"), str(tmp_path / "out.pt"), epochs=1, plan="host", augment_policy=pol)
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(tmp_path / "nothing_here"), str(tmp_path / "out.pt"), epochs=1, augment_policy=pol)
    with pytest.raises(TypeError):
        Hn.fit(str(tmp_path / "nothing_here"), str(tmp_path / "out.pt"), epochs=1, plan="device", augment_policy=dict(scale_prob=1.0))
    rng = np.random.default_rng(0)
    files = []
    for k in range(3):
        f = str(tmp_path / f"{k}.npz")
        Dm.save_clip(f, rng.normal(size=(14, 6)).astype(np.float32), np.arange(14), "yes", "me", np.arange(4),
                     rng.integers(0, 256, (14, 4, 4), dtype=np.uint8))
        files.append(f)
    store = ss.DeviceClipStore(files, {"yes": 0}, max_t=16, device="cpu")
    for kw in (dict(rng="device", augment=True), dict(rng="reference", augment=True), dict(rng="philox", augment=False), dict(augment=True)):
        with pytest.raises(ValueError, match="philox"):
            store.batch([0, 1], policy=pol, **kw)
    with pytest.raises(TypeError):
        store.batch([0, 1], rng="philox", augment=True, policy="lineage")
