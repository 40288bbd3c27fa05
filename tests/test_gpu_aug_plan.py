"""GPU: the augmentation policy of the device-planned path (ss_batch_plan_aug, ss_batch_gather_f32_aug,
ss_batch_gather_u8_shift, ``DeviceClipStore.batch(policy=)``, ``harness.fit(augment_policy=)``) against tests/aug_plan_ref.py --
integer maps, float32 bit patterns and bytes, all compared exactly.

Run on the MI355X box with ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest
import torch

import aug_plan_ref as A
import batch_plan_ref as P
from gpu_support import L, bits, sync  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
SEEDS = (SEED, 7, 2 ** 63 + 12345)
D = 10  # not a multiple of 4: a 16-byte chunk of X straddles two frames (and, at a clip's end, two clips)
# (T, Tr): one ROI track three frames short, one empty, one clip without ROI frames
CLIPS = [(3, 3), (10, 10), (11, 11), (12, 12), (13, 13), (14, 14), (40, 37), (64, 64), (65, 0), (90, None), (108, 108), (30, 33)]
POLICIES = {
    "warp": dict(warp_prob=1.0),
    "scale": dict(scale_prob=1.0),
    "shift": dict(shift_prob=1.0, shift_max=(4, 2)),
    "all": dict(warp_prob=1.0, warp_lo_pm=800, warp_hi_pm=1200, scale_prob=1.0, scale_lo=0.95, scale_span=0.1, shift_prob=1.0,
                shift_max=(4, 2)),
}


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda")


class Clips:
    """The synthetic store: files on disk (for DeviceClipStore), the concatenated arrays and the tables (for the restatement)."""

    def __init__(self, tmp, hw):
        rng = np.random.default_rng(hw[0] * 1000 + hw[1])
        self.hw, self.files, xs, rs = hw, [], [], []
        for n, (T, Tr) in enumerate(CLIPS):
            X = rng.normal(size=(T, D)).astype(np.float32)
            roi = None if Tr is None else rng.integers(0, 256, (Tr,) + hw, dtype=np.uint8)
            f = str(tmp / f"{n:02d}.npz")
            # (written directly: data.save_clip aligns X and roi to one length, these clips are ragged on purpose)
            arrays = dict(X=X, ts=np.arange(T), label="w%d" % (n % 3), speaker="me", idxs=np.arange(4))
            if roi is not None:
                arrays["roi"] = roi
            np.savez(f, **arrays)
            self.files.append(f)
            xs.append(X)
            if roi is not None:
                rs.append(roi)
        self.Xs, self.Rs = np.concatenate(xs, 0), np.concatenate(rs, 0)
        self.tables = P.store_tables(CLIPS)
        self.y = np.array([n % 3 for n in range(len(CLIPS))], np.int64)

    def store(self, max_t):
        import silent_speech_amd as ss

        return ss.DeviceClipStore(self.files, {"w0": 0, "w1": 1, "w2": 2}, max_t=max_t)


@pytest.fixture(scope="module")
def clips(tmp_path_factory, L):
    return {hw: Clips(tmp_path_factory.mktemp("clips%dx%d" % hw), hw) for hw in ((32, 32), (48, 96), (20, 12))}


def run_plan_aug(L, indices, x_off, x_len, r_off, r_len, y, max_t, augment, first_row, seed, noise_prob=0.7, drop_prob=0.35,
                 drop_max=2, warp_prob=0.0, warp_lo_pm=800, warp_hi_pm=1200, scale_prob=0.0, scale_lo=0.95, scale_span=0.1,
                 shift_prob=0.0, shift_max=(0, 0), plain=False):
    """ss_batch_plan_aug (``plain``: ss_batch_plan) through the C ABI, outputs poisoned first: every element must be written."""
    idx = indices if isinstance(indices, torch.Tensor) else i32(indices)
    B = idx.numel()
    t = dict(x_off=i32(x_off), x_len=i32(x_len), y=torch.tensor(np.asarray(y), dtype=torch.int64, device="cuda"))
    has_roi = r_off is not None
    if has_roi:
        t["r_off"], t["r_len"] = i32(r_off), i32(r_len)
    maps = torch.full((3, B, max_t), -77, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    y_out = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    row_scale = torch.full((B,), -77.0, dtype=torch.float32, device="cuda")
    row_shift = torch.full((B, 2), -77, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    head = (idx.data_ptr(), B, t["x_off"].data_ptr(), t["x_len"].data_ptr(), L.ptr(t.get("r_off")), L.ptr(t.get("r_len")),
            t["y"].data_ptr(), len(x_len), max_t, int(augment), first_row, seed, noise_prob, drop_prob, drop_max)
    outs = (maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr() if has_roi else None, lens.data_ptr(), y_out.data_ptr())
    if plain:
        L.call("ss_batch_plan", *head, *outs, err.data_ptr(), L.stream())
    else:
        L.call("ss_batch_plan_aug", *head, warp_prob, warp_lo_pm, warp_hi_pm, scale_prob, scale_lo, scale_span, shift_prob,
               shift_max[0], shift_max[1], *outs, row_scale.data_ptr(), row_shift.data_ptr(), err.data_ptr(), L.stream())
    sync()
    m = maps.cpu().numpy()
    return dict(xmap=m[0], nmap=m[1], rmap=m[2] if has_roi else None, lens=lens.cpu().numpy(), y_out=y_out.cpu().numpy(),
                row_scale=row_scale.cpu().numpy(), row_shift=row_shift.cpu().numpy(), bad=bool(err.item()))


def assert_plan_equal(got, ref, policy=True):
    for key in ("xmap", "nmap", "lens", "y_out"):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
    if ref["rmap"] is None:
        assert got["rmap"] is None
    else:
        assert np.array_equal(got["rmap"], ref["rmap"])
    assert got["bad"] == ref["bad"]
    if policy:
        assert np.array_equal(bits(got["row_scale"]), bits(ref["row_scale"]))
        assert got["row_shift"].dtype == np.int32 and np.array_equal(got["row_shift"], ref["row_shift"])


def gather_u8_shift(L, Rs_d, hw, rmap, row_shift, rows_per_clip, mx, my):
    rm, sh = i32(rmap), i32(row_shift)
    out = torch.full((rm.numel(),) + hw, 0xA5, dtype=torch.uint8, device="cuda")
    L.call("ss_batch_gather_u8_shift", Rs_d.data_ptr(), hw[0], hw[1], rm.data_ptr(), rm.numel(), sh.data_ptr(), rows_per_clip, mx,
           my, out.data_ptr(), L.stream())
    sync()
    return out.cpu().numpy().reshape(tuple(np.shape(rmap)) + hw)


# ------------------------------------------------------------------------------------------------ (a) policy off
@pytest.mark.parametrize("max_t", [16, 90])
def test_policy_off_is_the_present_plan(L, clips, max_t):
    """All three probabilities 0: ss_batch_plan_aug == ss_batch_plan (both on the device) == the restatement; scale 1, shift 0."""
    c = clips[(32, 32)]
    rng = np.random.default_rng(max_t)
    for tables in (c.tables, c.tables[:2] + (None, None)):
        for augment in (True, False):
            for first_row in (0, 2 ** 32 - 5, 2 ** 63 + 11):
                idx = np.concatenate([np.arange(len(CLIPS)), rng.integers(0, len(CLIPS), 4)])
                plain = run_plan_aug(L, idx, *tables, c.y, max_t, augment, first_row, SEED, plain=True)
                got = run_plan_aug(L, idx, *tables, c.y, max_t, augment, first_row, SEED, shift_max=(4, 2))
                assert_plan_equal(got, plain, policy=False)
                assert_plan_equal(got, P.plan(idx, *tables, c.y, max_t, augment, first_row, SEED), policy=False)
                assert np.all(got["row_scale"] == 1) and not got["row_shift"].any()


def test_batch_without_a_policy_is_unchanged(L, clips):
    """``policy=None`` issues exactly the three launches it issued before and gives the batch the plain restatement describes;
    a policy with nothing switched on gives the same bytes (noise included) through the three new entry points."""
    import silent_speech_amd as ss

    c = clips[(48, 96)]
    store = c.store(16)
    idx = np.arange(len(CLIPS))
    L.PROFILE = {}
    try:
        X, T, R, y = store.batch(idx.tolist(), augment=True, rng="philox", seed=SEED, first_row=40)
        sync()
        tags = list(L.PROFILE)
    finally:
        L.PROFILE = None
    assert tags == ["ss_batch_plan", "ss_batch_gather_f32", "ss_batch_gather_u8"]
    ref = P.plan(idx, *c.tables, c.y, 16, True, 40, SEED)
    Xc, Tc, Rc = X.cpu().numpy(), T.cpu().numpy().copy(), R.cpu().numpy()
    assert np.array_equal(Tc, ref["lens"]) and np.array_equal(Rc, P.gather(c.Rs, ref["rmap"], c.hw))
    X0 = P.gather(c.Xs, ref["xmap"], (D,))
    plain_rows = np.flatnonzero(~ref["noisy"])
    assert len(plain_rows) and all(np.array_equal(Xc[b], X0[b]) for b in plain_rows)
    L.PROFILE = {}
    try:
        X2, T2, R2, y2 = store.batch(idx.tolist(), augment=True, rng="philox", seed=SEED, first_row=40, policy=ss.AugmentPolicy())
        sync()
        tags = list(L.PROFILE)
    finally:
        L.PROFILE = None
    assert tags == ["ss_batch_plan_aug", "ss_batch_gather_f32_aug", "ss_batch_gather_u8_shift"]
    assert np.array_equal(bits(X2.cpu().numpy()), bits(Xc)) and np.array_equal(R2.cpu().numpy(), Rc)
    assert np.array_equal(T2.cpu().numpy(), Tc)
    store.check()


# ------------------------------------------------------------------------------------------------ (b) forced policies
@pytest.mark.parametrize("which", sorted(POLICIES))
@pytest.mark.parametrize("max_t", [16, 90])
def test_forced_policy_equals_the_restatement(L, clips, which, max_t):
    """B = 16, three seeds: maps, lengths, labels, the bits of row_scale and row_shift."""
    c = clips[(32, 32)]
    pol = POLICIES[which]
    seen = dict(warped=0, shifted=0, scaled=0, short_roi=0)
    for n, seed in enumerate(SEEDS):
        rng = np.random.default_rng(n)
        idx = np.concatenate([rng.permutation(len(CLIPS)), rng.integers(0, len(CLIPS), 4)])
        assert len(idx) == 16
        for first_row in (3, 2 ** 32 - 7):
            ref = A.plan(idx, *c.tables, c.y, max_t, True, first_row, seed, **pol)
            assert_plan_equal(run_plan_aug(L, idx, *c.tables, c.y, max_t, True, first_row, seed, **pol), ref)
            seen["warped"] += int(ref["warped"].sum())
            seen["shifted"] += int(ref["row_shift"].any(axis=1).sum())
            seen["scaled"] += int((ref["row_scale"] != 1).sum())
        # a store without ROI frames: no rmap, no shift
        ref = A.plan(idx, *c.tables[:2], None, None, c.y, max_t, True, 5, seed, **pol)
        got = run_plan_aug(L, idx, *c.tables[:2], None, None, c.y, max_t, True, 5, seed, **pol)
        assert_plan_equal(got, ref)
        assert not got["row_shift"].any()
    assert (seen["warped"] > 0) == (which in ("warp", "all"))
    assert (seen["shifted"] > 0) == (which in ("shift", "all"))
    assert (seen["scaled"] > 0) == (which in ("scale", "all"))


def test_store_batch_with_every_policy_forced(L, clips):
    """``batch(policy=)`` end to end on 48x96 frames: T, y, R (warped and shifted) and the rows of X the plan leaves without
    noise (warped, dropped from and scaled) are exactly what the restatement gives."""
    import silent_speech_amd as ss

    c = clips[(48, 96)]
    pol = ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=1.0, roi_shift_prob=1.0, roi_shift_max=(4, 2))
    kw = A.policy_kwargs(pol)
    n_plain = 0
    for max_t in (16, 90):
        store = c.store(max_t)
        idx = np.concatenate([np.arange(len(CLIPS)), [6, 10, 7, 11]])
        for first_row in (0, 16):
            X, T, R, y = store.batch(torch.tensor(idx, dtype=torch.int32, device="cuda"), augment=True, rng="philox", seed=SEED,
                                     first_row=first_row, policy=pol)
            sync()
            ref = A.plan(idx, *c.tables, c.y, max_t, True, first_row, SEED, **kw)
            assert np.array_equal(T.cpu().numpy(), ref["lens"]) and np.array_equal(y.cpu().numpy(), ref["y_out"])
            assert np.array_equal(R.cpu().numpy(), A.gather_shifted(c.Rs, ref["rmap"], ref["row_shift"]))
            Xc, X0 = X.cpu().numpy(), A.gather_scaled(c.Xs, ref["xmap"], ref["row_scale"])
            for b in range(16):
                assert not Xc[b, ref["lens"][b]:].any()
                if not ref["noisy"][b]:
                    assert np.array_equal(bits(Xc[b]), bits(X0[b]))
                    n_plain += 1
                elif ref["lens"][b]:
                    diff = Xc[b, :ref["lens"][b]] - X0[b, :ref["lens"][b]]
                    assert diff.any() and np.abs(diff).max() < 0.01 * 1.05 * 7     # noise of std 0.01, scaled: within 7 sigma
        store.check()
    assert n_plain > 0


# ------------------------------------------------------------------------------------------------ (c) feature values
def test_scaled_features_are_one_rounded_product(L, clips):
    import silent_speech_amd as ss

    c = clips[(32, 32)]
    Xs_d = torch.from_numpy(c.Xs).cuda()
    idx = np.concatenate([np.arange(len(CLIPS)), [6, 10, 7, 11]])
    for max_t in (16, 90):
        ref = A.plan(idx, *c.tables, c.y, max_t, True, 9, SEED, **POLICIES["all"])
        xmap, nmap, sc = i32(ref["xmap"]), i32(ref["nmap"]), torch.from_numpy(ref["row_scale"]).cuda()
        # noise off: exactly fl(src * s)
        out = torch.full((16, max_t, D), 7.0, device="cuda")
        L.call("ss_batch_gather_f32_aug", Xs_d.data_ptr(), D, xmap.data_ptr(), 16 * max_t, nmap.data_ptr(), 0.0, 5, 0, sc.data_ptr(),
               max_t, out.data_ptr(), L.stream())
        sync()
        assert np.array_equal(bits(out.cpu().numpy()), bits(A.gather_scaled(c.Xs, ref["xmap"], ref["row_scale"])))
        # noise on: exactly fl(X of the same policy without the scale * s), same seed and rows
        store = c.store(max_t)
        on = ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=1.0, roi_shift_prob=1.0, roi_shift_max=(4, 2))
        off = ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=0.0, roi_shift_prob=1.0, roi_shift_max=(4, 2))
        Xon = store.batch(idx.tolist(), augment=True, rng="philox", seed=SEED, first_row=9, policy=on)[0].cpu().numpy()
        Xoff = store.batch(idx.tolist(), augment=True, rng="philox", seed=SEED, first_row=9, policy=off)[0].cpu().numpy()
        s = A.plan(idx, *c.tables, c.y, max_t, True, 9, SEED, **A.policy_kwargs(on))["row_scale"]
        assert ref["noisy"].any() and np.all(s != 1)
        assert np.array_equal(bits(Xon), bits((Xoff * s[:, None, None]).astype(np.float32)))
        noisy_rows = np.flatnonzero(ref["noisy"] & (ref["lens"] > 0))
        assert all(not np.array_equal(Xoff[b], P.gather(c.Xs, ref["xmap"], (D,))[b]) for b in noisy_rows)


# ------------------------------------------------------------------------------------------------ (d) ROI gather
def _shift_case(L, c, shifts, mx, my, rows_per_clip=3):
    """One launch: clip n of the batch is shifted by shifts[n]; its rows map to the first frame of the store, the last one, a
    random one -- and every seventh row is padding."""
    rng = np.random.default_rng(len(shifts))
    n = len(shifts)
    N = len(c.Rs)
    rmap = rng.integers(0, N, (n, rows_per_clip)).astype(np.int32)
    rmap[:, 0] = np.where(np.arange(n) % 2 == 0, 0, N - 1)
    rmap.reshape(-1)[6::7] = -1
    got = gather_u8_shift(L, torch.from_numpy(c.Rs).cuda(), c.hw, rmap, np.asarray(shifts, np.int32), rows_per_clip, mx, my)
    want = A.gather_shifted(c.Rs, rmap, np.asarray(shifts, np.int32))
    assert np.array_equal(got, want)
    assert (rmap[:, 0] == 0).any() and (rmap[:, 0] == N - 1).any() and (rmap < 0).any()


def test_shifted_gather_32x32_every_shift_of_the_box(L, clips):
    _shift_case(L, clips[(32, 32)], [(dx, dy) for dx in range(-8, 9) for dy in range(-4, 5)], 8, 4)


@pytest.mark.parametrize("hw", [(32, 32), (48, 96), (20, 12)])
def test_shifted_gather_extremes_and_every_dx(L, clips, hw):
    """+-(W-1), +-(H-1) in every combination, every dx with a dy that cycles through its range, every dy with a dx that does."""
    H, W = hw
    shifts = [(sx * (W - 1), sy * (H - 1)) for sx in (-1, 0, 1) for sy in (-1, 0, 1)]
    shifts += [(dx, (dx * 7) % (2 * H - 1) - (H - 1)) for dx in range(-(W - 1), W)]
    shifts += [((dy * 5) % (2 * W - 1) - (W - 1), dy) for dy in range(-(H - 1), H)]
    _shift_case(L, clips[hw], shifts, W - 1, H - 1)


def test_shifted_gather_20x12_every_shift(L, clips):
    """The per-byte path (W % 16 != 0): every (dx, dy) there is."""
    _shift_case(L, clips[(20, 12)], [(dx, dy) for dx in range(-11, 12) for dy in range(-19, 20)], 11, 19, rows_per_clip=2)


def test_shifted_gather_clamps_whatever_the_table_holds(L, clips):
    """Shifts past the frame (they cannot come out of the planner) read the replicated edge, not another frame."""
    big = 2 ** 31 - 1
    for hw in ((32, 32), (20, 12)):
        H, W = hw
        _shift_case(L, clips[hw], [(W, H), (-W, -H), (big, -big - 1), (-big - 1, big), (W + 5, 0), (0, -H - 5), (1000, 1000)], W - 1, H - 1)


# ------------------------------------------------------------------------------------------------ (e) shards
def test_shards_of_a_batch_equal_the_whole_batch(L, clips):
    import silent_speech_amd as ss

    c = clips[(32, 32)]
    pol = ss.AugmentPolicy.lineage(time_warp_prob=0.7, scale_prob=0.7, roi_shift_prob=0.7, roi_shift_max=(4, 2))
    for max_t in (16, 90):
        store = c.store(max_t)
        idx = torch.tensor(np.concatenate([np.arange(len(CLIPS)), [6, 10, 7, 11]]), dtype=torch.int32, device="cuda")
        base = 2 ** 32 - 8
        whole = [t.clone() for t in store.batch(idx, augment=True, rng="philox", seed=SEED, first_row=base, policy=pol)]
        same = [t.clone() for t in store.batch(idx, augment=True, rng="philox", seed=SEED, first_row=base, batch_first_row=base, policy=pol)]
        parts = []
        for lo, hi in ((0, 6), (6, 11), (11, 16)):
            parts.append([t.clone() for t in store.batch(idx[lo:hi], augment=True, rng="philox", seed=SEED, first_row=base + lo,
                                                         batch_first_row=base, policy=pol)])
        sync()
        for n in range(4):
            cat = torch.cat([p[n] for p in parts], 0)
            assert cat.shape == whole[n].shape and torch.equal(cat, whole[n]), n
            assert torch.equal(same[n], whole[n])
        assert whole[0].abs().sum() > 0 and whole[2].any()
        store.check()


# ------------------------------------------------------------------------------------------------ (f) out of range
def test_out_of_range_device_index_with_a_policy(L, clips):
    import silent_speech_amd as ss

    c = clips[(32, 32)]
    n = len(CLIPS)
    idx = [0, n, -1, 7, 2 ** 31 - 1]
    ref = A.plan(idx, *c.tables, c.y, 16, True, 0, SEED, **POLICIES["all"])
    got = run_plan_aug(L, idx, *c.tables, c.y, 16, True, 0, SEED, **POLICIES["all"])
    assert_plan_equal(got, ref)
    assert got["bad"] and got["lens"][[1, 2, 4]].tolist() == [0, 0, 0] and got["lens"][0] > 0 and got["lens"][3] > 0
    assert np.all(got["row_scale"][[1, 2, 4]] == 1) and not got["row_shift"][[1, 2, 4]].any()
    assert got["row_scale"][0] != 1 and got["row_scale"][3] != 1
    store = c.store(16)
    pol = ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=1.0, roi_shift_prob=1.0, roi_shift_max=(4, 2))
    with pytest.raises(IndexError):
        store.batch(idx, augment=True, rng="philox", policy=pol)      # host indices: before any launch
    store.check()
    X, T, R, y = store.batch(torch.tensor(idx, dtype=torch.int32, device="cuda"), augment=True, rng="philox", seed=SEED, policy=pol)
    sync()
    for b in (1, 2, 4):
        assert int(T[b]) == 0 and not X[b].any() and not R[b].any() and int(y[b]) == 0
    assert int(T[0]) > 0 and int(T[3]) > 0 and X[3].any() and R[3].any()
    with pytest.raises(IndexError, match="outside"):
        store.check()
    store.check()


# ------------------------------------------------------------------------------------------------ (g) argument errors
def test_entry_points_refuse_bad_arguments(L, clips):
    import silent_speech_amd as ss

    c = clips[(32, 32)]
    idx = np.arange(4)
    for bad in (dict(shift_prob=1.5), dict(warp_prob=-0.25), dict(scale_prob=1.0001), dict(warp_lo_pm=0), dict(warp_hi_pm=4001),
                dict(warp_lo_pm=1300), dict(scale_lo=0.0), dict(scale_span=-1.0), dict(shift_max=(-1, 0))):
        with pytest.raises(RuntimeError, match="argument"):
            run_plan_aug(L, idx, *c.tables, c.y, 16, True, 0, SEED, **bad)
    Rs_d = torch.from_numpy(c.Rs).cuda()
    rmap, sh = np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32)
    for mx, my in ((32, 0), (0, 32), (100, 100), (-1, 0)):
        with pytest.raises(RuntimeError, match="argument"):
            gather_u8_shift(L, Rs_d, (32, 32), rmap, sh, 2, mx, my)
    gather_u8_shift(L, Rs_d, (32, 32), rmap, sh, 2, 31, 31)
    store = c.store(16)
    with pytest.raises(ValueError, match="roi_shift_max"):
        store.batch([0, 1], augment=True, rng="philox", policy=ss.AugmentPolicy(roi_shift_prob=1.0, roi_shift_max=(32, 0)))
    with pytest.raises(ValueError, match="philox"):
        store.batch([0, 1], augment=True, rng="device", policy=ss.AugmentPolicy())
    with pytest.raises(ValueError, match="philox"):
        store.batch([0, 1], augment=False, rng="philox", policy=ss.AugmentPolicy())
    store.check()


# ------------------------------------------------------------------------------------------------ (h) fit
def test_fit_with_an_augment_policy(L, tmp_path, monkeypatch):
    """Two epochs on a tiny clip directory: finite losses, the same run from the same seed, another one without the policy.

    What "the same run" can mean here: the training batches are a pure function of (seed, draw index) -- every batch of two runs
    is compared bit for bit.  ``Trainer.step`` itself sums its loss and several gradients with f32 atomics whose order is not
    fixed (as it did before the policy existed), so two histories agree to f32 summation noise, not to the bit: a sum of up to
    ~10^3 terms reordered moves by at most ~10^3 * 2^-24 = 6e-5 of its size; the losses are compared to rtol 1e-4.  (Measured:
    train loss 1.068958044 against 1.068957965, 7e-8 apart; the run without the policy gives 1.0665532.)"""
    import silent_speech_amd as ss
    from silent_speech_amd import data as Dm
    from silent_speech_amd import harness as Hn

    rng = np.random.default_rng(0)
    clip_dir = tmp_path / "clips_npz"
    clip_dir.mkdir()
    words = ["aura", "no", "yes"]
    for k in range(30):
        T = int(rng.integers(14, 22))
        X = (0.05 * rng.normal(size=(T, 20))).astype(np.float32)
        X[:, (k % 3) * 4:(k % 3) * 4 + 4] += 0.5
        roi = rng.integers(0, 256, (T, 32, 32), dtype=np.uint8)
        Dm.save_clip(str(clip_dir / f"{k:03d}.npz"), X, np.arange(T), words[k % 3], "me", np.arange(4), roi)
    pol = ss.AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(4, 2))
    seen = []
    real_batch = ss.DeviceClipStore.batch

    def recording_batch(self, *args, **kw):
        out = real_batch(self, *args, **kw)
        if kw.get("augment"):                       # the training batches; validation is never augmented
            seen.append((kw.get("policy"), [t.clone() for t in out]))
        else:
            assert kw.get("policy") is None
        return out

    monkeypatch.setattr(ss.DeviceClipStore, "batch", recording_batch)

    def run(policy):
        hist = []
        del seen[:]
        Hn.fit(str(clip_dir), str(tmp_path / "m.pt"), epochs=2, batch_size=8, patience=3, max_t=24, lr=3e-3, log=lambda *a: None,
               plan="device", history=hist, augment_policy=policy)
        return hist, list(seen)

    (a, batches_a), (b, batches_b), (plain, batches_plain) = run(pol), run(pol), run(None)
    print("policy", a, "again", b, "plain", plain)
    keys = ("train_loss", "val_loss", "train_acc", "val_acc")
    assert len(a) == 2 and all(np.isfinite(h[key]) for h in a for key in keys)
    assert len(batches_a) == len(batches_b) == len(batches_plain) > 2
    assert all(p is pol for p, _ in batches_a) and all(p is None for p, _ in batches_plain)
    for (_, ta), (_, tb) in zip(batches_a, batches_b):
        assert all(torch.equal(u, v) for u, v in zip(ta, tb))
    assert any(not torch.equal(ta[0], tp[0]) for (_, ta), (_, tp) in zip(batches_a, batches_plain))
    assert any(not torch.equal(ta[2], tp[2]) for (_, ta), (_, tp) in zip(batches_a, batches_plain))
    assert len(b) == 2 and all(np.isclose(ha[key], hb[key], rtol=1e-4, atol=0) for ha, hb in zip(a, b) for key in ("train_loss", "val_loss"))
    assert not np.allclose([h["train_loss"] for h in a], [h["train_loss"] for h in plain], rtol=1e-4, atol=0)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(clip_dir), str(tmp_path / "m.pt"), epochs=1, plan="host", augment_policy=pol)
