"""GPU: the masking augmentations of the device-planned path (ss_batch_plan_mask, ss_batch_mask_apply,
``DeviceClipStore.batch(policy=)`` with a mask on, ``harness.fit(augment_policy=)``) against tests/mask_plan_ref.py -- integer maps
and tables, float32 bit patterns and bytes, all compared exactly.

The draw indices the cases run at are picked on the CPU from the restatement (``chosen``) so that every mask occurs active and
inactive, with its smallest and its largest width, and with a rectangle on each edge of the frame and over the whole frame; the
test that compares the plans asserts that they do.

Run on the MI355X box with ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest
import torch

import aug_plan_ref as A
import batch_plan_ref as P
import mask_plan_ref as M
from gpu_support import L, bits, sync  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
MAX_T = 24
# (T, Tr): feature lengths 3, 8, 9, 24, 31, 40 (the last two are trimmed to max_t), an ROI track shorter than its features, and a
# clip without ROI frames
CLIPS = [(3, 3), (8, 8), (9, 9), (24, 24), (31, 31), (40, 40), (31, 20), (24, None)]
GEOMETRIES = {"84_64x64": (84, (64, 64)), "83_12x20": (83, (12, 20))}  # D, (H, W): aligned rows and W % 16 == 0; neither
IDX7 = np.array([0, 1, 2, 3, 5, 6, 7])
IDX70 = np.arange(70) % len(CLIPS)
AUG = dict(warp_prob=0.5, scale_prob=0.5, shift_prob=0.5, shift_max=(2, 1))
WANTED_MAIN = {"time_on", "time_off", "band_on", "band_off", "cut_on", "cut_off", "tw1", "twcap", "cw1", "left", "right", "top", "bottom"}
WANTED_FULL = {"cwD", "full"}


def main_masks(D, hw):
    return dict(time_mask_prob=0.6, time_mask_max=6, feat_mask_prob=0.6, feat_mask_max=20, cutout_prob=0.6,
                cutout_max=(max(2, hw[1] // 4), max(2, hw[0] // 3)))


def full_masks(D, hw):
    return dict(time_mask_prob=1.0, time_mask_max=100, feat_mask_prob=1.0, feat_mask_max=D + 5, cutout_prob=1.0, cutout_max=(hw[1], hw[0]))


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda")


class Clips:
    """The synthetic store: files on disk (for DeviceClipStore), the concatenated arrays and the tables (for the restatement)."""

    def __init__(self, tmp, D, hw):
        rng = np.random.default_rng(D * 100 + hw[0])
        self.D, self.hw, self.files, xs, rs = D, hw, [], [], []
        for n, (T, Tr) in enumerate(CLIPS):
            X = rng.normal(size=(T, D)).astype(np.float32)
            arrays = dict(X=X, ts=np.arange(T), label="w%d" % (n % 3), speaker="me", idxs=np.arange(4))
            if Tr is not None:
                arrays["roi"] = rng.integers(1, 256, (Tr,) + hw, dtype=np.uint8)  # no zero byte: a zero in R is padding or a mask
                rs.append(arrays["roi"])
            f = str(tmp / f"{n:02d}.npz")
            np.savez(f, **arrays)
            self.files.append(f)
            xs.append(X)
        self.Xs, self.Rs = np.concatenate(xs, 0), np.concatenate(rs, 0)
        self.tables = P.store_tables(CLIPS)
        self.y = np.array([n % 3 for n in range(len(CLIPS))], np.int64)
        self._store = None

    @property
    def store(self):
        if self._store is None:
            import silent_speech_amd as ss

            self._store = ss.DeviceClipStore(self.files, {"w0": 0, "w1": 1, "w2": 2}, max_t=MAX_T)
        return self._store


@pytest.fixture(scope="module")
def clips(tmp_path_factory, L):
    return {k: Clips(tmp_path_factory.mktemp("mask_" + k), D, hw) for k, (D, hw) in GEOMETRIES.items()}


# ------------------------------------------------------------------------------------------------ restatement and coverage
def ref_plan(c, idx, first_row, seed, masks, aug=AUG):
    """The planner's restatement (``aug`` None: ss_batch_plan) with the masks planned behind it -> dict(before=, xmap, nmap,
    rmap, lens, row_mask)."""
    if aug is None:
        before = P.plan(idx, *c.tables, c.y, MAX_T, True, first_row, seed)
    else:
        before = A.plan(idx, *c.tables, c.y, MAX_T, True, first_row, seed, **aug)
    xmap, nmap, rmap, lens, table = M.plan_mask(before["xmap"], before["nmap"], before["rmap"], before["lens"], first_row, seed, c.D,
                                                c.hw[0], c.hw[1], True, **masks)
    return dict(before=before, xmap=xmap, nmap=nmap, rmap=rmap, lens=lens, row_mask=table)


def covered(c, ref, masks):
    """The names of the wanted cases that occur in one planned batch."""
    H, W = c.hw
    n = ref["lens"]
    t0, tw, col0, cw, x0, y0, rw, rh = ref["row_mask"].astype(np.int64).T
    has_roi = (n > 0) & (ref["before"]["rmap"][:, 0] >= 0)
    got = set()
    flag = lambda name, cond: got.add(name) if np.any(cond) else None  # noqa: E731
    flag("time_on", tw > 0), flag("time_off", (tw == 0) & (n >= 8))
    flag("band_on", cw > 0), flag("band_off", (cw == 0) & (n > 0))
    flag("cut_on", rw > 0), flag("cut_off", (rw == 0) & has_roi)
    flag("tw1", tw == 1), flag("twcap", (tw > 1) & (tw == np.minimum(masks["time_mask_max"], n // 4)))
    flag("cw1", cw == 1), flag("cwD", (cw == c.D) & (masks["feat_mask_max"] >= c.D))
    cut = rw > 0
    flag("left", cut & (x0 == 0)), flag("right", cut & (x0 + rw == W)), flag("top", cut & (y0 == 0)), flag("bottom", cut & (y0 + rh == H))
    flag("full", (rw == W) & (rh == H) & (tuple(masks["cutout_max"]) == (W, H)))
    return got


def chosen(c):
    """[(idx, first_row, masks)] for one geometry.  B = 7: first rows 0, 7, 14, ... taken greedily while they add a wanted case of
    ``main_masks``, then two first rows for ``full_masks`` that put a band of all D columns and a whole-frame rectangle on row 3 (a
    clip with ROI frames): the band and the rectangle depend on the draw index alone, so the index is searched in one vectorised
    pass over the restatement.  B = 70: two first rows, one of them across the 2^32 boundary of the counter."""
    main, full = main_masks(c.D, c.hw), full_masks(c.D, c.hw)
    cases, have = [], set()
    for first_row in range(0, 7 * 400, 7):
        new = covered(c, ref_plan(c, IDX7, first_row, SEED, main), main) & WANTED_MAIN
        if new - have:
            cases.append((IDX7, first_row, main))
            have |= new
        if have == WANTED_MAIN:
            break
    table = M.decisions(np.full(1 << 18, MAX_T), True, 3, SEED, c.D, c.hw[0], c.hw[1], **full).astype(np.int64)
    for hit in ((table[:, 3] == c.D), (table[:, 6] == c.hw[1]) & (table[:, 7] == c.hw[0])):
        assert hit.any()
        cases.append((IDX7, int(np.flatnonzero(hit)[0]), full))  # (draw 3 + j is row 3 of the batch whose first row is j)
    cases += [(IDX70, 3, main), (IDX70, 2 ** 32 - 7, main)]
    return cases


@pytest.fixture(scope="module")
def cases(clips):
    return {k: chosen(c) for k, c in clips.items()}


# ------------------------------------------------------------------------------------------------ the entry points, directly
def run_planner(L, c, idx, first_row, seed, aug):
    """ss_batch_plan (``aug`` None) or ss_batch_plan_aug through the C ABI -> device maps (3, B, max_t) and lens."""
    x_off, x_len, r_off, r_len = c.tables
    idx_d, B = i32(idx), len(idx)
    t = [i32(x_off), i32(x_len), i32(r_off), i32(r_len), torch.tensor(c.y, dtype=torch.int64, device="cuda")]
    maps = torch.full((3, B, MAX_T), -77, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    y_out = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    row_scale, row_shift = torch.empty(B, device="cuda"), torch.empty(B, 2, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    head = (idx_d.data_ptr(), B, *[v.data_ptr() for v in t], len(x_len), MAX_T, 1, first_row, seed, 0.7, 0.35, 2)
    outs = (maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), lens.data_ptr(), y_out.data_ptr())
    if aug is None:
        L.call("ss_batch_plan", *head, *outs, err.data_ptr(), L.stream())
    else:
        k = dict(warp_prob=0.0, warp_lo_pm=800, warp_hi_pm=1200, scale_prob=0.0, scale_lo=0.95, scale_span=0.1, shift_prob=0.0,
                 shift_max=(0, 0))
        k.update(aug)
        L.call("ss_batch_plan_aug", *head, k["warp_prob"], k["warp_lo_pm"], k["warp_hi_pm"], k["scale_prob"], k["scale_lo"],
               k["scale_span"], k["shift_prob"], k["shift_max"][0], k["shift_max"][1], *outs, row_scale.data_ptr(),
               row_shift.data_ptr(), err.data_ptr(), L.stream())
    sync()
    assert not err.item()
    return maps, lens


def mask_args(D, hw, masks, augment=1, first_row=0, seed=SEED, fill=128):
    """ss_batch_plan_mask's scalars between ``lens`` and ``row_mask`` (B and max_t are put in front by the caller)."""
    k = dict(M.DEFAULTS, **masks)
    return (D, hw[0], hw[1], augment, first_row, seed, float(k["time_mask_prob"]), k["time_mask_max"],
            M.STREAMS.index(k["time_mask_streams"]), M.FILLS.index(k["time_mask_fill"]), float(k["feat_mask_prob"]), k["feat_mask_max"],
            float(k["cutout_prob"]), k["cutout_max"][0], k["cutout_max"][1], fill)


def run_plan_mask(L, maps, lens, D, hw, masks, first_row, seed, rmap=True, **kw):
    """ss_batch_plan_mask on clones of the planner's outputs, row_mask poisoned first -> numpy (xmap, nmap, rmap, lens, row_mask)."""
    maps, lens = maps.clone(), lens.clone()
    B = lens.numel()
    table = torch.full((B, 8), -77, dtype=torch.int32, device="cuda")
    L.call("ss_batch_plan_mask", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr() if rmap else None, lens.data_ptr(), B,
           MAX_T, *mask_args(D, hw, masks, first_row=first_row, seed=seed, **kw), table.data_ptr(), L.stream())
    sync()
    m = maps.cpu().numpy()
    return m[0], m[1], m[2], lens.cpu().numpy(), table.cpu().numpy()


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_planned_masks_equal_the_restatement(L, clips, cases, geometry):
    """Maps, lens and row_mask, exactly: both fills, the three stream settings, either planner in front, B = 7 and 70 -- at draw
    indices that are asserted to produce every wanted case."""
    c = clips[geometry]
    seen = set()
    for idx, first_row, masks in cases[geometry]:
        for aug in (AUG, None):
            maps, lens = run_planner(L, c, idx, first_row, SEED, aug)
            for fill in M.FILLS:
                for streams in M.STREAMS:
                    mk = dict(masks, time_mask_fill=fill, time_mask_streams=streams)
                    ref = ref_plan(c, idx, first_row, SEED, mk, aug)
                    assert np.array_equal(maps.cpu().numpy(), np.stack([ref["before"][k] for k in ("xmap", "nmap", "rmap")]))
                    gx, gn, gr, gl, table = run_plan_mask(L, maps, lens, c.D, c.hw, mk, first_row, SEED)
                    where = (geometry, len(idx), first_row, aug is None, fill, streams)
                    assert table.dtype == np.int32 and np.array_equal(table, ref["row_mask"]), where
                    assert np.array_equal(gx, ref["xmap"]) and np.array_equal(gn, ref["nmap"]) and np.array_equal(gr, ref["rmap"]), where
                    assert np.array_equal(gl, ref["lens"]) and np.array_equal(gl, ref["before"]["lens"]), where
                    seen |= covered(c, ref, mk)
            # a store without ROI frames (rmap NULL): the time mask and the band as before, no rectangle
            off = dict(masks, cutout_prob=0.0)
            gx, gn, gr, gl, table = run_plan_mask(L, maps, lens, c.D, (0, 0), off, first_row, SEED, rmap=False)
            ref = M.plan_mask(maps[0].cpu().numpy(), maps[1].cpu().numpy(), None, lens.cpu().numpy(), first_row, SEED, c.D, **off)
            assert np.array_equal(gx, ref[0]) and np.array_equal(gn, ref[1]) and np.array_equal(gr, maps[2].cpu().numpy())
            assert np.array_equal(table, ref[4]) and not table[:, 4:].any()
    assert seen >= WANTED_MAIN | WANTED_FULL, (WANTED_MAIN | WANTED_FULL) - seen


def test_masks_off_and_empty_rows_edit_nothing(L, clips):
    """augment = 0, every probability 0, every maximum 0: the maps come back as they went in and the table is zero; a row the
    planner left empty (an index outside the store) is eight zeros whatever the policy."""
    c = clips["84_64x64"]
    maps, lens = run_planner(L, c, IDX70, 3, SEED, AUG)
    on = full_masks(c.D, c.hw)
    for mk, kw in ((on, dict(augment=0)), (dict(on, time_mask_prob=0.0, feat_mask_prob=0.0, cutout_prob=0.0), {}),
                   (dict(on, time_mask_max=0, feat_mask_max=0, cutout_max=(0, 0)), {}), ({}, {})):
        gx, gn, gr, gl, table = run_plan_mask(L, maps, lens, c.D, c.hw, mk, 3, SEED, **kw)
        assert np.array_equal(np.stack([gx, gn, gr]), maps.cpu().numpy()) and np.array_equal(gl, lens.cpu().numpy())
        assert not table.any()
    empty_maps = torch.full((3, 4, MAX_T), -1, dtype=torch.int32, device="cuda")
    empty_lens = torch.zeros(4, dtype=torch.int64, device="cuda")
    gx, gn, gr, gl, table = run_plan_mask(L, empty_maps, empty_lens, c.D, c.hw, on, 3, SEED)
    assert np.all(np.stack([gx, gn, gr]) == -1) and not gl.any() and not table.any()


# ------------------------------------------------------------------------------------------------ batch(policy=)
def policy_of(ss, masks, aug=AUG, **more):
    return ss.AugmentPolicy(time_warp_prob=aug["warp_prob"], scale_prob=aug["scale_prob"], roi_shift_prob=aug["shift_prob"],
                            roi_shift_max=aug["shift_max"], **dict(masks, **more))


def expected_batch(c, ref, X_off, R_off, fill, masks):
    """What the masks make of the unmasked batch of the same seed and rows, wherever that is exact: -> (X, R, fresh) with ``fresh``
    (B, max_t) bool = the "hold" rows of noisy clips, whose features carry noise of their own (compared apart)."""
    X, R = X_off.copy(), R_off.copy()
    k = dict(M.DEFAULTS, **masks)
    feat, roi, hold = k["time_mask_streams"] != "roi", k["time_mask_streams"] != "features", k["time_mask_fill"] == "hold"
    fresh = np.zeros(X.shape[:2], bool)
    for b, (t0, tw, *_rest) in enumerate(ref["row_mask"].astype(np.int64)):
        if not tw:
            continue
        run = slice(t0, t0 + tw)
        if feat:
            X[b, run] = X_off[b, t0 - 1] if hold else 0.0
            fresh[b, run] = hold and bool(ref["before"]["noisy"][b])
        if roi:
            R[b, run] = R_off[b, t0 - 1] if hold else 0
    return (*M.apply(X, R, ref["rmap"], ref["row_mask"], fill), fresh)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_batch_with_masks_against_the_unmasked_batch(L, clips, cases, geometry):
    """``batch(policy=masks on)`` against ``batch(policy=same, masks off)``: outside the masked rows, columns and rectangles equal
    bits; inside, X is 0.0 and R is the fill where the frame is mapped and 0 where it is not; "hold" rows are the held frame -- the
    bytes of R exactly, the features exactly for a clip without noise and within seven noise sigmas (0.01, times the scale factor
    of at most 1.05), but not equal, for a noisy one, whose repeated rows take fresh noise."""
    import silent_speech_amd as ss

    c = clips[geometry]
    store = c.store
    n_exact = n_fresh = n_fill = 0
    settings = [("zero", "both"), ("hold", "both"), ("zero", "features"), ("hold", "roi")]
    for idx, first_row, masks in cases[geometry]:
        idx_d = i32(idx)
        kw = dict(augment=True, rng="philox", seed=SEED, first_row=first_row)
        X_off, T_off, R_off, y_off = [t.cpu().numpy().copy() for t in store.batch(idx_d, policy=policy_of(ss, {}), **kw)]
        for fill_mode, streams in settings:
            mk = dict(masks, time_mask_fill=fill_mode, time_mask_streams=streams)
            X, T, R, y = store.batch(idx_d, policy=policy_of(ss, mk, cutout_fill=201), **kw)
            sync()
            ref = ref_plan(c, idx, first_row, SEED, mk)
            assert np.array_equal(T.cpu().numpy(), T_off) and np.array_equal(y.cpu().numpy(), y_off)
            Xe, Re, fresh = expected_batch(c, ref, X_off, R_off, 201, mk)
            Xg, Rg = X.cpu().numpy(), R.cpu().numpy()
            assert np.array_equal(Rg, Re), (geometry, first_row, fill_mode, streams)
            assert np.array_equal(bits(Xg[~fresh]), bits(Xe[~fresh])), (geometry, first_row, fill_mode, streams)
            # the fresh-noise rows: the band is 0.0, the rest the held frame under noise of its own
            for b, t in zip(*np.nonzero(fresh)):
                col0, cw = int(ref["row_mask"][b, 2]), int(ref["row_mask"][b, 3])
                keep = np.ones(c.D, bool)
                keep[col0:col0 + cw] = False
                assert not Xg[b, t, ~keep].any()
                diff = Xg[b, t, keep] - Xe[b, t, keep]
                assert diff.any() and np.abs(diff).max() < 2 * 0.01 * 1.05 * 7   # (both rows carry noise: twice the bound of one)
                n_fresh += 1
            table = ref["row_mask"].astype(np.int64)
            n_exact += int((table[:, 1] > 0).sum())
            n_fill += int((Rg == 201).sum())
            # inside, spelled out: zeros in the band, and the fill on mapped frames only
            for b in np.flatnonzero(table[:, 3]):
                assert not Xg[b, :, table[b, 2]:table[b, 2] + table[b, 3]].any()
            for b in np.flatnonzero(table[:, 6]):
                x0, y0, rw, rh = table[b, 4:]
                rect = Rg[b, :, y0:y0 + rh, x0:x0 + rw]
                mapped = ref["rmap"][b] >= 0
                assert mapped.any() and np.all(rect[mapped] == 201) and not rect[~mapped].any()
    store.check()
    assert n_exact > 0 and n_fresh > 0 and n_fill > 0


def test_shards_of_a_masked_batch_equal_the_whole_batch(L, clips):
    import silent_speech_amd as ss

    for geometry, c in clips.items():
        store = c.store
        idx = i32(IDX70)
        for fill in M.FILLS:
            pol = policy_of(ss, dict(main_masks(c.D, c.hw), time_mask_fill=fill))
            base = 2 ** 32 - 8
            kw = dict(augment=True, rng="philox", seed=SEED, policy=pol)
            whole = [t.clone() for t in store.batch(idx, first_row=base, **kw)]
            parts = [[t.clone() for t in store.batch(idx[lo:hi], first_row=base + lo, batch_first_row=base, **kw)]
                     for lo, hi in ((0, 33), (33, 70))]
            sync()
            for n in range(4):
                cat = torch.cat([p[n] for p in parts], 0)
                assert cat.shape == whole[n].shape and torch.equal(cat, whole[n]), (geometry, fill, n)
            ref = ref_plan(c, IDX70, base, SEED, main_masks(c.D, c.hw))
            assert (ref["row_mask"][:33, [1, 3, 6]] > 0).any(0).all() and (ref["row_mask"][33:, [1, 3, 6]] > 0).any(0).all()
        store.check()


def test_embedded_batch_with_masks(L, clips):
    """``embedded=True``: the feature columns of Z are X of the pixel-path batch of the same call, a zero-masked ROI row holds
    ``store.E0``, every other mapped row its stored embedding; a cutout is refused."""
    import silent_speech_amd as ss

    c = clips["84_64x64"]
    store = ss.DeviceClipStore(c.files, {"w0": 0, "w1": 1, "w2": 2}, max_t=MAX_T)
    torch.manual_seed(5)
    model = ss.BiGRUClassifier(c.D, 3, use_roi=True, roi_emb=32, hidden=192).cuda().eval()
    store.embed(model)
    masks = dict(main_masks(c.D, c.hw), time_mask_prob=1.0, feat_mask_prob=1.0, cutout_prob=0.0)
    pol = policy_of(ss, masks, aug=dict(AUG, shift_prob=0.0))
    kw = dict(augment=True, rng="philox", seed=SEED, first_row=3, policy=pol)
    idx = i32(IDX70)
    X, T, R, y = [t.clone() for t in store.batch(idx, **kw)]
    Z, Tz, none, yz = store.batch(idx, embedded=True, **kw)
    sync()
    assert none is None and torch.equal(T, Tz) and torch.equal(y, yz) and Z.shape == (70, MAX_T, c.D + 32)
    assert torch.equal(Z[:, :, :c.D], X)
    ref = ref_plan(c, IDX70, 3, SEED, masks, aug=dict(AUG, shift_prob=0.0))
    rmap = torch.from_numpy(ref["rmap"]).cuda().long()
    want = torch.where((rmap >= 0)[:, :, None], store.E[rmap.clamp(min=0)], store.E0[None, None, :].expand(70, MAX_T, 32))
    assert torch.equal(Z[:, :, c.D:], want)
    masked = 0
    for b, (t0, tw, col0, cw, *_r) in enumerate(ref["row_mask"].astype(np.int64)):
        if tw and ref["before"]["rmap"][b, 0] >= 0:
            assert all(torch.equal(Z[b, t, c.D:], store.E0) for t in range(t0, t0 + tw)) and not X[b, t0:t0 + tw].any()
            assert not R[b, t0:t0 + tw].any()
            masked += 1
        assert cw > 0 or T[b] == 0
        assert not Z[b, :, col0:col0 + cw].any()
    assert masked > 0
    with pytest.raises(ValueError, match="cutout_prob"):
        store.batch(idx, embedded=True, augment=True, rng="philox", policy=ss.AugmentPolicy(cutout_prob=0.5, cutout_max=(4, 4)))
    store.check()


def test_masks_off_issue_the_launches_of_the_policy_batch(L, clips):
    """A policy that leaves the masks off -- by default, by probability 0 or by maximum 0 -- gives the bits of today's policy batch
    through today's three launches; with a mask on the two new entry points appear, ss_batch_mask_apply only for band or cutout."""
    import silent_speech_amd as ss

    c = clips["84_64x64"]
    store = c.store
    idx = i32(IDX7)

    def traced(policy):
        L.PROFILE = {}
        try:
            out = [t.clone() for t in store.batch(idx, augment=True, rng="philox", seed=SEED, first_row=40, policy=policy)]
            sync()
            return out, list(L.PROFILE)
        finally:
            L.PROFILE = None

    three = ["ss_batch_plan_aug", "ss_batch_gather_f32_aug", "ss_batch_gather_u8_shift"]
    today, tags = traced(policy_of(ss, {}))
    assert tags == three
    full = full_masks(c.D, c.hw)
    for off in (dict(full, time_mask_prob=0.0, feat_mask_prob=0.0, cutout_prob=0.0),
                dict(full, time_mask_max=0, feat_mask_max=0, cutout_max=(0, 5)), dict(time_mask_streams="roi", time_mask_fill="hold", cutout_fill=7)):
        out, tags = traced(policy_of(ss, off))
        assert tags == three and all(torch.equal(u, v) for u, v in zip(out, today))
    _, tags = traced(None)
    assert tags == ["ss_batch_plan", "ss_batch_gather_f32", "ss_batch_gather_u8"]
    _, tags = traced(policy_of(ss, dict(time_mask_prob=1.0, time_mask_max=3)))
    assert tags == [three[0], "ss_batch_plan_mask"] + three[1:]
    for on in (dict(feat_mask_prob=1.0, feat_mask_max=3), dict(cutout_prob=1.0, cutout_max=(3, 3)), full):
        _, tags = traced(policy_of(ss, on))
        assert tags == [three[0], "ss_batch_plan_mask"] + three[1:] + ["ss_batch_mask_apply"]


# ------------------------------------------------------------------------------------------------ ss_batch_mask_apply alone
def test_apply_clamps_whatever_the_table_holds_and_refuses_bad_arguments(L):
    """A hand-made row_mask whose entries lie outside the row and the frame: nothing outside X and R is written (guard bytes on
    both sides of each, checked afterwards; inside either result is accepted).  A table inside the bounds, on views with an odd
    byte offset and a row pitch above D, gives exactly the restatement.  Then the SS_ERR_ARG cases of both entry points."""
    big = 2 ** 31 - 1
    D, ld, H, W, rpc = 10, 13, 6, 9, 2
    outside = [[0, 0, -5, 1000, -3, -7, 10000, 10000], [0, 0, D + 10, 5, W + 3, H + 2, 4, 4], [0, 0, big, big, big, big, big, big],
               [0, 0, -big - 1, big, -big - 1, -big - 1, big, big], [9, 9, D - 1, big, W - 1, H - 1, big, big], [0, 0, 3, -4, 2, 2, -1, 5]]
    inside = [[0, 0, 0, D, 0, 0, W, H], [0, 0, 3, 4, 1, 2, 7, 3], [0, 0, 0, 0, 8, 5, 1, 1], [0, 0, 9, 1, 0, 0, 0, 0], [0, 0, 0, 1, 2, 0, 5, 6],
              [0, 0, 5, 5, 0, 3, 9, 1]]
    clips_n = len(outside)
    rows, guard = clips_n * rpc, 64
    rmap_h = np.arange(rows, dtype=np.int32)
    rmap_h[3::4] = -1
    rng = np.random.default_rng(1)
    rm = i32(rmap_h)
    for table_h, exact in ((outside, False), (inside, True)):
        table = i32(table_h)
        xbuf = torch.full((guard + rows * ld + guard,), 7.0, device="cuda")
        rbuf = torch.full((guard + 3 + rows * H * W + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        X = xbuf[guard:guard + rows * ld].view(rows, ld)
        R = rbuf[guard + 3:guard + 3 + rows * H * W].view(rows, H, W)  # (3 bytes off any 4-byte address)
        X0 = rng.normal(size=(rows, ld)).astype(np.float32)
        R0 = rng.integers(1, 200, (rows, H, W), dtype=np.uint8)
        X.copy_(torch.from_numpy(X0))
        R.copy_(torch.from_numpy(R0))
        L.call("ss_batch_mask_apply", X.data_ptr(), ld, D, R.data_ptr(), H, W, rm.data_ptr(), table.data_ptr(), rows, rpc, 250, L.stream())
        sync()
        xb, rb = xbuf.cpu().numpy(), rbuf.cpu().numpy()
        assert np.all(xb[:guard] == 7.0) and np.all(xb[-guard:] == 7.0)
        assert np.all(rb[:guard + 3] == 0x5A) and np.all(rb[-guard:] == 0x5A)
        Xg, Rg = X.cpu().numpy(), R.cpu().numpy()
        assert np.array_equal(bits(Xg[:, D:]), bits(X0[:, D:]))                     # the columns behind D are never touched
        assert np.all((Xg == X0) | (Xg == 0)) and np.all((Rg == R0) | (Rg == 250))  # nothing but zeros and the fill is written
        assert np.array_equal(Rg[rmap_h < 0], R0[rmap_h < 0])
        if exact:
            Xe, Re = M.apply(X0.reshape(clips_n, rpc, ld), R0.reshape(clips_n, rpc, H, W), rmap_h.reshape(clips_n, rpc), table_h, 250)
            assert np.array_equal(bits(Xg), bits(Xe.reshape(rows, ld))) and np.array_equal(Rg, Re.reshape(rows, H, W))
            assert (Xg != X0).any() and (Rg != R0).any()
    # X alone and R alone
    table = i32(inside)
    X1 = torch.ones(rows, D, device="cuda")
    L.call("ss_batch_mask_apply", X1.data_ptr(), D, D, None, 0, 0, None, table.data_ptr(), rows, rpc, 0, L.stream())
    R1 = torch.ones(rows, H, W, dtype=torch.uint8, device="cuda")
    L.call("ss_batch_mask_apply", None, 0, 0, R1.data_ptr(), H, W, rm.data_ptr(), table.data_ptr(), rows, rpc, 9, L.stream())
    sync()
    Xe, Re = M.apply(np.ones((clips_n, rpc, D), np.float32), np.ones((clips_n, rpc, H, W), np.uint8), rmap_h.reshape(clips_n, rpc), inside, 9)
    assert np.array_equal(X1.cpu().numpy(), Xe.reshape(rows, D)) and np.array_equal(R1.cpu().numpy(), Re.reshape(rows, H, W))
    # refusals: nothing is written
    apply_ok = dict(X=X1.data_ptr(), ld=D, D=D, R=R1.data_ptr(), H=H, W=W, rmap=rm.data_ptr(), table=table.data_ptr(), rows=rows, rpc=rpc, fill=9)
    X1.fill_(1.0), R1.fill_(1)
    for bad in (dict(fill=256), dict(fill=-1), dict(rows=rows + 1), dict(rpc=0), dict(rows=0), dict(X=None, R=None), dict(ld=D - 1),
                dict(rmap=None), dict(table=None), dict(H=0), dict(D=0)):
        a = dict(apply_ok, **bad)
        with pytest.raises(RuntimeError, match="argument"):
            L.call("ss_batch_mask_apply", a["X"], a["ld"], a["D"], a["R"], a["H"], a["W"], a["rmap"], a["table"], a["rows"], a["rpc"],
                   a["fill"], L.stream())
    sync()
    assert torch.all(X1 == 1) and torch.all(R1 == 1)
    maps = torch.zeros(3, 4, MAX_T, dtype=torch.int32, device="cuda")
    lens = torch.full((4,), MAX_T, dtype=torch.int64, device="cuda")
    ok = dict(time_mask_prob=1.0, time_mask_max=4, feat_mask_prob=1.0, feat_mask_max=4, cutout_prob=1.0, cutout_max=(4, 4))
    before = maps.clone()
    for bad, kw in ((dict(time_mask_prob=1.5), {}), (dict(feat_mask_prob=-0.25), {}), (dict(cutout_prob=1.0001), {}),
                    (dict(time_mask_prob=float("nan")), {}), (dict(time_mask_max=-1), {}), (dict(feat_mask_max=-1), {}),
                    (dict(cutout_max=(-1, 4)), {}), (dict(cutout_max=(4, -2)), {}), ({}, dict(fill=256)), ({}, dict(fill=-1)),
                    ({}, dict(rmap=False))):
        with pytest.raises(RuntimeError, match="argument"):
            run_plan_mask(L, maps, lens, 10, (H, W), dict(ok, **bad), 0, SEED, **kw)
    table = torch.full((4, 8), -77, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="argument"):  # (on the live buffers: nothing written)
        L.call("ss_batch_plan_mask", maps[0].data_ptr(), maps[1].data_ptr(), None, lens.data_ptr(), 4, MAX_T, *mask_args(10, (H, W), ok),
               table.data_ptr(), L.stream())
    sync()
    assert torch.equal(maps, before) and torch.all(table == -77)
    # the cutout off: rmap may be NULL
    run_plan_mask(L, maps, lens, 10, (0, 0), dict(ok, cutout_prob=0.0), 0, SEED, rmap=False)


# ------------------------------------------------------------------------------------------------ fit
def test_fit_with_masks(L, tmp_path):
    """A short ``fit(plan="device", augment_policy=masks on)`` on the 45-clip, 3-word directory of test_fit_with_the_device_plan: it
    runs to the end with finite losses and writes a checkpoint the loader accepts.  (No accuracy threshold: what masking does to
    the accuracy on 45 synthetic clips is not a property of the code.)"""
    import silent_speech_amd as ss
    from silent_speech_amd import data as Dm
    from silent_speech_amd import harness as Hn

    rng = np.random.default_rng(0)
    clip_dir = tmp_path / "clips_npz"
    clip_dir.mkdir()
    words = ["aura", "no", "yes"]
    for k in range(45):
        T = int(rng.integers(14, 22))
        X = (0.05 * rng.normal(size=(T, 20))).astype(np.float32)
        X[:, (k % 3) * 4:(k % 3) * 4 + 4] += 0.5
        roi = rng.integers(0, 256, (T, 32, 32), dtype=np.uint8)
        Dm.save_clip(str(clip_dir / f"{k:03d}.npz"), X, np.arange(T), words[k % 3], "me", np.arange(4), roi)
    pol = ss.AugmentPolicy.lineage(time_mask_prob=0.5, time_mask_max=4, time_mask_fill="hold", feat_mask_prob=0.5, feat_mask_max=4,
                                   cutout_prob=0.5, cutout_max=(8, 8))
    out, hist, logs = str(tmp_path / "masked.pt"), [], []
    best = Hn.fit(str(clip_dir), out, epochs=2, batch_size=16, patience=3, max_t=24, lr=3e-3, log=logs.append, plan="device",
                  history=hist, augment_policy=pol)
    print("history", hist, "best", best)
    assert len(hist) == 2 and all(np.isfinite(h[k]) for h in hist for k in ("train_loss", "val_loss", "train_acc", "val_acc"))
    assert np.isfinite(best) and any("saved" in ln for ln in logs)
    model, id_to_label, max_t, use_roi = ss.load_classifier(out)
    assert max_t == 24 and use_roi and sorted(id_to_label.values()) == words
