"""GPU: the plan of an epoch and of a batch made on the device (ss_epoch_sample, ss_batch_plan, DeviceClipStore's
``rng="philox"`` mode, ``harness.fit(plan="device")``) against tests/batch_plan_ref.py -- integer outputs, compared exactly.

Run on the MI355X box with ``python -m pytest tests -m gpu``.
"""
import os
import re

import numpy as np
import pytest
import torch

import batch_plan_ref as P
from gpu_support import L, sync  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda")


def run_plan(L, indices, x_off, x_len, r_off, r_len, y, max_t, augment, first_row, seed, drop_max=2):
    """ss_batch_plan through the C ABI; ``indices`` a host array (uploaded) or a device int32 tensor."""
    idx = indices if isinstance(indices, torch.Tensor) else i32(indices)
    B = idx.numel()
    t = dict(x_off=i32(x_off), x_len=i32(x_len), y=torch.tensor(np.asarray(y), dtype=torch.int64, device="cuda"))
    has_roi = r_off is not None
    if has_roi:
        t["r_off"], t["r_len"] = i32(r_off), i32(r_len)
    # poisoned outputs: every element must be written
    maps = torch.full((3, B, max_t), -77, dtype=torch.int32, device="cuda")
    lens = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    y_out = torch.full((B,), -77, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.call("ss_batch_plan", idx.data_ptr(), B, t["x_off"].data_ptr(), t["x_len"].data_ptr(), L.ptr(t.get("r_off")),
           L.ptr(t.get("r_len")), t["y"].data_ptr(), len(x_len), max_t, int(augment), first_row, seed, 0.7, 0.35, drop_max,
           maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr() if has_roi else None, lens.data_ptr(), y_out.data_ptr(),
           err.data_ptr(), L.stream())
    sync()
    m = maps.cpu().numpy()
    return dict(xmap=m[0], nmap=m[1], rmap=m[2] if has_roi else None, lens=lens.cpu().numpy(), y_out=y_out.cpu().numpy(),
                bad=bool(err.item()))


def random_store(rng, n, roi):
    """Clips of 1..50 frames; with ``roi``: ROI tracks a few frames shorter / longer than the clip, every fifth clip none."""
    clips = []
    for k in range(n):
        T = int(rng.integers(1, 51))
        Tr = None
        if roi and k % 5 != 3:
            Tr = max(1, T + int(rng.integers(-3, 4)))
        clips.append((T, Tr))
    return clips


def assert_plan_equal(got, ref):
    for key in ("xmap", "nmap", "lens", "y_out"):
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key
    if ref["rmap"] is None:
        assert got["rmap"] is None
    else:
        assert np.array_equal(got["rmap"], ref["rmap"])
    assert got["bad"] == ref["bad"]


@pytest.mark.parametrize("B", [1, 16, 257])
@pytest.mark.parametrize("roi", [True, False])
def test_batch_plan_equals_the_restatement(L, B, roi):
    """Maps, lengths and labels, bit for bit: augmentation on / off, a store with ROI frames (some clips without, ROI tracks
    shorter and longer than the clip) and one without, clips longer than max_t, draw indices below, across and above 2^32."""
    rng = np.random.default_rng(100 + B)
    clips = random_store(rng, 40, roi)
    assert any(T > 24 for T, _ in clips) and (not roi or any(Tr is None for _, Tr in clips))
    x_off, x_len, r_off, r_len = P.store_tables(clips)
    y = rng.integers(0, 7, len(clips))
    tables = (x_off, x_len, r_off, r_len) if roi else (x_off, x_len, None, None)
    seen_drop = seen_noise = 0
    for max_t in (24, 90):  # 90: more than one pass of the wave over t
        for augment in (True, False):
            for first_row in (0, 2 ** 32 - 3, 2 ** 32 + 12345, 2 ** 63 + 11, 2 ** 64 - 2):
                idx = rng.integers(0, len(clips), B)
                ref = P.plan(idx, *tables, y, max_t, augment, first_row, SEED)
                assert_plan_equal(run_plan(L, idx, *tables, y, max_t, augment, first_row, SEED), ref)
                # a device tensor that is a slice of a longer one (as fit slices the epoch's order)
                longer = i32(np.concatenate([[0, 0, 0], idx, [0]]))
                assert_plan_equal(run_plan(L, longer[3:3 + B], *tables, y, max_t, augment, first_row, SEED), ref)
                seen_drop += int(ref["k"].sum())
                seen_noise += int(ref["noisy"].sum())
                if not augment:
                    assert not ref["k"].any() and not ref["noisy"].any()
    assert seen_noise > 0 and (B == 1 or seen_drop > 0)
    # one frame at most (DROP_FRAMES_MAX = 1) is the same kernel; three are refused
    idx = rng.integers(0, len(clips), B)
    ref = P.plan(idx, *tables, y, 24, True, 7, SEED, drop_max=1)
    assert ref["k"].max() <= 1
    assert_plan_equal(run_plan(L, idx, *tables, y, 24, True, 7, SEED, drop_max=1), ref)
    with pytest.raises(RuntimeError, match="unsupported"):
        run_plan(L, idx, *tables, y, 24, True, 7, SEED, drop_max=3)


def test_epoch_sample_equals_the_restatement(L):
    rng = np.random.default_rng(5)
    labels = rng.permutation(np.repeat([0, 2, 3, 5, 9], [50, 5, 1, 20, 124]))
    members, class_start = P.class_tables(labels)
    md, cd = i32(members), i32(class_start)
    for first, count in ((0, 20000), (2 ** 32 - 100, 300), (2 ** 63 + 5, 257), (0, 1)):
        out = torch.full((count,), -77, dtype=torch.int32, device="cuda")
        L.call("ss_epoch_sample", md.data_ptr(), len(members), cd.data_ptr(), len(class_start) - 1, first, count, SEED,
               out.data_ptr(), L.stream())
        sync()
        assert np.array_equal(out.cpu().numpy(), P.sample_epoch(members, class_start, first, count, SEED))
    # a rank's shard of the epoch is a slice of the whole draw
    whole, part = (torch.empty(n, dtype=torch.int32, device="cuda") for n in (1000, 400))
    L.call("ss_epoch_sample", md.data_ptr(), len(members), cd.data_ptr(), 5, 10, 1000, SEED, whole.data_ptr(), L.stream())
    L.call("ss_epoch_sample", md.data_ptr(), len(members), cd.data_ptr(), 5, 610, 400, SEED, part.data_ptr(), L.stream())
    sync()
    assert torch.equal(whole[600:], part)


def test_noise_stream_from_every_offset_equals_the_whole_gather(L):
    """C ABI only: ss_batch_gather_f32_at and ss_batch_gather_f32_aug on rows [r0, 12) of a 12-row gather, noise_first = r0 * D,
    against the rows of ss_batch_gather_f32 (Philox noise) over all 12 -- bit for bit, for every r0.  D = 7 makes noise_first & 3
    take all four values (the shard tests use D = 10: only even offsets), so a destination chunk takes its four normals from
    one Philox block or from two neighbouring ones at every split.  The scale of _aug is one rounded product on top."""
    D, rows, std, seed = 7, 12, 0.01, 0xF23456789ABCDEF1
    rng = np.random.default_rng(7)
    src = rng.normal(size=(9, D)).astype(np.float32)
    fmap = np.array([0, 3, -1, 8, 2, 2, 5, -1, 1, 7, 4, 6], np.int32)
    nmap = np.array([0, 0, 0, -1, 0, -1, 0, 0, 0, 0, -1, 0], np.int32)
    scale = (0.9 + 0.02 * np.arange(rows)).astype(np.float32)
    assert (fmap < 0).sum() == 2 and (nmap < 0).any() and [(r0 * D) & 3 for r0 in range(4)] == [0, 3, 2, 1]
    src_d, fmap_d, nmap_d = torch.from_numpy(src).cuda(), i32(fmap), i32(nmap)
    ones_d, scale_d = torch.ones(rows, device="cuda"), torch.from_numpy(scale).cuda()

    def bits(t):
        sync()
        return t.cpu().numpy().view(np.uint32)

    whole_d = torch.full((rows, D), 7.0, device="cuda")
    L.call("ss_batch_gather_f32", src_d.data_ptr(), D, fmap_d.data_ptr(), rows, None, nmap_d.data_ptr(), std, seed,
           whole_d.data_ptr(), L.stream())
    sync()
    whole = whole_d.cpu().numpy()
    noisy = (fmap >= 0) & (nmap >= 0)
    plain = np.where(fmap[:, None] >= 0, src[np.maximum(fmap, 0)], np.float32(0))
    assert all(np.array_equal(whole[r], plain[r]) != noisy[r] for r in range(rows))  # noise exactly where both maps say so
    for r0 in range(rows):
        n = rows - r0
        want = whole[r0:].view(np.uint32)
        head = (src_d.data_ptr(), D, fmap_d[r0:].data_ptr(), n, nmap_d[r0:].data_ptr(), std, seed, r0 * D)
        out = torch.full((n, D), 7.0, device="cuda")  # poisoned: every element must be written
        L.call("ss_batch_gather_f32_at", *head, out.data_ptr(), L.stream())
        assert np.array_equal(bits(out), want), r0
        out = torch.full((n, D), 7.0, device="cuda")
        L.call("ss_batch_gather_f32_aug", *head, ones_d.data_ptr(), 1, out.data_ptr(), L.stream())
        assert np.array_equal(bits(out), want), r0
        out = torch.full((n, D), 7.0, device="cuda")
        L.call("ss_batch_gather_f32_aug", *head, scale_d[r0:].data_ptr(), 1, out.data_ptr(), L.stream())
        assert np.array_equal(bits(out), np.float32(whole[r0:] * scale[r0:, None]).view(np.uint32)), r0


def golden_store(tmp_path):
    from test_host_formats import _golden_clips
    import silent_speech_amd as ss

    d, files = _golden_clips(str(tmp_path), GOLDEN)
    store = ss.DeviceClipStore(files, {"no": 0, "yes": 1}, max_t=int(d["max_t"]))
    n = int(d["n_clips"])
    Xs = np.concatenate([d[f"clip{k}::X"] for k in range(n)], 0)
    Rs = np.concatenate([d[f"clip{k}::roi"] for k in range(n) if f"clip{k}::roi" in d.files], 0)
    return d, store, Xs, Rs


def test_store_plain_batch_through_the_device_plan_equals_the_reference(L, tmp_path):
    """store.batch(range(n), augment=False, rng="philox") == the reference's own plain batch (tests/golden/dataset.npz), for
    host and device indices; sample_epoch == the restatement on the store's labels."""
    d, store, _, _ = golden_store(tmp_path)
    n = len(store)
    for idx in (range(n), list(range(n)), np.arange(n), torch.arange(n, dtype=torch.int32, device="cuda")):
        X, T, R, y = store.batch(idx, augment=False, rng="philox", seed=3, first_row=99)
        sync()
        assert np.array_equal(X.cpu().numpy(), d["plain::X"]) and np.array_equal(R.cpu().numpy(), d["plain::R"])
        assert np.array_equal(T.cpu().numpy(), d["plain::T"]) and np.array_equal(y.cpu().numpy(), d["plain::y"])
        assert T.dtype == torch.int64 and y.dtype == torch.int64 and X.dtype == torch.float32 and R.dtype == torch.uint8
    store.check()
    labels = store.y.cpu().numpy()
    members, class_start = P.class_tables(labels)
    for kw, ref_args in ((dict(), (0, n, 0)), (dict(num_samples=500, seed=SEED, first=2 ** 32 - 9), (2 ** 32 - 9, 500, SEED))):
        got = store.sample_epoch(**kw)
        assert got.dtype == torch.int32 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), P.sample_epoch(members, class_start, *ref_args))
    # the existing modes are untouched by the new one
    X, T, R, y = store.batch(range(n), augment=False)
    sync()
    assert np.array_equal(X.cpu().numpy(), d["plain::X"]) and np.array_equal(T.cpu().numpy(), d["plain::T"])


def test_store_augmented_batches_follow_the_plan(L, tmp_path):
    """Rows the plan leaves without noise are the plain gather through the reference maps, exactly; noisy rows differ from it
    by noise of standard deviation 0.01 (+- 0.002, the bound of the device-rng test); padding is exactly zero; a batch is a
    function of (seed, first_row); consecutive first_row values give other noise."""
    d, store, Xs, Rs = golden_store(tmp_path)
    n, max_t = len(store), store.max_t
    tables = (store.x_off, store.x_len, store.r_off, store.r_len)
    labels = store.y.cpu().numpy()
    order = store.sample_epoch(num_samples=16 * 12, seed=SEED)
    order_h = order.cpu().numpy()
    noise_std, n_plain_rows, n_dropped = [], 0, 0
    for step in range(12):
        lo = step * 16
        X, T, R, y = store.batch(order[lo:lo + 16], augment=True, rng="philox", seed=SEED, first_row=lo)
        sync()
        Xc, Tc, Rc, yc = X.cpu().numpy(), T.cpu().numpy(), R.cpu().numpy(), y.cpu().numpy()
        ref = P.plan(order_h[lo:lo + 16], *tables, labels, max_t, True, lo, SEED)
        assert np.array_equal(Tc, ref["lens"]) and np.array_equal(yc, ref["y_out"])
        assert np.array_equal(Rc, P.gather(Rs, ref["rmap"], Rs.shape[1:]))          # ROI frames: never dropped, never noised
        X0 = P.gather(Xs, ref["xmap"], Xs.shape[1:])
        for b in range(16):
            assert not Xc[b, Tc[b]:].any()                                            # padding exactly zero
            if ref["noisy"][b]:
                diff = Xc[b, :Tc[b]] - X0[b, :Tc[b]]
                if Tc[b]:
                    assert diff.any()
                    noise_std.append(diff.ravel())
            else:
                assert np.array_equal(Xc[b], X0[b])
                n_plain_rows += 1
        n_dropped += int(ref["k"].sum())
        # host indices: the same batch
        X2, T2, R2, y2 = store.batch(order_h[lo:lo + 16].tolist(), augment=True, rng="philox", seed=SEED, first_row=lo)
        sync()
        assert torch.equal(X2, X) and torch.equal(R2, R) and np.array_equal(T2.cpu().numpy(), Tc) and np.array_equal(y2.cpu().numpy(), yc)
    assert n_plain_rows > 0 and n_dropped > 0 and len(noise_std) > 50
    std = float(np.concatenate(noise_std).std())
    print(f"noise std over {len(noise_std)} noisy rows: {std:.5f}")
    assert abs(std - 0.01) < 0.002, std
    store.check()
    # consecutive first_row values on the same clips (clip 3: 9 frames, never dropped from): rows noisy in both differ
    idx = [3] * 16
    Xa = store.batch(idx, augment=True, rng="philox", seed=SEED, first_row=0)[0].cpu().numpy()
    Xb = store.batch(idx, augment=True, rng="philox", seed=SEED, first_row=1)[0].cpu().numpy()
    na = P.plan(idx, *tables, labels, max_t, True, 0, SEED)["noisy"]
    nb = P.plan(idx, *tables, labels, max_t, True, 1, SEED)["noisy"]
    both = np.flatnonzero(na & nb)
    assert len(both) > 0 and all(not np.array_equal(Xa[b], Xb[b]) for b in both)
    assert all(np.array_equal(Xa[b], d["plain::X"][3]) for b in np.flatnonzero(~na))
    # rows of one batch do not share noise either
    assert len(both) < 2 or not np.array_equal(Xa[both[0]], Xa[both[1]])


def test_out_of_range_indices_are_caught_not_dereferenced(L, tmp_path):
    d, store, _, _ = golden_store(tmp_path)
    n = len(store)
    for bad in ([0, n], [-1, 2], [2 ** 31 - 1]):
        with pytest.raises(IndexError):
            store.batch(bad, augment=True, rng="philox")
    store.check()  # nothing was launched, nothing is flagged
    idx = torch.tensor([0, n, -1, 1, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    X, T, R, y = store.batch(idx, augment=True, rng="philox", seed=1, first_row=0)
    sync()
    assert T.cpu().tolist()[1:3] == [0, 0] and int(T[4]) == 0 and int(T[0]) > 0 and int(T[3]) > 0
    for b in (1, 2, 4):
        assert not X[b].any() and not R[b].any() and int(y[b]) == 0
    assert y.cpu().tolist()[0] == int(d["plain::y"][0]) and int(y[3]) == int(d["plain::y"][1])
    with pytest.raises(IndexError, match="outside"):
        store.check()
    store.check()  # reading the flag clears it
    with pytest.raises(ValueError):
        store.batch(torch.zeros(4, dtype=torch.int64, device="cuda"), rng="philox")


def test_fit_with_the_device_plan(L, tmp_path):
    """fit(plan="device") on a small synthetic directory (as test_harness_fit_evaluate_checkpoint builds one): two epochs,
    the training loss falls, the checkpoint loads, and evaluate() gives the same numbers through either plan (validation is not
    augmented, so both assemble identical batches)."""
    import silent_speech_amd as ss
    from silent_speech_amd import data as Dm
    from silent_speech_amd import harness as Hn

    rng = np.random.default_rng(0)
    clip_dir = tmp_path / "clips_npz"
    clip_dir.mkdir()
    words = ["aura", "no", "yes"]
    for k in range(45):
        lab = words[k % 3]
        T = int(rng.integers(14, 22))
        X = (0.05 * rng.normal(size=(T, 20))).astype(np.float32)
        X[:, (k % 3) * 4:(k % 3) * 4 + 4] += 0.5
        roi = rng.integers(0, 256, (T, 32, 32), dtype=np.uint8)
        Dm.save_clip(str(clip_dir / f"{k:03d}.npz"), X, np.arange(T), lab, "me", np.arange(4), roi)
    out = str(tmp_path / "word_model_points_roi.pt")
    logs = []
    best = Hn.fit(str(clip_dir), out, epochs=2, batch_size=16, patience=3, max_t=24, lr=3e-3, log=logs.append, plan="device")
    epochs = [ln for ln in logs if ln.startswith("ep ")]
    assert len(epochs) == 2 and epochs[0].startswith("ep 01 | train loss"), logs
    tr = [float(re.search(r"train loss ([0-9.]+)", ln).group(1)) for ln in epochs]
    va = [(float(m.group(1)), float(m.group(2))) for m in (re.search(r"val loss ([0-9.]+) acc ([0-9.]+)", ln) for ln in epochs)]
    print("train loss per epoch", tr, "val (loss, acc)", va, "best", best)
    assert tr[1] < tr[0], tr
    assert any("saved" in ln for ln in logs)
    model, id_to_label, max_t, use_roi = ss.load_classifier(out)
    assert max_t == 24 and use_roi and sorted(id_to_label.values()) == words
    info = Hn.scan_clips(str(clip_dir))
    _, val_files = Hn.split_by_label(info["files"], info["labels"], seed=42)
    store = ss.DeviceClipStore(val_files, info["label_to_id"], max_t=24)
    dev_res = Hn.evaluate(model, store, batch_size=16, plan="device")
    host_res = Hn.evaluate(model, store, batch_size=16, plan="host")
    assert dev_res == host_res, (dev_res[:2], host_res[:2])
    # ... and they are what fit logged for the epoch whose parameters the checkpoint holds (the last one that improved)
    top, saved_ep = 0.0, None
    for i, (_, acc) in enumerate(va):
        if acc > top:
            top, saved_ep = acc, i
    assert abs(dev_res[1] - best) < 1e-9 and f"{dev_res[0]:.4f}" == f"{va[saved_ep][0]:.4f}"
    # other batch sizes (a last, shorter batch) walk the same clips
    assert Hn.evaluate(model, store, batch_size=4, plan="device")[1:] == host_res[1:]
    with pytest.raises(ValueError):
        Hn.fit(str(clip_dir), out, epochs=1, plan="gpu")
