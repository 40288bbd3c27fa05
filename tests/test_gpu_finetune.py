"""GPU: fine-tuning with the ROI CNN frozen -- ``ss_batch_gather_z``, ``DeviceClipStore.embed`` / ``batch(embedded=True)``,
``Trainer(freeze_cnn=True).step_embedded`` and ``harness.fit(init_from=, freeze_cnn=)``.

Bounds.  The gather against its siblings and against torch indexing, the embedded batch against the pixel batch (eval logits) and the
frozen parameter range: equal bits.  The frozen step against the full step of the same model on the same batch: the loss within 2e-5
and every non-CNN gradient within ``2e-4 * scale + 2e-3 * max|ref|`` (``scale = max(max|ref|, 1e-4)``), the two figures
tests/test_gpu_model.py holds the full step to against the oracle; ``grad_norm()`` within 1e-3 relative.  A resumed frozen ``fit``
against the uninterrupted one: ``LOSS_BOUND`` of tests/test_gpu_ema_resume.py (ten times the spread measured between two
uninterrupted runs).

Run on the MI355X box with ``python -m pytest tests -m gpu``.
"""
import numpy as np
import pytest
import torch

import launch_trace as LT
import weights as W
from gpu_support import L, ss, write_clips  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
MAX_T, HW, XD, NCLS = 16, (32, 32), 84, 5
LOSS_BOUND = 10 * 9.781275e-08  # tests/test_gpu_ema_resume.py
# (T, Tr): longer than max_t; two with T > 12 (frames get dropped); an ROI track three frames short; two clips without ROI frames;
# one frame; the rest ordinary
CLIPS = [(20, 20), (13, 13), (14, 14), (10, 7), (9, None), (5, None), (1, 1), (16, 16), (8, 8), (11, 11)]
SENTINEL = -12345.0


def write_store_clips(tmp):
    rng = np.random.default_rng(3)
    files = []
    for n, (T, Tr) in enumerate(CLIPS):
        arrays = dict(X=(0.3 * rng.normal(size=(T, XD))).astype(np.float32), ts=np.arange(T), label="w%d" % (n % NCLS), speaker="me",
                      idxs=np.arange(4))
        if Tr is not None:
            arrays["roi"] = rng.integers(0, 256, (Tr,) + HW, dtype=np.uint8)
        f = str(tmp / f"{n:02d}.npz")
        np.savez(f, **arrays)
        files.append(f)
    return files


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_store_clips(tmp_path_factory.mktemp("finetune_store"))


def new_store(ss, files):
    return ss.DeviceClipStore(files, {"w%d" % c: c for c in range(NCLS)}, max_t=MAX_T)


def new_model(ss, seed=11, **kw):
    m = ss.BiGRUClassifier(XD, NCLS, use_roi=True, hidden=192, **kw)
    m.load_state_dict(W.make_state_dict(seed, XD, NCLS, True))
    return m.cuda()


@pytest.fixture(scope="module")
def policy(ss):
    return ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=1.0)


@pytest.fixture(scope="module")
def world(ss, files, policy):
    """One store with its embeddings, the model they were made with, and ONE planned batch, pixel and embedded (shared, unchanged)."""
    model = new_model(ss).eval()
    store = new_store(ss, files)
    store.embed(model)
    idx = list(range(len(CLIPS)))
    kw = dict(augment=True, rng="philox", seed=SEED, first_row=40, policy=policy)
    X, T, R, y = store.batch(idx, **kw)
    X, T, R, y = X.clone(), T.clone(), R.clone(), y.clone()
    Z, Tz, none, yz = store.batch(idx, embedded=True, **kw)
    assert none is None and torch.equal(T, Tz) and torch.equal(y, yz)
    return dict(model=model, store=store, idx=idx, kw=kw, X=X, T=T, R=R, y=y, Z=Z.clone())


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def planned(ss, files):
    """Maps of ss_batch_plan_aug for 5 clips x 16 rows with all three policy draws on (the store's own plan buffers, cloned)."""
    store = new_store(ss, files)
    pol = ss.AugmentPolicy(time_warp_prob=1.0, scale_prob=1.0, roi_shift_prob=1.0, roi_shift_max=(3, 2))
    store.batch([0, 3, 4, 6, 2], augment=True, rng="philox", seed=SEED, first_row=9, policy=pol)
    xmap, nmap, rmap, lens, y, row_scale, row_shift = [b.clone() for b in store._plan_bufs[5]]
    torch.cuda.synchronize()
    assert (nmap >= 0).any() and (xmap < 0).any() and (rmap[2] < 0).all() and (xmap[2] >= 0).any()  # noise, padding, an ROI-less clip
    return dict(xmap=xmap, nmap=nmap, rmap=rmap, row_scale=row_scale, n_x=store.X.shape[0], n_r=store.R.shape[0])


def gather_z(L, feat, D, xmap, emb, E, rmap, fill, rows, nmap, std, seed, first, scale, rpc, dst, ld, status=False):
    args = (feat.data_ptr(), D, xmap.data_ptr(), L.ptr(emb), E, L.ptr(rmap), L.ptr(fill), rows, L.ptr(nmap), std, seed, first,
            L.ptr(scale), rpc, dst if isinstance(dst, int) else dst.data_ptr(), ld, L.stream())
    if status:
        return L.load().ss_batch_gather_z(*args)
    L.call("ss_batch_gather_z", *args)


GEOMETRIES = [(84, 32, 116), (83, 32, 115), (5, 20, 28), (84, 32, 120)]


@pytest.mark.parametrize("D,E,ld", GEOMETRIES)
@pytest.mark.parametrize("noise_first", [0, 4 * 83 + 3])
def test_gather_z_both_halves(L, planned, D, E, ld, noise_first):
    """Columns [0, D) against ss_batch_gather_f32_aug (and _at without a scale), bit for bit; columns [D, D + E) against torch indexing;
    the columns behind D + E untouched.  (84, 32, 116 / 120): 16 bytes per lane; 83 and (5, 20, 28): the element path."""
    assert noise_first == 0 or noise_first & 3
    g = torch.Generator().manual_seed(D * 1000 + E)
    feat = torch.randn(planned["n_x"], D, generator=g).cuda()
    emb = torch.randn(planned["n_r"], E, generator=g).cuda()
    fill = torch.randn(E, generator=g).cuda()
    xmap, nmap, rmap, sc = planned["xmap"], planned["nmap"], planned["rmap"], planned["row_scale"]
    rows, std = 5 * MAX_T, 0.01
    rm = rmap.reshape(-1).long()
    for scale in (sc, None):
        ref = torch.full((rows, D), SENTINEL, device="cuda")
        if scale is not None:
            L.call("ss_batch_gather_f32_aug", feat.data_ptr(), D, xmap.data_ptr(), rows, nmap.data_ptr(), std, SEED, noise_first,
                   scale.data_ptr(), MAX_T, ref.data_ptr(), L.stream())
        else:
            L.call("ss_batch_gather_f32_at", feat.data_ptr(), D, xmap.data_ptr(), rows, nmap.data_ptr(), std, SEED, noise_first,
                   ref.data_ptr(), L.stream())
        for use_rmap, use_fill in ((True, True), (True, False), (False, True), (False, False)):
            dst = torch.full((rows, ld), SENTINEL, device="cuda")
            gather_z(L, feat, D, xmap, emb, E, rmap if use_rmap else None, fill if use_fill else None, rows, nmap, std, SEED,
                     noise_first, scale, MAX_T, dst, ld)
            torch.cuda.synchronize()
            assert torch.equal(dst[:, :D], ref), (scale is not None, float((dst[:, :D] - ref).abs().max()))
            other = fill if use_fill else torch.zeros(E, device="cuda")
            want = torch.where((rm >= 0)[:, None], emb[rm.clamp(min=0)], other[None, :]) if use_rmap else other[None, :].expand(rows, E)
            assert torch.equal(dst[:, D:D + E], want)
            assert (dst[:, D + E:] == SENTINEL).all()
    # no noise map: the plain gather
    dst = torch.full((rows, ld), SENTINEL, device="cuda")
    gather_z(L, feat, D, xmap, emb, E, rmap, fill, rows, None, std, SEED, noise_first, None, 1, dst, ld)
    xm = xmap.reshape(-1).long()
    assert torch.equal(dst[:, :D], torch.where((xm >= 0)[:, None], feat[xm.clamp(min=0)], torch.zeros((), device="cuda")))


def test_gather_z_refuses_bad_arguments_and_writes_nothing(L, planned):
    D, E, ld, rows = 84, 32, 116, 5 * MAX_T
    feat = torch.randn(planned["n_x"], D).cuda()
    emb = torch.randn(planned["n_r"], E).cuda()
    xmap, nmap, rmap, sc = planned["xmap"], planned["nmap"], planned["rmap"], planned["row_scale"]
    dst = torch.full((rows, ld), SENTINEL, device="cuda")
    bad = [dict(D=0), dict(D=-4), dict(E=0), dict(ld=D + E - 1), dict(rpc=7), dict(rpc=0), dict(dst=dst.data_ptr() + 2),
           dict(feat_off=1), dict(emb_off=2)]
    for case in bad:
        f, e = feat, emb
        a = dict(D=D, E=E, ld=ld, rpc=MAX_T, dst=dst)
        a.update({k: v for k, v in case.items() if k in a})
        args = [f.data_ptr() + case.get("feat_off", 0), a["D"], xmap.data_ptr(), e.data_ptr() + case.get("emb_off", 0), a["E"],
                rmap.data_ptr(), None, rows, nmap.data_ptr(), 0.01, SEED, 0, sc.data_ptr(), a["rpc"],
                a["dst"] if isinstance(a["dst"], int) else a["dst"].data_ptr(), a["ld"], L.stream()]
        assert L.load().ss_batch_gather_z(*args) == -1, case
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()
    # rows % rows_per_clip matters only with a scale table
    gather_z(L, feat, D, xmap, emb, E, rmap, None, rows, nmap, 0.01, SEED, 0, None, 7, dst, ld)
    torch.cuda.synchronize()
    assert (dst != SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- the store
def test_embedded_batch_equals_the_pixel_batch(ss, world):
    """Z = X | CNN(R): the feature half is the pixel batch's X, bit for bit, and in eval mode forward_embedded(Z, T) are the logits of
    model(X, T, R).  The embedded batch issues the plan kernel and ONE gather.  A shard (batch_first_row) is rows of the batch."""
    model, store, X, T, R, Z = (world[k] for k in ("model", "store", "X", "T", "R", "Z"))
    assert Z.shape == (len(CLIPS), MAX_T, XD + 32) and Z.dtype == torch.float32
    assert torch.equal(Z[:, :, :XD], X)
    assert store.E.shape == (store.R.shape[0], 32) and store.E0.shape == (32,) and float(store.E0.abs().max()) > 0
    # a clip without ROI frames carries the embedding of a zero frame on its rows
    assert torch.equal(Z[4, :int(T[4]), XD:], store.E0.expand(int(T[4]), 32))
    with torch.no_grad():
        a, b = model(X, T, R), model.forward_embedded(Z, T)
    print("max |logit difference|:", float((a - b).abs().max()))
    assert torch.equal(a, b)
    mp = pytest.MonkeyPatch()
    log = LT.traced(mp, model, lambda: store.batch(world["idx"], embedded=True, **world["kw"]))
    assert [e[1] for e in LT.launches(log)] == ["ss_batch_plan_aug", "ss_batch_gather_z"]
    log = LT.traced(mp, model, lambda: store.batch(world["idx"], augment=True, rng="philox", seed=SEED, embedded=True))
    assert [e[1] for e in LT.launches(log)] == ["ss_batch_plan", "ss_batch_gather_z"]
    # rows [3, 10) of the batch, as a data-parallel rank gathers them
    kw = dict(world["kw"], first_row=world["kw"]["first_row"] + 3, batch_first_row=world["kw"]["first_row"])
    Zs, Ts, _, ys = store.batch(world["idx"][3:], embedded=True, **kw)
    assert torch.equal(Zs, Z[3:]) and torch.equal(Ts, T[3:]) and torch.equal(ys, world["y"][3:])
    # without augmentation and without a policy
    X0, T0, R0, _ = store.batch(world["idx"], augment=False, rng="philox")
    X0, T0 = X0.clone(), T0.clone()
    Z0, _, _, _ = store.batch(world["idx"], augment=False, rng="philox", embedded=True)
    with torch.no_grad():
        assert torch.equal(model(X0, T0, R0), model.forward_embedded(Z0, T0))
    Ze, Te, Re, ye = store.empty_batch(embedded=True)
    assert Ze.shape == (0, MAX_T, XD + 32) and Re is None and Te.shape == (0,) and ye.shape == (0,)
    store.check()


# ---------------------------------------------------------------------------------------------------------------- the step
def test_frozen_step_against_the_full_step(ss, world):
    X, T, R, y, Z = (world[k] for k in ("X", "T", "R", "y", "Z"))
    full, frozen = new_model(ss).train(), new_model(ss).train()
    tf, tz = ss.Trainer(full), ss.Trainer(frozen, freeze_cnn=True, ema_decay=0.9)
    n_cnn = frozen.cnn_param_range()
    assert 0 < n_cnn < frozen.flat_params.numel() and tz.n_frozen == n_cnn
    p0 = frozen.flat_params.clone()
    lf, cf = tf.step(X, T, R, y)
    lz, cz = tz.step_embedded(Z, T, y)
    print(f"loss: full {float(lf):.9f} frozen {float(lz):.9f} diff {abs(float(lf) - float(lz)):.3e}")
    assert abs(float(lf) - float(lz)) <= 2e-5
    Gf, Gz = full._views_of(full.flat_grads), frozen._views_of(frozen.flat_grads)
    for k in Gf:
        ref, got = Gf[k], Gz[k]
        if k.startswith("roi_cnn."):
            assert float(ref.abs().max()) > 0 and not got.any()  # no CNN gradient is written
            continue
        if k == "pool.score.bias":
            # as tests/test_gpu_model.py treats it: softmax is shift-invariant, the true gradient is exactly 0 and both sides hold
            # rounding noise of the sum over the attention weights (~1e-8)
            assert float(got.abs().max()) < 1e-6 and float(ref.abs().max()) < 1e-6
            continue
        scale = max(float(ref.abs().max()), 1e-4)
        err = float((got - ref).abs().max())
        print(f"{k}: max err {err:.3e}, bound {2e-4 * scale + 2e-3 * float(ref.abs().max()):.3e}")
        assert err <= 2e-4 * scale + 2e-3 * float(ref.abs().max()), k
    want = float(full.flat_grads[n_cnn:].double().pow(2).sum().sqrt())
    print(f"grad_norm: {float(tz.grad_norm()):.9f}, norm of the full step's non-CNN gradients {want:.9f}")
    assert abs(float(tz.grad_norm()) - want) <= 1e-3 * want
    assert float(tf.grad_norm()) > want  # (the full step's norm holds the CNN's share as well)
    tz.step_embedded(Z, T, y)
    tz.step_embedded(Z, T, y)
    assert torch.equal(frozen.flat_params[:n_cnn], p0[:n_cnn]) and torch.equal(tz.ema[:n_cnn], p0[:n_cnn])
    assert not torch.equal(frozen.flat_params[n_cnn:], p0[n_cnn:]) and not torch.equal(tz.ema[n_cnn:], p0[n_cnn:])
    assert not torch.equal(tz.ema[n_cnn:], frozen.flat_params[n_cnn:])
    raw, avg = frozen.flat_params.clone(), tz.ema.clone()
    with tz.ema_weights():
        assert torch.equal(frozen.flat_params[:n_cnn], p0[:n_cnn])
        assert torch.equal(frozen.flat_params[n_cnn:], avg[n_cnn:]) and torch.equal(tz.ema[n_cnn:], raw[n_cnn:])
    assert torch.equal(frozen.flat_params, raw) and torch.equal(tz.ema, avg)
    # an empty shard is a legal step, class weights work, the state round-trips
    store = world["store"]
    tz.step_embedded(*[store.empty_batch(embedded=True)[k] for k in (0, 1, 3)], global_batch=4)
    assert torch.equal(frozen.flat_params[:n_cnn], p0[:n_cnn])
    state = tz.state_dict()
    assert state["freeze_cnn"] is True and "freeze_cnn" not in tf.state_dict()
    other = ss.Trainer(new_model(ss).train(), freeze_cnn=True, ema_decay=0.9)
    other.load_state_dict(state)
    assert other.step_count == tz.step_count == 4
    with pytest.raises(ValueError, match="freeze_cnn"):
        ss.Trainer(new_model(ss), ema_decay=0.9).load_state_dict(state)
    with pytest.raises(ValueError, match="freeze_cnn"):
        other.load_state_dict(ss.Trainer(new_model(ss), ema_decay=0.9).state_dict())
    tw = ss.Trainer(new_model(ss).train(), freeze_cnn=True, class_weights=[1.0, 2.0, 0.5, 1.0, 3.0])
    lw, _ = tw.step_embedded(Z, T, y)
    assert np.isfinite(float(lw)) and abs(float(lw) - float(lz)) > 1e-4


def test_frozen_step_launches_no_cnn_kernel(ss, world):
    X, T, R, y, Z = (world[k] for k in ("X", "T", "R", "y", "Z"))
    mp = pytest.MonkeyPatch()
    full, frozen = new_model(ss).train(), new_model(ss).train()
    tf, tz = ss.Trainer(full), ss.Trainer(frozen, freeze_cnn=True)
    tf.step(X, T, R, y)
    tz.step_embedded(Z, T, y)
    a = LT.launches(LT.traced(mp, full, lambda: tf.step(X, T, R, y)))
    b = LT.launches(LT.traced(mp, frozen, lambda: tz.step_embedded(Z, T, y)))
    assert any(e[1].startswith("ss_roi_cnn") for e in a)
    assert not any(e[1].startswith("ss_roi_cnn") or e[1] == "ss_roi_active_frames" for e in b), [e[1] for e in b]
    dx = lambda log: sum(e[2] == "gemm_gru_dX" for e in log)  # noqa: E731
    assert dx(b) == dx(a) - 1 and dx(b) == 1
    ws = frozen._workspace_embedded(Z, train=True)
    assert ws.Z is None and ws.dZ is None and ws.frames is None and not hasattr(ws, "st_a1")
    # the optimiser's launches cover [n_cnn, n)
    n, n_cnn = frozen.flat_params.numel(), frozen.cnn_param_range()
    assert [e[4][4] for e in b if e[1] == "ss_adam_clip"] == [n - n_cnn] and [e[4][1] for e in b if e[1] == "ss_sumsq_f32"] == [n - n_cnn]
    assert [e[4][4] for e in a if e[1] == "ss_adam_clip"] == [n]


def test_guards(ss, world, files):
    X, T, R, y, Z = (world[k] for k in ("X", "T", "R", "y", "Z"))
    frozen, normal = ss.Trainer(new_model(ss).train(), freeze_cnn=True), ss.Trainer(new_model(ss).train())
    with pytest.raises(RuntimeError, match="step_embedded"):
        frozen.step(X, T, R, y)
    with pytest.raises(RuntimeError, match="freeze_cnn"):
        normal.step_embedded(Z, T, y)
    assert frozen.step_count == 0 and normal.step_count == 0
    fresh = new_store(ss, files)
    with pytest.raises(RuntimeError, match="embed"):
        fresh.batch([0, 1], rng="philox", embedded=True)
    with pytest.raises(RuntimeError, match="embed"):
        fresh.empty_batch(embedded=True)
    store = world["store"]
    with pytest.raises(ValueError, match="roi_shift"):
        store.batch([0, 1], augment=True, rng="philox", embedded=True,
                    policy=ss.AugmentPolicy(roi_shift_prob=0.5, roi_shift_max=(2, 2)))
    with pytest.raises(ValueError, match="philox"):
        store.batch([0, 1], embedded=True)
    bf16 = ss.BiGRUClassifier(XD, NCLS, use_roi=True, roi_emb=64, hidden=128, precision="bf16", cnn_channels=(16, 32, 64, 96)).cuda()
    with pytest.raises(RuntimeError, match="f32"):
        ss.Trainer(bf16, freeze_cnn=True)
    with pytest.raises(RuntimeError, match="f32"):
        fresh.embed(bf16)
    with pytest.raises(RuntimeError, match="f32"):
        ss.Trainer(ss.BiGRUClassifier(XD, NCLS).cuda(), freeze_cnn=True)  # no ROI branch to freeze
    with pytest.raises(ValueError, match="micro_batches"):
        ss.Trainer(new_model(ss), freeze_cnn=True, micro_batches=2)
    no_roi = ss.DeviceClipStore(files, {"w%d" % c: c for c in range(NCLS)}, max_t=MAX_T, use_roi=False)
    with pytest.raises(RuntimeError, match="no ROI frames"):
        no_roi.embed(new_model(ss))


def test_stale_embeddings_are_reported(ss, files):
    model, store = new_model(ss), new_store(ss, files)
    store.embed(model)
    store.check()
    with torch.no_grad():
        getattr(model.roi_cnn.net, "3").weight[2, 1, 0, 0] += 0.25
    with pytest.raises(RuntimeError, match="stale"):
        store.check()
    store.embed(model)
    store.check()
    with torch.no_grad():
        model.gru.weight_hh_l0[0, 0] += 0.25  # (not the CNN's business)
    store.check()


# ---------------------------------------------------------------------------------------------------------------- fit
def write_words(clip_dir, words, n, D=XD, seed=0):
    """The shared recipe at 9 to 14 frames a clip."""
    return write_clips(clip_dir, words, n, D=D, roi=HW, frames=(9, 15), seed=seed)


FIT = dict(batch_size=16, patience=5, max_t=MAX_T, lr=3e-3, plan="device", log=lambda *a, **k: None)


@pytest.fixture(scope="module")
def fits(ss, tmp_path_factory):
    """Checkpoint A from scratch on three words; then, on four other words, from A with the CNN frozen: two epochs uninterrupted, and
    one epoch resumed to two.  Each ``fit`` once."""
    from silent_speech_amd import harness as Hn

    d = tmp_path_factory.mktemp("finetune_fit")
    dir_a = write_words(str(d / "clips_a"), ["aura", "no", "yes"], 36, seed=0)
    dir_b = write_words(str(d / "clips_b"), ["down", "left", "right", "up"], 40, seed=1)
    A = str(d / "a.pt")
    Hn.fit(dir_a, A, epochs=2, **FIT)
    logs, hu, h1, h2 = [], [], [], []
    kw = dict(FIT, init_from=A, freeze_cnn=True, ema_decay=0.9, log=logs.append)
    Hn.fit(dir_b, str(d / "u.pt"), epochs=2, state_path=str(d / "u_state.pt"), history=hu, **kw)
    Hn.fit(dir_b, str(d / "r.pt"), epochs=1, state_path=str(d / "r_state.pt"), history=h1, **kw)
    Hn.fit(dir_b, str(d / "r.pt"), epochs=2, state_path=str(d / "r_state.pt"), resume=True, history=h2, **kw)
    return dict(dir=d, dir_a=dir_a, dir_b=dir_b, A=A, hu=hu, h1=h1, h2=h2, logs=logs)


def test_fit_from_a_checkpoint_with_the_cnn_frozen(ss, fits):
    from silent_speech_amd import checkpoint as Ck

    a = torch.load(fits["A"], map_location="cpu", weights_only=False)
    u = torch.load(str(fits["dir"] / "u.pt"), map_location="cpu", weights_only=False)
    model, id_to_label, max_t, use_roi = ss.load_classifier(str(fits["dir"] / "u.pt"))
    assert use_roi and max_t == MAX_T and sorted(id_to_label.values()) == ["down", "left", "right", "up"]
    assert list(u["model"]) == list(a["model"])
    for k in a["model"]:
        if k.startswith("roi_cnn."):
            assert torch.equal(u["model"][k], a["model"][k]), k
        elif k.startswith("gru."):
            assert not torch.equal(u["model"][k], a["model"][k]), k
    assert u["model"]["head.4.weight"].shape == (4, 128) and a["model"]["head.4.weight"].shape == (3, 128)
    assert any("fresh initialisation" in str(line) for line in fits["logs"])
    state = Ck.load_train_state(str(fits["dir"] / "u_state.pt"))
    assert state["fingerprint"]["freeze_cnn"] is True and len(state["fingerprint"]["init_from"]) == 64
    assert state["trainer"]["freeze_cnn"] is True
    # interrupted after epoch 1 and resumed: the uninterrupted run
    hu, h1, h2 = fits["hu"], fits["h1"], fits["h2"]
    assert [h["epoch"] for h in hu] == [1, 2] and [h["epoch"] for h in h1] == [1] and [h["epoch"] for h in h2] == [2]
    for p, q in zip(hu, h1 + h2):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {p['epoch']} {key}: uninterrupted {p[key]:.9f} resumed {q[key]:.9f} diff {abs(p[key] - q[key]):.3e}")
    for p, q in zip(hu, h1 + h2):
        assert abs(p["train_loss"] - q["train_loss"]) <= LOSS_BOUND and abs(p["val_loss"] - q["val_loss"]) <= LOSS_BOUND, (p, q)


def test_fit_refuses_a_checkpoint_of_another_shape(ss, fits, tmp_path):
    from silent_speech_amd import harness as Hn

    narrow = write_words(str(tmp_path / "clips_d20"), ["aura", "no", "yes"], 9, D=20)
    with pytest.raises(ValueError, match="x_dim"):
        Hn.fit(narrow, str(tmp_path / "x.pt"), epochs=1, init_from=fits["A"], **FIT)
    # a resumed run must have started from the same file
    other = str(tmp_path / "other.pt")
    ck = torch.load(fits["A"], map_location="cpu", weights_only=False)
    ck["seed"] = 43
    torch.save(ck, other)
    with pytest.raises(ValueError, match="init_from"):
        Hn.fit(fits["dir_b"], str(tmp_path / "y.pt"), epochs=2, state_path=str(fits["dir"] / "r_state.pt"), resume=True,
               init_from=other, freeze_cnn=True, ema_decay=0.9, **FIT)
