"""GPU: the data-parallel ``harness.fit`` as far as one GPU can show it -- ``evaluate_device`` against ``evaluate``, rank shards
that rebuild the single-process batch bit for bit, ``Trainer.step`` on an empty shard, and the whole ``fit`` over a one-rank
RCCL group in a fresh child process against the single-process ``fit``.  More than one rank has not run anywhere."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_support import WORDS, ss, write_clips  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = dict(epochs=3, batch_size=16, patience=3, max_t=24, lr=3e-3, plan="device")
# Bound on the per-epoch losses of the one-rank RCCL run against the single-process run: measured, not chosen.  Two
# single-process ``fit(plan="device")`` runs of this configuration (fresh processes, MI355X, the commit before this feature)
# differed per epoch by 9.78e-08, 0, 1.22e-08 (train loss) and 1.99e-08, 1.99e-08, 0 (validation loss); the bound is ten times
# the largest of these.
SPREAD = 9.781275e-08
LOSS_BOUND = 10 * SPREAD


@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    return write_clips(str(tmp_path_factory.mktemp("dp") / "clips_npz"), WORDS)


@pytest.fixture(scope="module")
def single(ss, clip_dir, tmp_path_factory):
    """The single-process ``fit(plan="device")``, run once: its checkpoint, log and unrounded history."""
    from silent_speech_amd import harness as Hn

    out = str(tmp_path_factory.mktemp("single") / "word_model.pt")
    logs, history = [], []
    best = Hn.fit(clip_dir, out, log=logs.append, history=history, **FIT)
    return dict(best=best, logs=logs, history=history, ckpt=out)


@pytest.fixture(scope="module")
def whole_store(ss, clip_dir):
    from silent_speech_amd import harness as Hn

    info = Hn.scan_clips(clip_dir)
    return info, ss.DeviceClipStore(info["files"], info["label_to_id"], max_t=24)


def models(ss, single, info):
    """A trained model (few errors) and an untrained one (many): both kinds of confusion list."""
    trained = ss.load_classifier(single["ckpt"])[0]
    torch.manual_seed(3)
    fresh = ss.BiGRUClassifier(info["x_dim"], 3, use_roi=True, roi_emb=32, hidden=192).cuda()
    return {"trained": trained.cuda(), "fresh": fresh}


def test_evaluate_device_equals_evaluate(ss, single, whole_store):
    from silent_speech_amd import harness as Hn

    info, store = whole_store
    names = info["id_to_label"]
    n_err = 0
    for name, model in models(ss, single, info).items():
        loss, acc, y_true, y_pred = Hn.evaluate(model, store, batch_size=4)
        res = Hn.evaluate_device(model, store, batch_size=4)
        assert isinstance(res, Hn.EvalResult) and res.n == len(store) == 45
        assert res.acc == acc and abs(res.loss - loss) < 1e-4, (name, res.loss, loss)
        assert res.y_true.dtype == torch.int32 and res.y_true.is_cuda
        assert res.y_true.cpu().tolist() == y_true and res.y_pred.cpu().tolist() == y_pred
        assert res.confusion.sum() == 45 and int(np.trace(res.confusion)) == round(acc * 45)
        for k in (1, 6, 50):
            assert Hn.top_confusions_from_matrix(res.confusion, res.first_seen, names, k) == Hn.top_confusions(y_true, y_pred, names, k)
        n_err += 45 - int(np.trace(res.confusion))
        # three ranks without a group, reduced on the host: sums, and first_seen by minimum
        parts = [Hn.evaluate_device(model, store, batch_size=4, rank=r, world_size=3) for r in range(3)]
        assert [p.n for p in parts] == [15, 15, 15]
        assert sum((p.y_true.cpu().tolist() for p in parts), []) == y_true
        assert sum((p.y_pred.cpu().tolist() for p in parts), []) == y_pred
        assert np.array_equal(sum(p.confusion for p in parts), res.confusion)
        assert np.array_equal(np.minimum.reduce([p.first_seen for p in parts]), res.first_seen)
        assert sum(round(p.acc * p.n) for p in parts) == round(res.acc * res.n)
        # float32 sums of the same 45 losses in another order: the whole is within 44 u S of the exact sum S, the three parts
        # within 14 u S together (u = 2^-24), and the stored sums round once more -- 64 u S covers it, S / 45 = the mean loss
        assert abs(sum(p.loss * p.n for p in parts) / 45 - res.loss) <= 64 * 2.0 ** -24 * max(1.0, res.loss)
        # an uneven world: 45 clips over 4 ranks = 12, 12, 12, 9
        assert [Hn.evaluate_device(model, store, batch_size=16, rank=r, world_size=4).n for r in range(4)] == [12, 12, 12, 9]
    assert n_err > 0  # the confusion lists compared above were not all empty
    store.check()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape", ["roi_d20", "plain_d5"])
def test_rank_shards_rebuild_the_single_process_batch(ss, whole_store, tmp_path, world, shape):
    """An epoch with a partial last batch (45 draws, global batch 16): the rank batches drawn through ``epoch_shards``, concatenated
    in rank order, are the single-process ``store.batch`` of that global batch bit for bit -- X, T, R, y, augmentation on.
    ``plain_d5``: 7 x 5 floats per clip, so most shards begin inside a 4-element block of the noise stream."""
    from silent_speech_amd import harness as Hn

    if shape == "roi_d20":
        _, store = whole_store
    else:
        info = Hn.scan_clips(write_clips(str(tmp_path / "plain"), WORDS, D=5, roi=None))
        store = ss.DeviceClipStore(info["files"], info["label_to_id"], max_t=7)
    seed, base, batch = 5, 45, 16  # (the second epoch of a run: draws 45 ...)
    order = store.sample_epoch(seed=seed, first=base)
    keep = lambda b: tuple(None if t is None else t.clone() for t in b)  # noqa: E731  (T and y are buffers the store reuses)
    per_rank = [list(Hn.epoch_shards(len(order), batch, r, world)) for r in range(world)]
    noisy = 0
    for k, g in enumerate(range(0, len(order), batch)):
        g_end = min(len(order), g + batch)
        whole = keep(store.batch(order[g:g_end], augment=True, rng="philox", seed=seed, first_row=base + g))
        plain = keep(store.batch(order[g:g_end], augment=False, rng="philox"))
        noisy += int(not torch.equal(whole[0], plain[0]))
        parts = []
        for r in range(world):
            lo, hi, first_row, global_batch = per_rank[r][k]
            assert global_batch == g_end - g and hi > lo
            parts.append(keep(store.batch(order[lo:hi], augment=True, rng="philox", seed=seed, first_row=base + first_row,
                                          batch_first_row=base + g)))
        for j, what in enumerate("XTRy"):
            if whole[j] is None:
                assert all(p[j] is None for p in parts)
                continue
            assert torch.equal(torch.cat([p[j] for p in parts]), whole[j]), (what, k)
    assert noisy == 3  # the comparison was of augmented batches
    store.check()


def test_trainer_step_on_an_empty_shard(ss, whole_store):
    """(0, T, D) inputs on a fresh trainer: a zero gradient with zero moments is a zero update, so every parameter keeps its
    bits; zero loss, zero hits, the step counts; a normal step afterwards runs."""
    info, store = whole_store
    torch.manual_seed(0)
    model = ss.BiGRUClassifier(info["x_dim"], 3, use_roi=True, roi_emb=32, hidden=192).cuda().train()
    trainer = ss.Trainer(model, lr=3e-3)
    before = model.flat_params.clone()
    X, T, R, y = store.empty_batch()
    assert X.shape == (0, 24, 20) and R.shape == (0, 24, 32, 32) and T.numel() == 0 and y.numel() == 0
    loss, correct = trainer.step(X, T, R, y, global_batch=5)
    assert float(loss) == 0.0 and int(correct) == 0 and trainer.step_count == 1
    assert torch.equal(model.flat_params, before)
    assert float(trainer.grad_norm()) == 0.0 and not bool(trainer.m.any()) and not bool(trainer.v.any())
    X, T, R, y = store.batch(range(16), augment=False, rng="philox")
    loss, correct = trainer.step(X, T, R, y)
    assert trainer.step_count == 2 and float(loss) > 0 and 0 <= int(correct) <= 16
    assert bool(torch.isfinite(model.flat_params).all()) and not torch.equal(model.flat_params, before)


def test_one_rank_rccl_fit_equals_single_process(ss, single, clip_dir, tmp_path):
    """The data-parallel ``fit`` on the hardware at hand: a FRESH child (torch.distributed.run, one rank) joins an "nccl" (= RCCL)
    group and runs ``fit(plan="device", process_group=...)`` for 3 epochs -- broadcast, the gradient all-reduce of every step, the
    two metric collectives per epoch, the barrier.  Against the single-process ``fit(plan="device")``: sums over one rank are the
    identity, so the two runs differ only by the order of the float atomics.

    The bound on the per-epoch losses is measured, not chosen (``LOSS_BOUND`` above): the single-process ``fit(plan="device")``
    was run twice on the GPU at the commit before this feature, each in a fresh process.  Measured spread: the largest per-epoch
    difference between the two runs was 9.78e-08 (train loss of epoch 1: 0.841275240 against 0.841275337; the other five
    differences were between 0 and 1.99e-08).  Bound: ten times that, 9.78e-07 (atomic-order noise through Adam has a long
    tail).  The differences of this run are printed before they are compared."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out, ckpt = str(tmp_path / "child.pt"), str(tmp_path / "child_model.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "_fit_child.py"), clip_dir, ckpt, out,
                        str(FIT["epochs"])], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = torch.load(out, map_location="cpu", weights_only=False)
    assert got["backend"] == "nccl" and got["world"] == 1
    epoch_lines = lambda logs: [ln for ln in logs if ln.startswith("ep ")]  # noqa: E731
    assert len(epoch_lines(got["logs"])) == len(epoch_lines(single["logs"])) == len(got["history"]) == len(single["history"]) == 3
    model, id_to_label, max_t, use_roi = ss.load_classifier(ckpt)
    assert max_t == 24 and use_roi and sorted(id_to_label.values()) == WORDS
    assert got["best"] >= 0.8 and single["best"] >= 0.8, (got["best"], single["best"], got["logs"])
    for a, b in zip(got["history"], single["history"]):
        for key in ("train_loss", "val_loss"):
            print(f"epoch {a['epoch']} {key}: child {a[key]:.9f} single {b[key]:.9f} diff {abs(a[key] - b[key]):.3e}")
    for a, b in zip(got["history"], single["history"]):
        assert abs(a["train_loss"] - b["train_loss"]) <= LOSS_BOUND and abs(a["val_loss"] - b["val_loss"]) <= LOSS_BOUND, (a, b)
