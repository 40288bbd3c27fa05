"""CPU: the host side of the weight average and of resumable ``fit`` runs -- the two new entry points in the header, the
library and the ctypes table; the atomic train-state writer; the fingerprint comparison; the warm-up schedule; the NumPy
restatement of the optimiser step against ``torch.optim.Adam``; argument checks that fire before any device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ss_adam_clip_ema", "ss_swap_f32")


def declared_arguments(name):
    """Number of arguments of ``name`` as include/ss_hotpath.h declares it (None: not declared)."""
    txt = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    return None if m is None else len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_ctypes_table_agree_on_the_new_entry_points():
    from silent_speech_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from silent_speech_amd.build import build

        build(verbose=False)
    lib = _lib.load()
    assert declared_arguments("ss_adam_clip") == 14  # (the parser, on an entry point that was there before)
    for name, n_args in zip(NEW_ENTRY_POINTS, (16, 4)):
        assert declared_arguments(name) == n_args, f"{name} is not declared with {n_args} arguments"
        assert hasattr(lib, name), f"{name} declared in include/ss_hotpath.h but not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n_args
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    # ss_adam_clip_ema = ss_adam_clip + the ema pointer behind v + the decay in front of the stream
    a, e = _lib.SIGNATURES["ss_adam_clip"], _lib.SIGNATURES["ss_adam_clip_ema"]
    assert e == a[:4] + [_lib._vp] + a[4:-1] + [_lib._f] + a[-1:]


def example_state():
    g = torch.Generator().manual_seed(0)
    return dict(format=1, model={"head.4.bias": torch.randn(5, generator=g)},
                trainer=dict(m=torch.randn(8, generator=g), v=torch.rand(8, generator=g), ema=None, step_count=9, ema_decay=None,
                             ema_warmup=True, betas=(0.9, 0.999), eps=1e-8, lr=3e-3, max_norm=1.0, numel=8),
                epoch=3, best=0.875, bad=1, stopped=False,
                fingerprint=dict(seed=42, labels=["aura", "no"], class_weights=None, augment_policy=dict(scale_range=[0.9, 1.1])))


def test_train_state_round_trip_loads_with_weights_only(tmp_path):
    from silent_speech_amd import checkpoint as Ck

    path = str(tmp_path / "state.pt")
    state = example_state()
    Ck.save_train_state(path, state)
    assert os.listdir(tmp_path) == ["state.pt"]  # no temporary file left behind
    raw = torch.load(path, map_location="cpu", weights_only=True)  # (what load_train_state does; here without its help)
    got = Ck.load_train_state(path)
    for s in (raw, got):
        assert s["epoch"] == 3 and s["best"] == 0.875 and s["bad"] == 1 and s["stopped"] is False
        assert s["trainer"]["ema"] is None and s["trainer"]["betas"] == [0.9, 0.999] and s["trainer"]["step_count"] == 9
        assert torch.equal(s["trainer"]["m"], state["trainer"]["m"]) and torch.equal(s["model"]["head.4.bias"], state["model"]["head.4.bias"])
        assert s["fingerprint"] == state["fingerprint"]
    torch.save({"format": 99}, path)
    with pytest.raises(ValueError, match="train-state"):
        Ck.load_train_state(path)


def test_train_state_writer_is_atomic(tmp_path, monkeypatch):
    """A writer that dies after half of its bytes leaves the previous file as it was, and no temporary file."""
    from silent_speech_amd import checkpoint as Ck

    path = str(tmp_path / "state.pt")
    Ck.save_train_state(path, example_state())
    before = open(path, "rb").read()

    def dies_midway(obj, f, *a, **k):
        f.write(before[:len(before) // 2])
        f.flush()
        raise OSError("disk full")

    monkeypatch.setattr(Ck.torch, "save", dies_midway)
    newer = example_state()
    newer["epoch"] = 4
    with pytest.raises(OSError, match="disk full"):
        Ck.save_train_state(path, newer)
    monkeypatch.undo()
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["state.pt"]
    assert Ck.load_train_state(path)["epoch"] == 3
    Ck.save_train_state(path, newer)  # and an undisturbed writer replaces it
    assert Ck.load_train_state(path)["epoch"] == 4 and os.listdir(tmp_path) == ["state.pt"]


def test_fingerprint_difference_names_the_first_differing_field():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    base = dict(seed=42, batch_size=16, world_size=1, max_t=24, lr=3e-3, labels=["aura", "no", "yes"], x_dim=20, use_roi=True,
                n_train=38, n_val=7, class_weights=None, augment_policy=None, ema_decay=None)
    fp = Hn.run_fingerprint(**base)
    assert list(fp) == list(Ck.FINGERPRINT_FIELDS)
    assert Ck.fingerprint_difference(fp, Hn.run_fingerprint(**base)) is None
    changes = dict(seed=7, batch_size=8, world_size=2, max_t=90, lr=3e-4, labels=["aura", "no"], x_dim=84, use_roi=False, n_train=37,
                   n_val=8, class_weights=[1.0, 2.0, 0.5], augment_policy=ss.AugmentPolicy(scale_prob=0.3), ema_decay=0.9)
    assert set(changes) == set(Ck.FINGERPRINT_FIELDS)
    for name, value in changes.items():
        assert Ck.fingerprint_difference(fp, Hn.run_fingerprint(**dict(base, **{name: value}))) == name
    # several differences: the first in FINGERPRINT_FIELDS order; a field one side lacks differs
    assert Ck.fingerprint_difference(fp, Hn.run_fingerprint(**dict(base, ema_decay=0.5, batch_size=4, lr=1.0))) == "batch_size"
    assert Ck.fingerprint_difference(fp, {k: v for k, v in fp.items() if k != "max_t"}) == "max_t"
    assert Ck.fingerprint_difference(fp, dict(fp, extra=1)) == "extra"
    # a saved fingerprint comes back from the file with lists for tuples and compares equal to the live one
    pol = ss.AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(2, 1))
    base = dict(base, class_weights=np.float32([0.5, 1.5, 1.0]))
    live = Hn.run_fingerprint(**dict(base, augment_policy=pol))
    assert Ck.fingerprint_difference(Ck._plain(live), live) is None
    assert Ck.fingerprint_difference(live, Hn.run_fingerprint(**dict(base, augment_policy=ss.AugmentPolicy.lineage()))) == "augment_policy"


def test_ema_warmup_schedule():
    from silent_speech_amd.train import ema_decay_at

    assert ema_decay_at(0.999, 0) == 1.0 / 10.0
    assert ema_decay_at(0.999, 1) == 2.0 / 11.0
    assert ema_decay_at(0.999, 89) == 90.0 / 99.0
    assert ema_decay_at(0.999, 10 ** 6) == 0.999          # (1 + t) / (10 + t) = 0.999991 there
    assert ema_decay_at(0.9, 89) == 0.9                   # 90 / 99 = 0.909 > 0.9: the decay itself from t = 80 on
    assert ema_decay_at(0.9, 79) == 80.0 / 89.0 < 0.9
    assert ema_decay_at(0.0, 5) == 0.0
    for t in (0, 1, 89, 10 ** 6):
        assert ema_decay_at(0.999, t, warmup=False) == 0.999
        assert ema_decay_at(0.999, t) == min(0.999, (1 + t) / (10 + t))


def test_optim_ref_against_torch_adam_clip_and_an_ema_loop():
    """Three steps of ``optim_ref.adam_clip_ema_step`` (float64) against ``clip_grad_norm_`` + ``torch.optim.Adam`` + a plain
    EMA loop on float64 tensors: the same arithmetic in another order, 1e-12 relative."""
    rng = np.random.default_rng(5)
    n, decay = 1000, 0.9
    p0 = rng.normal(size=n)
    grads = [rng.normal(size=n) * s for s in (0.2, 0.001, 3.0)]  # clipped, not clipped (norm 0.03), clipped hard
    p, m, v, ema = p0.copy(), np.zeros(n), np.zeros(n), p0.copy()
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=3e-4)
    t_ema = tp.detach().clone()
    for step, g in enumerate(grads, 1):
        total = OR.adam_clip_ema_step(p, g.copy(), m, v, ema, step, decay)
        tp.grad = torch.from_numpy(g.copy())
        t_total = torch.nn.utils.clip_grad_norm_([tp], 1.0)
        opt.step()
        t_ema.mul_(decay).add_(tp.detach(), alpha=1.0 - decay)
        assert abs(total - float(t_total)) <= 1e-12 * total
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-12 * np.abs(p).max()
        assert np.abs(ema - t_ema.numpy()).max() <= 1e-12 * np.abs(ema).max()
    assert np.abs(p - p0).max() > 1e-4 and np.abs(ema - p).max() > 1e-5  # the steps moved the weights; the average lags


def test_ema_expected_bound_is_two_ulp_of_the_larger_operand():
    e, bound = OR.ema_expected(np.float32([1.0, -3.0, 0.25]), np.float32([1.5, 1.0, -0.125]), 0.0)
    assert np.array_equal(e, [1.5, 1.0, -0.125])  # d = 0: p_new exactly
    assert np.array_equal(bound, 2 * np.float64([2.0 ** -23, 2.0 ** -22, 2.0 ** -25]))


def test_arguments_refused_before_any_device_is_touched(tmp_path):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    m = ss.BiGRUClassifier(20, 3, use_roi=False)
    for bad in (1.0, -0.1, float("nan"), 0.99999999):  # (the last one is 1.0 as float32)
        with pytest.raises(ValueError, match="ema_decay"):
            ss.Trainer(m, ema_decay=bad)
    with pytest.raises(RuntimeError, match="HIP device"):  # a good decay gets as far as the device check
        ss.Trainer(m, ema_decay=0.9)
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(tmp_path), str(tmp_path / "m.pt"), plan="host", state_path=str(tmp_path / "s.pt"))
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(tmp_path), str(tmp_path / "m.pt"), plan="host", resume=True)
    with pytest.raises(ValueError, match="state_path"):
        Hn.fit(str(tmp_path), str(tmp_path / "m.pt"), plan="device", resume=True)
