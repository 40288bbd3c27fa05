"""CPU: the host side of fine-tuning with a frozen ROI CNN -- the CNN's range of the flat bucket, the run fingerprint, the argument
checks of ``fit`` and of ``load_init_checkpoint``, the ABI of ``ss_batch_gather_z``.  No device is touched."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("roi_emb", [20, 32])
def test_cnn_range_is_the_padded_prefix_of_the_layout(roi_emb):
    import silent_speech_amd as ss

    m = ss.BiGRUClassifier(84, 5, use_roi=True, roi_emb=roi_emb)
    lay, total = m._layout()
    names = [name for name, *_ in lay]
    cnn = [name for name in names if name.startswith("roi_cnn.")]
    assert len(cnn) == 8 and names[:8] == cnn  # a prefix, nothing of the CNN behind it
    padded = sum((p.numel() + 3) // 4 * 4 for name, p in m.named_parameters() if name.startswith("roi_cnn."))
    n_cnn = m.cnn_param_range()
    assert n_cnn == padded and n_cnn % 4 == 0 and 0 < n_cnn < total
    assert lay[8][1] == n_cnn and lay[7][1] + lay[7][2] <= n_cnn  # the first GRU tensor starts there, the last CNN tensor ends before
    # (8*9 + 8) + (16*8*9 + 16) + (24*16*9 + 24) + (roi_emb*24 + roi_emb), each tensor padded to 4
    assert n_cnn == 72 + 8 + 1152 + 16 + 3456 + 24 + roi_emb * 24 + roi_emb
    assert ss.BiGRUClassifier(84, 5).cnn_param_range() == 0


FIELDS = dict(seed=42, batch_size=16, world_size=1, max_t=90, lr=3e-4, labels=["a", "b"], x_dim=84, use_roi=True, n_train=10, n_val=2,
              class_weights=None, augment_policy=None, ema_decay=None)


def test_run_fingerprint_is_unchanged_without_the_new_arguments():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    assert Hn.run_fingerprint(**FIELDS) == FIELDS and set(Hn.run_fingerprint(**FIELDS)) == set(Ck.FINGERPRINT_FIELDS)
    assert Hn.run_fingerprint(**FIELDS, init_from=None, freeze_cnn=False) == FIELDS
    pol = ss.AugmentPolicy.lineage()
    full = Hn.run_fingerprint(**dict(FIELDS, class_weights=np.array([1.0, 2.0], np.float32), augment_policy=pol, ema_decay=0.9))
    assert full == dict(FIELDS, class_weights=[1.0, 2.0], ema_decay=0.9,
                        augment_policy=dict(time_warp_prob=0.5, time_warp_range=[0.8, 1.2], scale_prob=0.3, scale_range=[0.95, 1.05],
                                            roi_shift_prob=0.0, roi_shift_max=[0, 0]))
    # set, they are two more entries and nothing else moves
    sha = "ab" * 32
    both = Hn.run_fingerprint(**FIELDS, init_from=sha, freeze_cnn=True)
    assert both == dict(FIELDS, init_from=sha, freeze_cnn=True)
    assert Hn.run_fingerprint(**FIELDS, init_from=sha) == dict(FIELDS, init_from=sha)
    assert Ck.fingerprint_difference(FIELDS, both) == "freeze_cnn" and Ck.fingerprint_difference(both, both) is None
    assert Ck.fingerprint_difference(dict(FIELDS, init_from=sha), dict(FIELDS, init_from="cd" * 32)) == "init_from"


def test_fit_checks_its_arguments_before_anything_else(tmp_path, monkeypatch):
    from silent_speech_amd import harness as Hn

    def never(*a, **k):
        raise AssertionError("fit went past its argument checks")

    monkeypatch.setattr(Hn, "scan_clips", never)
    monkeypatch.setattr(Hn, "DeviceClipStore", never)
    out = str(tmp_path / "o.pt")
    with pytest.raises(ValueError, match="init_from"):
        Hn.fit(str(tmp_path), out, plan="device", freeze_cnn=True)
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(str(tmp_path), out, plan="host", freeze_cnn=True, init_from="a.pt")
    from silent_speech_amd import AugmentPolicy

    with pytest.raises(ValueError, match="roi_shift"):
        Hn.fit(str(tmp_path), out, plan="device", freeze_cnn=True, init_from="a.pt",
               augment_policy=AugmentPolicy(roi_shift_prob=0.5, roi_shift_max=(1, 1)))


def test_init_checkpoint_must_fit_the_clips(tmp_path):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    path = str(tmp_path / "a.pt")
    ss.save_checkpoint(path, ss.BiGRUClassifier(84, 3, use_roi=True), ["a", "b", "c"], max_t=16, roi_w=32, roi_h=32)
    ck = Hn.load_init_checkpoint(path, 84, True, 32, 192)
    assert ck["labels"] == ["a", "b", "c"] and ck["model"]["head.4.weight"].shape == (3, 128)
    for field, args in (("x_dim", (83, True, 32, 192)), ("use_roi", (84, False, 32, 192)), ("roi_emb", (84, True, 20, 192)),
                        ("hidden", (84, True, 32, 128))):
        with pytest.raises(ValueError, match=field):
            Hn.load_init_checkpoint(path, *args)
    assert len(Hn.file_sha256(path)) == 64 and Hn.file_sha256(path) == Hn.file_sha256(path)


def test_trainer_arguments_need_no_device_to_be_refused():
    import silent_speech_amd as ss

    with pytest.raises(RuntimeError, match="f32 use_roi"):
        ss.Trainer(ss.BiGRUClassifier(84, 5), freeze_cnn=True)
    with pytest.raises(ValueError, match="micro_batches"):
        ss.Trainer(ss.BiGRUClassifier(84, 5, use_roi=True), freeze_cnn=True, micro_batches=2)


def test_gather_z_is_declared_exported_and_checks_its_arguments_on_the_host():
    """The header, the library and _lib.SIGNATURES agree on the new symbol; every SS_ERR_ARG case returns before a launch (the
    pointers below are never dereferenced on the host)."""
    from silent_speech_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    assert "int ss_batch_gather_z(" in hdr and len(_lib.SIGNATURES["ss_batch_gather_z"]) == 17
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    one = ctypes.cast(buf, ctypes.c_void_p).value  # 16-byte aligned or not, at least 4
    assert one % 4 == 0

    def status(feat=one, D=8, xmap=one, emb=one, E=4, rmap=one, fill=None, rows=4, nmap=None, std=0.0, scale=None, rpc=1, dst=one, ld=12):
        return lib.ss_batch_gather_z(feat, D, xmap, emb, E, rmap, fill, rows, nmap, std, 0, 0, scale, rpc, dst, ld, None)

    for bad in (dict(D=0), dict(E=0), dict(D=-1), dict(ld=11), dict(rows=0), dict(feat=None), dict(xmap=None), dict(dst=None),
                dict(emb=None), dict(std=-1.0), dict(scale=one, rpc=3), dict(scale=one, rpc=0), dict(dst=one + 2), dict(feat=one + 1),
                dict(emb=one + 3), dict(fill=one + 2), dict(rmap=one + 1)):
        assert status(**bad) == -1, bad
    assert not any(buf)
