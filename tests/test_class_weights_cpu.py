"""CPU: the class-weighted cross entropy's surface -- the four C-ABI entry points (declared, exported, prototyped, ABI version
unchanged), ``harness.balanced_class_weights`` against the reference's recipe (train_model_official.py:407-412) restated here,
and the weight validation of ``Trainer``, ``fit``, ``evaluate`` and ``evaluate_device`` (``ValueError`` before anything touches a
device)."""
import collections
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ss_class_weight_sum": 6, "ss_ce_ls_w_fwd_bwd": 11, "ss_tail_fwd_w": 34, "ss_eval_accum_w": 16}


def header_prototypes():
    txt = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ss_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_new_entry_points_are_declared_exported_and_prototyped():
    from silent_speech_amd import _lib

    protos = header_prototypes()
    lib = _lib.load()
    for name, n_args in NEW.items():
        assert name in protos, f"{name} is not declared in include/ss_hotpath.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
        declared = [a for a in protos[name].split(",") if a.strip()]
        assert len(declared) == n_args == len(_lib.SIGNATURES[name]), (name, len(declared), len(_lib.SIGNATURES[name]))
    # the weighted forms are the unweighted ones plus pointers: same number of leading arguments, the host denom gone
    assert len(_lib.SIGNATURES["ss_ce_ls_w_fwd_bwd"]) == len(_lib.SIGNATURES["ss_ce_ls_fwd_bwd"]) + 1
    assert len(_lib.SIGNATURES["ss_tail_fwd_w"]) == len(_lib.SIGNATURES["ss_tail_fwd"]) + 1
    assert len(_lib.SIGNATURES["ss_eval_accum_w"]) == len(_lib.SIGNATURES["ss_eval_accum"]) + 2
    assert lib.ss_abi_version() == 3


def test_argument_checks_of_the_new_entry_points_need_no_gpu():
    """NULL pointers and non-positive sizes are refused on the host, before any launch."""
    from silent_speech_amd import _lib

    lib = _lib.load()
    assert lib.ss_class_weight_sum(None, 4, None, 3, None, None) == -1
    assert lib.ss_class_weight_sum(8, 0, 8, 3, 8, None) == -1
    assert lib.ss_ce_ls_w_fwd_bwd(8, 8, 4, 3, 0.05, None, 8, None, None, None, None) == -1   # no weights
    assert lib.ss_ce_ls_w_fwd_bwd(8, 8, 4, 3, 0.05, 8, None, None, None, None, None) == -1   # no normaliser
    assert lib.ss_eval_accum_w(8, 8, 4, 3, 0.05, 0, 8, 8, None, 8, 8, 8, None, None, 8, None) == -1  # no wsum
    assert lib.ss_tail_fwd_w(*([8] * 10), 8, 2, 3, 8, 4, 3, 1e-5, 0.0, 0, 0, 0.05, None, 8, *([None] * 6), 8, 8, None, None, None) == -1


def test_balanced_class_weights_is_the_references_recipe():
    from silent_speech_amd import harness as Hn

    id_to_label = {0: "aura", 1: "maybe", 2: "no", 3: "yes"}
    train_labels = ["no"] * 24 + ["aura"] * 14 + ["yes"] * 7 + ["maybe"]
    np.random.default_rng(0).shuffle(train_labels)
    got = Hn.balanced_class_weights(train_labels, id_to_label)
    # train_model_official.py:407-412, restated
    train_counts = collections.Counter(train_labels)
    class_weights = torch.tensor([1.0 / train_counts[id_to_label[i]] for i in range(4)], dtype=torch.float32)
    class_weights = class_weights / class_weights.mean()
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (4,)
    assert got.tobytes() == class_weights.numpy().tobytes()
    assert abs(float(got.astype(np.float64).mean()) - 1.0) < 4 * 2.0 ** -24
    assert got[1] > got[3] > got[0] > got[2]  # the single-clip class weighs most
    np.testing.assert_allclose(got * np.array([14, 1, 24, 7]), np.full(4, got[1]), rtol=1e-6)


BAD = {"too short": [1.0, 1.0], "too long": [1.0] * 4, "zero": [1.0, 0.0, 1.0], "negative": [1.0, -0.5, 1.0],
       "nan": [1.0, float("nan"), 1.0], "inf": [1.0, float("inf"), 1.0], "float32 overflow": [1.0, 1e39, 1.0],
       "float32 underflow": [1.0, 1e-50, 1.0], "matrix": [[1.0, 1.0, 1.0]], "a word": "balanced-ish"}


@pytest.mark.parametrize("what", sorted(BAD))
def test_the_shared_check_rejects(what):
    from silent_speech_amd.train import check_class_weights

    with pytest.raises(ValueError):
        check_class_weights(BAD[what], 3)


def test_the_shared_check_accepts_sequences_arrays_and_tensors():
    from silent_speech_amd.train import check_class_weights

    for w in ([0.4, 2.1, 0.5], (0.4, 2.1, 0.5), np.array([0.4, 2.1, 0.5]), torch.tensor([0.4, 2.1, 0.5], dtype=torch.float64)):
        got = check_class_weights(w, 3)
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and got.tolist() == np.float32([0.4, 2.1, 0.5]).tolist()


@pytest.mark.parametrize("what", ["too short", "zero", "negative", "nan", "inf"])
def test_trainer_and_evaluate_reject_bad_weights_before_they_need_a_device(what):
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    m = ss.BiGRUClassifier(20, 3, use_roi=False)
    with pytest.raises(ValueError):
        ss.Trainer(m, class_weights=BAD[what])
    with pytest.raises(ValueError):
        Hn.evaluate(m, None, class_weights=BAD[what])
    with pytest.raises(ValueError):
        Hn.evaluate_device(m, None, class_weights=BAD[what])
    # good weights get as far as the device check
    with pytest.raises(RuntimeError, match="HIP device"):
        ss.Trainer(m, class_weights=[0.5, 1.5, 1.0])


@pytest.mark.parametrize("what", ["too long", "zero", "negative", "nan", "inf", "a word"])
def test_fit_rejects_bad_weights_after_the_scan(what, tmp_path):
    from silent_speech_amd import data as Dm
    from silent_speech_amd import harness as Hn

    rng = np.random.default_rng(0)
    for k in range(6):
        X = rng.normal(size=(5, 8)).astype(np.float32)
        Dm.save_clip(str(tmp_path / f"{k}.npz"), X, np.arange(5), ["aura", "no", "yes"][k % 3], "me", np.arange(4), None)
    with pytest.raises(ValueError):
        Hn.fit(str(tmp_path), str(tmp_path / "m.pt"), epochs=1, class_weights=BAD[what], device="cpu", log=lambda *a: None)


def test_the_public_arguments_exist_and_default_to_none():
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    for fn in (ss.Trainer.__init__, Hn.fit, Hn.evaluate, Hn.evaluate_device):
        assert inspect.signature(fn).parameters["class_weights"].default is None, fn
    assert inspect.signature(ss.Trainer.step).parameters["y_global"].default is None
