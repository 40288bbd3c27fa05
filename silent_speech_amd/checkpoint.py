"""``.pt`` checkpoint round trip with the reference scripts.

Writer: the dict of /root/reference/train_model_official.py:489-500.  Reader: ``load_classifier`` of
/root/reference/live_infer_official.py:198-221 (accepts the optional ``gru_layers`` key, hard-codes roi_emb=32 and
hidden=192 like the reference).  ``topk_from_logits``: live_infer_official.py:223-226.

The train-state file of ``harness.fit(state_path=)`` is a format of this project (the reference cannot resume): written
atomically by ``save_train_state``, read by ``load_train_state`` with ``weights_only=True``; ``fingerprint_difference`` names the
first setting in which a saved run and the resuming call disagree.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .model import BiGRUClassifier


def calibration_keys(temperature=None, calibration=None) -> dict:
    """The two optional checkpoint keys of a calibrated model (``calibrate.calibrate``): ``"temperature"`` (a positive finite
    float) and ``"calibration"`` (a dict of plain numbers and lists, ``Calibration.plain()``), each only when given.  The
    reference's loader ignores both.  Host code."""
    from .calibrate import check_temperature

    extra = {}
    if temperature is not None:
        extra["temperature"] = check_temperature(temperature)
    if calibration is not None:
        if not isinstance(calibration, dict):
            raise ValueError("calibration must be a dict of plain numbers and lists (Calibration.plain())")
        extra["calibration"] = _plain(calibration)
    return extra


def save_checkpoint(path: str, model: BiGRUClassifier, labels: Sequence[str], max_t: int = 90, roi_w: int = 96,
                    roi_h: int = 48, seed: int = 42, temperature=None, calibration=None) -> None:
    """``temperature`` / ``calibration``: see ``calibration_keys``; without them the file has exactly the reference's keys."""
    labels = list(labels)
    label_to_id = {lab: i for i, lab in enumerate(labels)}
    extra = calibration_keys(temperature, calibration)
    torch.save({
        "model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        "x_dim": model.cfg.x_dim, "max_t": max_t, "use_roi": bool(model.use_roi), "roi_w": roi_w, "roi_h": roi_h,
        "labels": labels, "label_to_id": label_to_id, "id_to_label": {i: lab for lab, i in label_to_id.items()},
        "seed": seed, "gru_layers": model.cfg.gru_layers, **extra,
    }, path)


def add_calibration(path: str, temperature, calibration) -> None:
    """Rewrite the checkpoint at ``path`` with the two calibration keys added (or replaced) and everything else as it was, weights
    bit for bit; atomically, as ``save_train_state`` writes."""
    extra = calibration_keys(temperature, calibration)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    ckpt.update(extra)
    _save_atomically(path, ckpt)


def load_classifier(path: str, device="cuda", roi_standardize: bool = True):
    """-> (model.eval() on ``device``, id_to_label, max_t, use_roi).  ``roi_standardize=False`` reproduces the live
    script's own forward (which skips the per-frame standardisation, SURVEY.md note N2)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    x_dim, max_t = int(ckpt["x_dim"]), int(ckpt["max_t"])
    use_roi = bool(ckpt.get("use_roi", False))
    labels = ckpt["labels"]
    model = BiGRUClassifier(x_dim=x_dim, num_classes=len(labels), use_roi=use_roi, roi_emb=32, hidden=192,
                            gru_layers=int(ckpt.get("gru_layers", 2)), roi_standardize=roi_standardize)
    model.load_state_dict(ckpt["model"])
    model.to(device).eval()
    # the fitted temperature of a calibrated checkpoint (1.0 without one): a plain attribute, no parameter or buffer
    model.temperature = float(ckpt.get("temperature", 1.0))
    return model, ckpt["id_to_label"], max_t, use_roi


TRAIN_STATE_FORMAT = 1
# the order in which a resuming ``fit`` compares the fingerprint of the saved run with its own (the first difference is named)
FINGERPRINT_FIELDS = ("seed", "batch_size", "world_size", "max_t", "lr", "labels", "x_dim", "use_roi", "n_train", "n_val",
                      "class_weights", "augment_policy", "ema_decay")


def _plain(v):
    """Tensors to the CPU, tuples to lists, recursively: what ``torch.load(weights_only=True)`` reads back unchanged."""
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def save_train_state(path: str, state: dict) -> None:
    """``torch.save`` of ``state`` (tensors, numbers, strings, lists, dicts, None) to ``path``, atomically: the bytes go to a
    temporary name in the same directory and ``os.replace`` puts the finished file in place, so a writer that dies midway
    leaves the previous file as it was."""
    _save_atomically(path, _plain(state))


def _save_atomically(path: str, obj) -> None:
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def load_train_state(path: str) -> dict:
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or state.get("format") != TRAIN_STATE_FORMAT:
        raise ValueError(f"{path} is not a train-state file of format {TRAIN_STATE_FORMAT}")
    return state


def fingerprint_difference(saved: dict, current: dict) -> Optional[str]:
    """The first field of ``FINGERPRINT_FIELDS`` (then any other key, sorted) whose values differ between the two
    fingerprints, or None.  Pure host code: values are numbers, strings, None, lists and dicts of these."""
    rest = sorted((set(saved) | set(current)) - set(FINGERPRINT_FIELDS))
    missing = object()
    for name in list(FINGERPRINT_FIELDS) + rest:
        if _plain(saved.get(name, missing)) != _plain(current.get(name, missing)):
            return name
    return None


def softmax_topk(logits: torch.Tensor, k: int = 3, temperature=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ss_softmax_topk`` over a (B, C) batch of logits on the device: -> (probs (B,k) f32, class ids (B,k) int32),
    most probable first.  What the serving path returns for thousands of windows instead of raw logits.
    ``temperature`` (a positive finite number, e.g. ``model.temperature`` of a calibrated checkpoint; anything else is a
    ``ValueError``): the probabilities of ``softmax(logits / temperature)`` by ``ss_softmax_topk_t``; the class ids do not change."""
    from . import _lib as L

    if temperature is not None:
        from .calibrate import check_temperature

        temperature = check_temperature(temperature)  # (host code, before anything touches the device)
    if not logits.is_cuda:
        raise RuntimeError("softmax_topk runs on the HIP device (there is no CPU path)")
    lg = logits.detach().float().contiguous().reshape(-1, logits.shape[-1])
    B, C = lg.shape
    probs = torch.empty(B, k, device=lg.device, dtype=torch.float32)
    idx = torch.empty(B, k, device=lg.device, dtype=torch.int32)
    if temperature is None:
        L.call("ss_softmax_topk", lg.data_ptr(), B, C, k, probs.data_ptr(), idx.data_ptr(), L.stream())
    else:
        inv_temp = torch.full((1,), 1.0 / temperature, device=lg.device, dtype=torch.float32)
        L.call("ss_softmax_topk_t", lg.data_ptr(), B, C, k, inv_temp.data_ptr(), probs.data_ptr(), idx.data_ptr(), L.stream())
    return probs, idx


def topk_from_logits(logits: torch.Tensor, id_to_label: Dict[int, str], k: int = 3, temperature=None) -> List[Tuple[str, float]]:
    """live_infer_official.py:223-226 for one clip's logits (1, C): [(label, probability)] of the k most probable.
    ``temperature``: as in ``softmax_topk``."""
    probs, idx = softmax_topk(logits.reshape(1, -1), min(k, logits.numel()), temperature=temperature)
    return [(id_to_label[int(i)], float(p)) for p, i in zip(probs[0].cpu().tolist(), idx[0].cpu().tolist())]
