"""Calibrated confidences: post-hoc temperature scaling fitted on the validation clips, and the reliability of the probabilities
the serving side prints (``ss_softmax_topk`` behind ``topk_from_logits``, live_infer_official.py:223-226).

Label smoothing, mixup, class weights, a teacher's soft targets and weight averaging all push the softmax probabilities away from
the hit rates they claim to be.  One scalar T, fitted on held-out logits by minimising the plain negative log-likelihood of
``softmax(logits / T)``, is the standard correction; it changes no arg-max and so no accuracy.  Here the fit and every measurement
stay on the device (``csrc/calib.hip``): ``fit_temperature`` enqueues ``FIT_ITERS`` pairs of launches and reads nothing back,
``reliability`` fills integer histograms, and ``calibrate`` ends in ONE host read.  DESIGN.md, "Calibrated confidences".

    cal = calibrate(model, val_store)                 # -> Calibration
    save_checkpoint(path, model, labels, temperature=cal.temperature, calibration=cal.plain())
    model, id_to_label, max_t, use_roi = load_classifier(path)      # model.temperature
    topk_from_logits(logits, id_to_label, temperature=model.temperature)
"""
from __future__ import annotations

import dataclasses
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

# the constants of include/ss_hotpath.h (tests/test_calib_cpu.py compares them with the header)
U_MIN, U_MAX, FIT_ITERS, MAX_PARTIALS = 0.05, 20.0, 35, 256
F32_MIN_NORMAL, F32_MAX = 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127
STATE_FIELDS = ("u", "lo", "hi", "nll", "g", "nll_at_1", "iteration", "at_bound")


def check_temperature(temperature) -> float:
    """A temperature the serving entry points accept: a positive finite number whose inverse is a normal float32 (the kernel
    reads 1 / T as one).  ``ValueError`` otherwise.  Host code."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.floating, np.integer)):
        raise ValueError(f"temperature must be a positive finite number, not {temperature!r}")
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0 and F32_MIN_NORMAL <= 1.0 / t <= F32_MAX):
        raise ValueError(f"temperature must be a positive finite number, not {temperature!r}")
    return t


def check_bins(n_bins, k_max) -> Tuple[int, int]:
    """``n_bins`` and ``k_max`` as ``ss_calib_bins`` takes them: integers in 1..64.  ``ValueError`` otherwise.  Host code."""
    for name, v in (("n_bins", n_bins), ("k_max", k_max)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 64:
            raise ValueError(f"{name} must be an integer in 1..64, not {v!r}")
    return int(n_bins), int(k_max)


def n_partials_for(n_rows: int) -> int:
    """Workgroups (= partial-sum slots) of an ``ss_calib_moments`` launch over ``n_rows`` rows: four rows per workgroup, capped."""
    return max(1, min(MAX_PARTIALS, (int(n_rows) + 3) // 4))


def _check_logits(logits: torch.Tensor, y: torch.Tensor, min_classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    if not logits.is_cuda or not y.is_cuda:
        raise RuntimeError("calibration runs on the HIP device (there is no CPU path)")
    if logits.dim() != 2 or y.dim() != 1 or y.shape[0] != logits.shape[0] or logits.shape[0] == 0:
        raise ValueError("logits must be (N, C) and y (N,), N > 0")
    if logits.shape[1] < min_classes:
        raise ValueError(f"calibration needs at least {min_classes} classes")
    return logits.detach().float().contiguous(), y.to(torch.int64).contiguous()


@torch.no_grad()
def collect_logits(model, store, batch_size: int = 16, embedded: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits (N, C) f32, y (N,) int64) of every clip of ``store``, in order, on the device: eval mode, no augmentation,
    batches planned by ``store.batch(rng="philox")`` as ``evaluate_device`` plans them; nothing is read back.
    ``embedded`` (after ``store.embed(model)``): ``model.forward_embedded`` on ``store.batch(embedded=True)``."""
    C, dev = model.cfg.num_classes, model.flat_params.device
    N = len(store)
    logits_all = torch.empty(N, C, device=dev, dtype=torch.float32)
    y_all = torch.empty(N, device=dev, dtype=torch.int64)
    every = torch.arange(N, dtype=torch.int32, device=store.device)
    was_training = model.training
    model.eval()
    for b0 in range(0, N, batch_size):
        b1 = min(N, b0 + batch_size)
        if embedded:
            Z, T, _, y = store.batch(every[b0:b1], augment=False, rng="philox", embedded=True)
            logits = model.forward_embedded(Z, T)
        else:
            X, T, R, y = store.batch(every[b0:b1], augment=False, rng="philox")
            logits = model(X, T, R if model.use_roi else None)
        logits_all[b0:b1].copy_(logits)
        y_all[b0:b1].copy_(y)
    model.train(was_training)
    return logits_all, y_all


def new_state(device) -> torch.Tensor:
    """The state a fit starts from (``STATE_FIELDS``, float64, on ``device``)."""
    return torch.tensor([1.0, U_MIN, U_MAX, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=device)


def fit_temperature(logits: torch.Tensor, y: torch.Tensor, err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fit u = 1 / T on device logits (N, C) and labels (N,): -> the device state (8 float64, ``STATE_FIELDS``).  Enqueues the
    ``FIT_ITERS`` (``ss_calib_moments``, ``ss_calib_bisect``) pairs and reads nothing back; bit-reproducible from run to run.
    ``err_flag`` (one device int32 the caller cleared): set when a label is outside [0, C) -- such rows count nowhere."""
    from . import _lib as L

    lg, yy = _check_logits(logits, y, 2)
    N, C = lg.shape
    n_part = n_partials_for(N)
    state = new_state(lg.device)
    partials = torch.empty(2 * n_part, dtype=torch.float64, device=lg.device)
    if err_flag is None:
        err_flag = torch.zeros(1, dtype=torch.int32, device=lg.device)
    for _ in range(FIT_ITERS):
        L.call("ss_calib_moments", lg.data_ptr(), yy.data_ptr(), N, C, state.data_ptr(), partials.data_ptr(), n_part,
               err_flag.data_ptr(), L.stream())
        L.call("ss_calib_bisect", state.data_ptr(), partials.data_ptr(), n_part, L.stream())
    return state


def reliability(logits: torch.Tensor, y: torch.Tensor, inv_temp: Optional[torch.Tensor] = None, n_bins: int = 15, k_max: int = 5,
                err_flag: Optional[torch.Tensor] = None):
    """``ss_calib_bins`` over device logits (N, C) and labels (N,) at the inverse temperature ``inv_temp`` (a one-float device
    tensor; None: 1) -> device integer tensors (bin_count (n_bins) i32, bin_hits (n_bins) i32, bin_conf_fx (n_bins) i64 = sum of
    round(confidence * 2^32), rank_hist (k_max + 1) i32 with the last entry "rank >= k_max").  Nothing is read back."""
    from . import _lib as L

    n_bins, k_max = check_bins(n_bins, k_max)
    lg, yy = _check_logits(logits, y, 1)
    N, C = lg.shape
    dev = lg.device
    if inv_temp is not None:
        if not inv_temp.is_cuda or inv_temp.dtype != torch.float32 or inv_temp.numel() != 1:
            raise ValueError("inv_temp must be a one-element float32 tensor on the device")
    bin_count = torch.zeros(n_bins, dtype=torch.int32, device=dev)
    bin_hits = torch.zeros(n_bins, dtype=torch.int32, device=dev)
    bin_conf_fx = torch.zeros(n_bins, dtype=torch.int64, device=dev)
    rank_hist = torch.zeros(k_max + 1, dtype=torch.int32, device=dev)
    if err_flag is None:
        err_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("ss_calib_bins", lg.data_ptr(), yy.data_ptr(), N, C, L.ptr(inv_temp), n_bins, k_max, bin_count.data_ptr(),
           bin_hits.data_ptr(), bin_conf_fx.data_ptr(), rank_hist.data_ptr(), err_flag.data_ptr(), L.stream())
    return bin_count, bin_hits, bin_conf_fx, rank_hist


def bin_stats(bin_count, bin_hits, bin_conf_fx):
    """Float64, on the host, from the integers of ``reliability``: -> (acc (n_bins), conf (n_bins), ece, mce).  An empty bin has
    accuracy and confidence 0 and adds nothing.  ece = sum_b count_b / n |acc_b - conf_b|, mce = max over the non-empty bins."""
    cnt = np.asarray(bin_count, np.float64)
    some = cnt > 0
    safe = np.where(some, cnt, 1.0)
    acc = np.where(some, np.asarray(bin_hits, np.float64) / safe, 0.0)
    conf = np.where(some, np.asarray(bin_conf_fx, np.float64) / 4294967296.0 / safe, 0.0)
    n = cnt.sum()
    gap = np.abs(acc - conf)
    ece = float((cnt * gap).sum() / n) if n > 0 else 0.0
    mce = float(gap[some].max()) if some.any() else 0.0
    return acc, conf, ece, mce


def topk_accuracy(rank_hist) -> List[float]:
    """[top-1, ..., top-k_max accuracy] from the prefix sums of ``rank_hist`` (k_max + 1 counts).  Float64, host."""
    h = np.asarray(rank_hist, np.float64)
    n = h.sum()
    return [float(v) for v in (np.cumsum(h[:-1]) / (n if n > 0 else 1.0))]


@dataclasses.dataclass
class Calibration:
    """What ``calibrate`` measured.  ``nll_*``: per-clip mean of the plain negative log-likelihood (no smoothing) at T = 1 and at
    the fitted T; ``ece_*`` / ``mce_after``: expected / maximum calibration error over ``n_bins`` equal-width confidence bins;
    ``topk_acc[k - 1]``: the share of clips whose true class is among the k most probable; the ``bin_*`` lists are per bin, before
    (T = 1) and after; ``n``: clips counted; ``at_bound``: -1 / +1 when the fit ended at the lower / upper bound of u = 1 / T."""
    temperature: float
    nll_before: float
    nll_after: float
    ece_before: float
    ece_after: float
    mce_after: float
    topk_acc: List[float]
    bin_count_before: List[int]
    bin_acc_before: List[float]
    bin_conf_before: List[float]
    bin_count_after: List[int]
    bin_acc_after: List[float]
    bin_conf_after: List[float]
    n: int
    at_bound: int

    def plain(self) -> dict:
        """Plain numbers and lists: what ``save_checkpoint(calibration=)`` stores."""
        return dataclasses.asdict(self)


def calibration_from_host(state, before, after, rank_hist) -> Calibration:
    """``Calibration`` from what the device computed, on the host in float64: ``state`` the 8 doubles of the fit, ``before`` /
    ``after`` the (bin_count, bin_hits, bin_conf_fx) of T = 1 and of the fitted T, ``rank_hist``."""
    st = dict(zip(STATE_FIELDS, (float(v) for v in state)))
    n = int(np.asarray(before[0], np.int64).sum())
    acc0, conf0, ece0, _ = bin_stats(*before)
    acc1, conf1, ece1, mce1 = bin_stats(*after)
    return Calibration(temperature=float(np.float32(1.0 / st["u"])), nll_before=st["nll_at_1"] / max(1, n),
                       nll_after=st["nll"] / max(1, n), ece_before=ece0, ece_after=ece1, mce_after=mce1,
                       topk_acc=topk_accuracy(rank_hist), bin_count_before=[int(v) for v in before[0]],
                       bin_acc_before=acc0.tolist(), bin_conf_before=conf0.tolist(), bin_count_after=[int(v) for v in after[0]],
                       bin_acc_after=acc1.tolist(), bin_conf_after=conf1.tolist(), n=n, at_bound=int(st["at_bound"]))


@torch.no_grad()
def calibrate(model, store, batch_size: int = 16, n_bins: int = 15, k_max: int = 5, embedded: bool = False) -> Calibration:
    """Fit the temperature of ``model`` on every clip of ``store`` and measure the reliability before and after: logits by
    ``collect_logits``, the fit, two ``reliability`` passes (T = 1 and the fitted T, whose inverse goes from the fit's state to the
    kernel on the device) -- all enqueue-only -- then ONE host read of everything.  A label outside the model's classes is a
    ``ValueError``, as in ``evaluate_device``.  ``Calibration.temperature`` is the float32 value a checkpoint keeps."""
    n_bins, k_max = check_bins(n_bins, k_max)
    if model.cfg.num_classes < 2:
        raise ValueError("calibration needs at least 2 classes")
    if len(store) == 0:
        raise ValueError("calibration needs at least one clip")
    logits, y = collect_logits(model, store, batch_size, embedded=embedded)
    err = torch.zeros(1, dtype=torch.int32, device=logits.device)
    state = fit_temperature(logits, y, err_flag=err)
    before = reliability(logits, y, None, n_bins, k_max, err_flag=err)
    after = reliability(logits, y, state[0:1].to(torch.float32), n_bins, k_max, err_flag=err)
    # the one read: the state's bits ride as int64 beside the integers, so nothing is rounded on the way
    parts = [state.view(torch.int64), err.long()] + [t.long() for t in before[:3]] + [t.long() for t in after[:3]] + [after[3].long()]
    host = torch.cat(parts).cpu().numpy()
    model.check_health()  # (the read above has synchronised)
    st = host[:8].view(np.float64)
    if int(host[8]):
        raise ValueError("calibrate: a label of the store is outside the model's %d classes" % model.cfg.num_classes)
    ints = host[9:]
    cut = [ints[i * n_bins:(i + 1) * n_bins] for i in range(6)]
    return calibration_from_host(st, cut[0:3], cut[3:6], ints[6 * n_bins:])
