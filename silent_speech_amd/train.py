"""Fused training step: forward -> CE(label smoothing) -> backward -> [RCCL all-reduce] -> clip -> Adam.

Counterpart of the loop body of /root/reference/train_model_official.py:433-443 with
``Adam(lr=3e-4)`` (:403), ``CrossEntropyLoss(label_smoothing=0.05)`` (:405) and
``clip_grad_norm_(.., 1.0)`` (:438).  No autograd graph, no host synchronisation inside a step: the
loss and the hit count stay on the device until the caller asks for them.

Data parallelism (the reference has none): one process per GPU, each rank holds a full replica and
takes its shard of the clips; the only exchange is ONE all-reduce (sum) of the flat fp32 gradient
bucket between backward and clip, so the global-norm clip sees the gradient of the whole global
batch exactly as a single process would.  ``torch.distributed`` backend "nccl" is RCCL on ROCm.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import engine as E
from .model import BiGRUClassifier, ParamGroup, no_decay


def shard_range(n_items: int, rank: int, world: int):
    """Contiguous clip shard of rank ``rank``: [lo, hi).  Equal shards when world | n_items."""
    per = (n_items + world - 1) // world
    lo = min(n_items, rank * per)
    return lo, min(n_items, lo + per)


def allreduce_flat_grads(flat: torch.Tensor, group=None, always: bool = False) -> None:
    """Sum the flat gradient bucket over ranks (one collective per step).  ``always`` issues the collective on a
    one-rank group too (a sum over one rank: the identity) -- how the RCCL leg is exercised on a one-GPU box."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and (always or dist.get_world_size(group) > 1):
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)


def check_class_weights(class_weights, num_classes: int) -> np.ndarray:
    """The class weights of ``CrossEntropyLoss(weight=)`` as a float32 array of ``num_classes`` entries.  ``ValueError`` unless
    they are that many finite, strictly positive numbers (as float32 too): the normaliser sum of w[y] then is positive whatever the
    batch holds, so torch's NaN for a batch of zero-weight rows has no counterpart here."""
    if isinstance(class_weights, str):
        raise ValueError(f"class_weights must be a sequence of {num_classes} numbers, not {class_weights!r}")
    if isinstance(class_weights, torch.Tensor):
        class_weights = class_weights.detach().cpu().numpy()
    try:
        w64 = np.asarray(class_weights, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"class_weights must be a sequence of {num_classes} numbers") from e
    if w64.shape != (num_classes,):
        raise ValueError(f"class_weights must hold one weight per class: shape ({num_classes},), not {w64.shape}")
    with np.errstate(over="ignore"):
        w = w64.astype(np.float32)
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("class_weights must be finite and strictly positive")
    return np.ascontiguousarray(w)


def check_distill(alpha, temperature):
    """The blend and the temperature of a distillation loss as floats.  ``ValueError`` unless 0 <= alpha <= 1 and temperature is
    finite and > 0, both as the float32 the kernels take.  Host code: nothing here touches a device."""
    try:
        a, t = float(np.float32(alpha)), float(np.float32(temperature))
    except (TypeError, ValueError):
        raise ValueError(f"distill_alpha and distill_temperature must be numbers, not {alpha!r} and {temperature!r}") from None
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"distill_alpha must lie in [0, 1], not {alpha!r}")
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"distill_temperature must be finite and > 0, not {temperature!r}")
    return float(alpha), float(temperature)


def check_weight_decay(weight_decay) -> None:
    """``ValueError`` unless ``weight_decay`` is finite and >= 0.  Host code, for ``Trainer`` and ``harness.fit`` alike."""
    if not (math.isfinite(float(weight_decay)) and float(weight_decay) >= 0.0):
        raise ValueError(f"weight_decay must be finite and >= 0, not {weight_decay!r}")


def check_sam_rho(sam_rho):
    """The neighbourhood radius of sharpness-aware minimisation as a float, or None (off).  ``ValueError`` unless it is finite and
    > 0 as the float32 the kernel takes.  Host code, for ``Trainer`` and ``harness.fit`` alike: nothing here touches a device."""
    if sam_rho is None:
        return None
    try:
        with np.errstate(over="ignore"):
            r = float(np.float32(sam_rho))
    except (TypeError, ValueError):
        raise ValueError(f"sam_rho must be a number or None, not {sam_rho!r}") from None
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"sam_rho must be finite and > 0 as float32, not {sam_rho!r}")
    return float(sam_rho)


def check_lr_schedule(lr_schedule) -> None:
    """``TypeError`` unless ``lr_schedule`` is None or an ``LrSchedule``.  Host code, for ``Trainer`` and ``harness.fit`` alike."""
    if lr_schedule is not None and not isinstance(lr_schedule, LrSchedule):
        raise TypeError("lr_schedule must be an LrSchedule")


def ema_decay_at(decay: float, t: int, warmup: bool = True) -> float:
    """The decay of the weight average at step ``t`` (``Trainer.step_count`` of the step being taken: 1 for the first), in
    double: ``min(decay, (1 + t) / (10 + t))`` -- the early steps, whose average would otherwise be dominated by the initial
    weights, average over a short window -- or ``decay`` itself without warm-up."""
    decay = float(decay)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


@dataclasses.dataclass(frozen=True)
class LrSchedule:
    """A learning-rate factor that is a pure function of ``Trainer.step_count`` (the number of the step being taken, 1 for the
    first), evaluated in float64 -- nothing to save, so a resumed run continues it exactly:

        step <= warmup_steps                 step / warmup_steps                 (linear warm-up; its last step runs at 1)
        decay "none"                         1
        warmup_steps < step < total_steps    t = (step - warmup_steps) / (total_steps - warmup_steps)
            "linear"                         1 - (1 - final_frac) * t
            "cosine"                         final_frac + (1 - final_frac) * (1 + cos(pi * t)) / 2
        step >= total_steps                  final_frac                          (held there)

    ``total_steps=None`` with a decay is filled by ``harness.fit`` (epochs x batches per epoch); evaluating such a schedule
    without it is a ``ValueError``."""
    warmup_steps: int = 0
    decay: str = "none"
    total_steps: Optional[int] = None
    final_frac: float = 0.0

    def __post_init__(self):
        if self.decay not in ("none", "linear", "cosine"):
            raise ValueError(f"LrSchedule.decay must be 'none', 'linear' or 'cosine', not {self.decay!r}")
        if int(self.warmup_steps) != self.warmup_steps or self.warmup_steps < 0:
            raise ValueError(f"LrSchedule.warmup_steps must be an integer >= 0, not {self.warmup_steps!r}")
        if self.total_steps is not None and (int(self.total_steps) != self.total_steps or self.total_steps <= self.warmup_steps):
            raise ValueError(f"LrSchedule.total_steps must be an integer > warmup_steps, not {self.total_steps!r}")
        if not 0.0 <= float(self.final_frac) <= 1.0:  # (a NaN fails both)
            raise ValueError(f"LrSchedule.final_frac must lie in [0, 1], not {self.final_frac!r}")

    def __call__(self, step: int) -> float:
        step, w = max(int(step), 1), int(self.warmup_steps)
        if step <= w:  # (w > 0: a step count is at least 1)
            return max(step, 0) / float(w)
        if self.decay == "none":
            return 1.0
        if self.total_steps is None:
            raise ValueError("LrSchedule: a decay needs total_steps (harness.fit fills it in)")
        f = float(self.final_frac)
        if step >= self.total_steps:
            return f
        t = (step - w) / float(int(self.total_steps) - w)
        return 1.0 - (1.0 - f) * t if self.decay == "linear" else f + (1.0 - f) * 0.5 * (1.0 + math.cos(math.pi * t))

    def plain(self) -> dict:
        return dict(warmup_steps=int(self.warmup_steps), decay=self.decay,
                    total_steps=None if self.total_steps is None else int(self.total_steps), final_frac=float(self.final_frac))


class PlateauSchedule:
    """torch's ``ReduceLROnPlateau`` (relative threshold, cooldown 0) as a scale on the learning rate; the defaults are
    inactive/train_reduced.py:199's (``mode='max', factor=0.5, patience=10``) and torch's (``threshold=1e-4``).  ``step(metric)``
    once per epoch: a metric that beats the best one by more than the threshold -- ``> best * (1 + threshold)`` for "max",
    ``< best * (1 - threshold)`` for "min" -- becomes the best and clears the count of bad epochs; any other adds one to it, and
    when the count exceeds ``patience`` the scale becomes ``max(scale * factor, min_scale)`` and the count starts again.  (torch
    also ignores reductions of the lr by less than ``eps=1e-8``; a scale has no such floor but ``min_scale``.)  -> True when the
    scale moved.  The state -- ``best``, ``bad``, ``scale`` -- is three numbers (``state_dict`` / ``load_state_dict``)."""

    def __init__(self, mode: str = "max", factor: float = 0.5, patience: int = 10, threshold: float = 1e-4, min_scale: float = 0.0):
        if mode not in ("max", "min"):
            raise ValueError(f"PlateauSchedule.mode must be 'max' or 'min', not {mode!r}")
        if not 0.0 < float(factor) < 1.0:
            raise ValueError(f"PlateauSchedule.factor must lie in (0, 1), not {factor!r}")
        if int(patience) != patience or patience < 0:
            raise ValueError(f"PlateauSchedule.patience must be an integer >= 0, not {patience!r}")
        if not (float(threshold) >= 0.0 and 0.0 <= float(min_scale) <= 1.0):
            raise ValueError("PlateauSchedule: threshold must be >= 0 and min_scale lie in [0, 1]")
        self.mode, self.factor, self.patience = mode, float(factor), int(patience)
        self.threshold, self.min_scale = float(threshold), float(min_scale)
        self.reset()

    def reset(self) -> None:
        self.best = -math.inf if self.mode == "max" else math.inf
        self.bad, self.scale = 0, 1.0

    def step(self, metric: float) -> bool:
        metric = float(metric)
        better = metric > self.best * (1.0 + self.threshold) if self.mode == "max" else metric < self.best * (1.0 - self.threshold)
        if better:
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            self.bad = 0
            new = max(self.scale * self.factor, self.min_scale)
            moved, self.scale = new != self.scale, new
            return moved
        return False

    def plain(self) -> dict:
        return dict(mode=self.mode, factor=self.factor, patience=self.patience, threshold=self.threshold, min_scale=self.min_scale)

    def state_dict(self) -> dict:
        return dict(best=float(self.best), bad=int(self.bad), scale=float(self.scale))

    def load_state_dict(self, state: dict) -> None:
        self.best, self.bad, self.scale = float(state["best"]), int(state["bad"]), float(state["scale"])


class SegmentTable:
    """The host arrays of one ``ss_adamw_clip_groups`` launch, built once per ``Trainer``: the segments of
    ``model.param_segments(param_groups, lo)`` and one (lr scale, weight decay) pair per group, the default group last (scale 1,
    the trainer's decay; a group's ``weight_decay=None`` inherits it).  The library reads them during the call and hands them to
    the kernel by value: nothing here lives on the device.  ``plain()`` is the table as lists, for ``state_dict``."""

    def __init__(self, model: BiGRUClassifier, param_groups, weight_decay: float, lo: int = 0):
        groups = tuple(param_groups or ())
        ends, ids, members = model.param_segments(groups, lo)
        self.n = model._layout()[1] - lo
        assert ends[-1] == self.n and all(e % 4 == 0 for e in ends)
        self.match = [list(g.match) for g in groups] + [[]]
        self.lr_scale = [g.lr_scale for g in groups] + [1.0]
        self.weight_decay = [float(weight_decay) if g.weight_decay is None else g.weight_decay for g in groups] + [float(weight_decay)]
        self.seg_end, self.seg_group, self.members = list(ends), list(ids), members
        self._end = (C.c_long * len(ends))(*ends)
        self._group = (C.c_int * len(ids))(*ids)
        self._scale = (C.c_float * len(self.lr_scale))(*self.lr_scale)
        self._decay = (C.c_float * len(self.weight_decay))(*self.weight_decay)

    @property
    def args(self):
        """(seg_end, seg_group, n_seg, group_lr_scale, group_weight_decay, n_groups) as the entry point takes them."""
        return (C.addressof(self._end), C.addressof(self._group), len(self.seg_end), C.addressof(self._scale),
                C.addressof(self._decay), len(self.lr_scale))

    def plain(self) -> dict:
        return dict(seg_end=[int(e) for e in self.seg_end], seg_group=[int(g) for g in self.seg_group], match=self.match,
                    lr_scale=[float(np.float32(x)) for x in self.lr_scale], weight_decay=[float(np.float32(x)) for x in self.weight_decay])


def check_lamb_exclude(exclude):
    """``enable_lamb(exclude=)`` / ``fit_lamb(lamb_exclude=)`` as a tuple of name patterns with ``ParamGroup.match``'s semantics (a
    prefix, or ``*`` + a suffix); None: what ``no_decay()`` matches, the biases and the LayerNorm.  An empty sequence excludes
    nothing.  ``ValueError`` for anything else.  Host code: nothing here touches a device."""
    if exclude is None:
        return tuple(no_decay().match)
    pats = (exclude,) if isinstance(exclude, str) else exclude
    try:
        pats = tuple(pats)
    except TypeError:
        raise ValueError(f"lamb exclude must be a name pattern or a sequence of them, not {exclude!r}") from None
    if not all(isinstance(p, str) and p not in ("", "*") for p in pats):
        raise ValueError(f"lamb exclude must hold non-empty name prefixes (or '*' + suffix), not {exclude!r}")
    return pats


class LambTable:
    """The host arrays of the two LAMB launches (``ss_lamb_moments``, ``ss_lamb_apply``), built once by ``Trainer.enable_lamb``:
    ``model.param_tensor_segments`` -- one segment per parameter tensor of ``[lo, n)``, since the norms are per tensor -- the
    trainer's groups as ``SegmentTable`` holds them (one default group without any), and ``seg_adapt``: 0 for the tensors whose
    name matches one of ``exclude`` (they take the trust ratio 1), 1 for the others."""

    def __init__(self, model: BiGRUClassifier, param_groups, weight_decay: float, exclude, lo: int = 0):
        groups = tuple(param_groups or ())
        ends, ids, names = model.param_tensor_segments(groups, lo)
        self.n = model._layout()[1] - lo
        assert ends[-1] == self.n and all(e % 4 == 0 for e in ends)
        self.exclude = tuple(exclude)
        self.names, self.seg_end, self.seg_group = list(names), list(ends), list(ids)
        self.adapt = [0 if any(ParamGroup.pattern_matches(p, name) for p in self.exclude) else 1 for name in names]
        self.lr_scale = [g.lr_scale for g in groups] + [1.0]
        self.weight_decay = [float(weight_decay) if g.weight_decay is None else g.weight_decay for g in groups] + [float(weight_decay)]
        self._end = (C.c_long * len(ends))(*ends)
        self._group = (C.c_int * len(ids))(*ids)
        self._scale = (C.c_float * len(self.lr_scale))(*self.lr_scale)
        self._decay = (C.c_float * len(self.weight_decay))(*self.weight_decay)
        self._adapt = (C.c_int * len(self.adapt))(*self.adapt)

    @property
    def args(self):
        """(seg_end, seg_group, n_seg, group_lr_scale, group_weight_decay, n_groups, seg_adapt) as the entry points take them."""
        return (C.addressof(self._end), C.addressof(self._group), len(self.seg_end), C.addressof(self._scale),
                C.addressof(self._decay), len(self.lr_scale), C.addressof(self._adapt))


class Trainer:
    """``micro_batches`` > 1 splits this rank's clips into that many equal slices which travel through forward and
    backward on their own HIP streams.  The GRU recurrence is latency-bound and occupies only one CU per
    (16-clip slice, direction); with two slices in flight the ROI-CNN / GEMM kernels of one slice fill the CUs
    the other slice's recurrence leaves idle.  The arithmetic is unchanged: every slice divides its loss by the
    global batch and adds its gradient into the same flat bucket (float atomics).

    Measured on MI355X at B=256: 2 staggered slices gain 1 % (3.66 vs 3.71 ms/step) -- the overlap is
    real (the second slice's CNN forward runs under the first slice's recurrence) but the half-size persistent CNN
    launches on 224 CUs lose what it wins -- so the default stays 1.

    ``class_weights`` (``num_classes`` finite positive numbers, or None): ``CrossEntropyLoss(weight=class_weights,
    label_smoothing=)``, the reference's commented-out loss (train_model_official.py:406-414).  The weighted mean divides by the
    sum of w[y] over the GLOBAL batch; that sum is taken on the device, per step, by one ``ss_class_weight_sum`` launch over
    ``step(y_global=)`` and read by the fused tail from device memory -- no read-back, no collective.  Without weights a step
    issues exactly the launches it always has.

    ``ema_decay`` (None, or ``d`` in [0, 1) as float32): ``self.ema``, an exponential moving average of the flat parameter bucket,
    starts as a copy of the parameters and is updated by the SAME launch that applies Adam (``ss_adam_clip_ema`` in place of
    ``ss_adam_clip``: nine streams of the bucket instead of seven), with the decay ``ema_decay_at(d, step_count, ema_warmup)`` of
    the step.  An empty shard updates it like every other rank's, so the ranks' averages stay the same bits as their parameters
    do.  ``ema_weights()`` puts the average behind the module's parameters for a block of code; ``state_dict()`` /
    ``load_state_dict()`` carry the moments, the average and the step count (``harness.fit(state_path=)``).  Without
    ``ema_decay`` a step issues exactly the launches it always has.

    ``freeze_cnn`` (an f32 ``use_roi`` model; fine-tuning a shipped checkpoint on a few clips): the ROI CNN is not trained, so its
    embeddings of the clips are constants of the run (``DeviceClipStore.embed``) and the step is ``step_embedded(Z, lengths, y)``
    on batches that already hold them (``store.batch(embedded=True)``): the ``z_ready`` forward, a backward that stops at the GRU
    input -- no ``ss_roi_cnn_*`` launch, no layer-0 d layer_in GEMM -- and the optimiser on the rest of the bucket.  ``roi_cnn`` is
    registered first, so its parameters are the leading range ``[0, n_cnn)`` of the flat bucket (``model.cnn_param_range()``, a
    multiple of 4 elements), and the existing entry points -- the zeroing, ``ss_sumsq_f32``, the all-reduce, ``ss_adam_clip`` /
    ``ss_adam_clip_ema``, ``ss_swap_f32`` -- simply run on ``[n_cnn, n)``.  Consequences: the frozen parameters and their average
    keep their exact bits (no launch ever writes them: not an update with a zero gradient, which would still move ``m``, ``v`` and
    the average); the clip norm is taken over the trainable parameters, as ``clip_grad_norm_`` sees a model whose CNN has
    ``requires_grad=False``, and ``grad_norm()`` reports that norm.  ``step`` on such a trainer raises, and so does
    ``step_embedded`` on any other: mixing the two would silently skip or apply CNN updates.  ``micro_batches`` > 1 is a
    ``ValueError``.  Class weights, the weight average, ``state_dict`` / ``load_state_dict`` and empty shards work as in ``step``.
    Without ``freeze_cnn`` a step issues exactly the launches it always has.

    ``weight_decay`` / ``param_groups`` (``model.ParamGroup``, ``model.no_decay()``): torch's decoupled AdamW with a learning-rate
    scale and a decay per parameter group -- a lower rate on the CNN, decay on the matrices but not on the biases or the LayerNorm.
    The one ``ss_adam_clip`` / ``ss_adam_clip_ema`` launch of a step becomes one ``ss_adamw_clip_groups`` launch on the same
    range with the ``SegmentTable`` of the groups (host arrays, built once); nothing else in the step changes, the clip still is
    one global norm, and with ``freeze_cnn`` the table covers ``[n_cnn, n)``.  With ``weight_decay == 0`` and no groups a step
    issues exactly the launches it always has.

    ``lr_schedule`` (``LrSchedule``) and ``lr_scale`` (an attribute: the plateau scale ``harness.fit(lr_plateau=)`` sets, 1
    otherwise): the learning rate of a step is ``lr * lr_scale * lr_schedule(step_count)`` in float64 (``current_lr()``); it is a
    per-launch scalar of either entry point, so a schedule alone changes no launch.

    ``step(teacher_logits=)`` / ``step_embedded(teacher_logits=)`` (knowledge distillation): a (B, C) float32 contiguous device
    tensor of a teacher's logits on this batch.  The loss becomes ``(1 - distill_alpha) * hard + distill_alpha *
    distill_temperature^2 * KL(softmax(t / tau) || softmax(z / tau)) / global_batch``, ``hard`` being the loss of the step
    without a teacher (smoothing, class weights, ``mix=``) over its own normaliser; the fused tail evaluates it in the launch it
    always was (``ss_tail_fwd_kd`` in place of ``ss_tail_fwd`` / ``_w`` / ``_mix``), so nothing else in the step changes.
    ``distill_alpha`` (0.5) and ``distill_temperature`` (2.0) are checked on the host (``ValueError``) and used only when
    teacher logits are given.  The teacher logits must be finite; with ``mix=`` the teacher is expected to have seen the blended
    batch.  Not with ``micro_batches`` > 1 (``ValueError``).  Without ``teacher_logits`` a step issues exactly the launches it
    always has.

    ``enable_sam(sam_rho, sam_adaptive=False)`` (a method, called once behind the constructor, whose signature is what it always
    was; ``sam_rho`` finite and > 0 as float32, checked on the host; ``harness.fit_sam`` calls it): sharpness-aware minimisation
    (Foret et al. 2021; ``sam_adaptive``: its scale-invariant form ASAM, Kwon et al. 2021), with the formulas of the widely used torch
    SAM optimiser (``adaptive=True``, no ``eta``).  On the trainable range ``[n_frozen, n)`` of the flat buckets a step then is:
    prologue, forward and backward as always (gradient ``g`` at the weights ``w``); the all-reduce of ``g``, if the trainer has one,
    so that the perturbation is that of the global batch and every rank holds the same weights in the second pass (per-rank
    perturbations, "m-sharpness", are not built); the norm ``s = sqrt(sum g^2)`` (``ss_sumsq_f32``) or ``sqrt(sum (|w| g)^2)``
    (``ss_sumsq_absw_f32``); ONE ``ss_sam_perturb`` launch: ``backup = w``, ``w += e``, ``g = 0`` with ``e = sam_rho * g / (s +
    1e-12)`` or ``sam_rho * w^2 * g / (s + 1e-12)``, which also clears the second pass's loss sum and hit count (``sam_scal``,
    ``sam_correct``: no zeroing launch between the passes); a second forward and backward at ``w + e`` on the same batch with the
    same ``engine.Loss`` (labels, smoothing, class weights and their normaliser, ``mix=``, ``teacher_logits=``) and the same
    dropout seed -- both gradients belong to the same sub-network, and the seed stays a pure function of the step count, so a
    resumed run reproduces it; the all-reduce of the new gradient ``g'``; ONE ``ss_sam_restore_sumsq`` launch in the place of
    ``ss_sumsq_f32``: ``w = backup`` bit for bit and ``sum g'^2`` for the clip; and the clip + Adam launch the trainer would use
    anyway (``ss_adam_clip``, ``_ema``, ``ss_adamw_clip_groups``) on ``(w, g')``: the weight average, groups and schedules need
    nothing new.  The step returns the loss and the hits of the FIRST pass -- the loss at the unperturbed weights, which a run
    without SAM logs; ``grad_norm()`` reports the norm of ``g'``, the one that is clipped.  An empty shard skips both passes and
    joins both all-reduces, the perturb, the restore and Adam.  Works through ``step`` and ``step_embedded`` (``freeze_cnn``: on
    ``[n_cnn, n)``) and on both engines.  On the bf16 engine the weights reach the MFMAs rounded to bf16, so a perturbation below
    bf16 resolution of a weight (``|e| < 2^-9 |w|``) vanishes in the operands: a property of the method at this precision, not a
    defect; the f32 parts (biases, LayerNorm, the head) see all of it.  Costs one more bucket-sized f32 buffer (``backup``: scratch,
    not saved) and about a second forward and backward per step.  With ``micro_batches`` > 1 ``enable_sam`` is a ``ValueError``.  ``state_dict()``
    gains ``sam_rho`` and ``sam_adaptive`` only with SAM, and ``load_state_dict`` raises ``ValueError`` when the two sides
    disagree.  Without ``enable_sam`` a step issues exactly the launches it always has.

    ``enable_lamb(exclude=None)`` (a method, like ``enable_sam``; ``harness.fit_lamb`` calls it): the layer-wise adaptive optimiser
    LAMB (You et al. 2020) for large and data-parallel batches.  The optimiser launch of every following step becomes
    ``ss_lamb_moments`` + ``ss_lamb_apply`` (include/ss_hotpath.h states the formulas) on the range the Adam launch would take
    (``[n_cnn, n)`` under ``freeze_cnn``), with the trainer's ``lr``, ``lr_scale``, ``lr_schedule``, ``weight_decay``,
    ``param_groups`` and weight average: the Adam direction plus the weight decay -- inside the update here, not decoupled -- is
    rescaled per PARAMETER TENSOR by ``|w| / |update|``, so the table of these launches has one segment per tensor
    (``model.param_tensor_segments``; more than 64 tensors: ``ValueError``).  Tensors whose name matches one of ``exclude``
    (``ParamGroup.match``'s patterns; default: what ``no_decay()`` matches, biases and LayerNorm) take the ratio 1.  The clip is
    still the one global norm.  ``trust_ratios()`` is the last step's ratio per tensor, a device tensor in the order of
    ``lamb_segments()``, the tensors' names; nothing is read back inside a step.  Combines with SAM (whose streams come first),
    ``micro_batches`` > 1, data parallelism (the gradient is all-reduced before the optimiser, so every rank computes the same
    ratios), ``step_embedded`` and both engines.  ``state_dict()`` gains ``lamb`` and ``lamb_exclude`` only with LAMB, and
    ``load_state_dict`` raises ``ValueError`` when the two sides disagree.  Without ``enable_lamb`` a step issues exactly the
    launches it always has."""

    # CUs left to the other micro-batch's recurrence while a persistent ROI-CNN kernel runs (2 directions x 8 slices)
    CNN_RESERVED_CUS = 32

    def __init__(self, model: BiGRUClassifier, lr: float = 3e-4, max_norm: float = 1.0,
                 label_smoothing: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8, world_size: int = 1,
                 process_group=None, dropout: bool = True, micro_batches: int = 1, always_allreduce: bool = False,
                 class_weights=None, ema_decay: Optional[float] = None, ema_warmup: bool = True, freeze_cnn: bool = False,
                 weight_decay: float = 0.0, param_groups=None, lr_schedule: Optional[LrSchedule] = None,
                 distill_alpha: float = 0.5, distill_temperature: float = 2.0):
        self.distill_alpha, self.distill_temperature = check_distill(distill_alpha, distill_temperature)  # (host code)
        weight_decay = float(weight_decay)
        check_weight_decay(weight_decay)
        check_lr_schedule(lr_schedule)
        # (host code: the ValueErrors of the groups come before anything touches a device)
        table = None
        if weight_decay != 0.0 or param_groups is not None:
            table = SegmentTable(model, param_groups, weight_decay, model.cnn_param_range() if freeze_cnn and model.cfg.use_roi else 0)
        if freeze_cnn:
            if not model.cfg.use_roi or model.cfg.precision != "f32":
                raise RuntimeError("freeze_cnn needs an f32 use_roi model (the bf16 engine has no frozen-CNN path)")
            if int(micro_batches) > 1:
                raise ValueError("freeze_cnn does not combine with micro_batches > 1")
        cw = None if class_weights is None else check_class_weights(class_weights, model.cfg.num_classes)
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= float(np.float32(ema_decay)) < 1.0:  # (the kernel takes it as float32)
                raise ValueError(f"ema_decay must lie in [0, 1) as float32, not {ema_decay!r}")
        if model.flat_params is None or not model.flat_params.is_cuda:
            raise RuntimeError("Trainer needs the model on a HIP device")
        L.load()
        self.model, self.lr, self.max_norm, self.ls = model, lr, max_norm, label_smoothing
        self.betas, self.eps = betas, eps
        self.world, self.group = world_size, process_group
        self.always_allreduce = always_allreduce
        # bench.py: when this is a list, every step appends a (start, end) HIP-event pair around the gradient all-reduce
        self.allreduce_events = None
        self.dropout = dropout
        dev = model.flat_params.device
        self.m = torch.zeros_like(model.flat_params)
        self.v = torch.zeros_like(model.flat_params)
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema = None if ema_decay is None else model.flat_params.detach().clone()
        self._ema_swapped = False  # inside ema_weights(): the bucket holds the average, ``ema`` the raw weights
        # [loss_sum, sumsq] fp32 and [correct] int32 live on the device
        self.scal = torch.zeros(2, device=dev, dtype=torch.float32)
        self.correct = torch.zeros(1, device=dev, dtype=torch.int32)
        # sharpness-aware minimisation: off until enable_sam(), which allocates what it needs
        self.sam_rho, self.sam_adaptive, self.backup, self.sam_scal, self.sam_correct = None, False, None, None, None
        # LAMB: off until enable_lamb(); then its table (host arrays), the partial sums, the norms and the ratios (device)
        self.lamb, self.lamb_scratch, self.lamb_norms, self.lamb_ratio = None, None, None, None
        self.param_groups = None if param_groups is None else tuple(param_groups)
        # class weights (uploaded once) and the step's normaliser, sum of w[y] over the global batch: both stay on the device
        self.cw = None if cw is None else torch.from_numpy(cw).to(dev)
        self.den = None if cw is None else torch.zeros(1, device=dev, dtype=torch.float32)
        self.freeze_cnn = bool(freeze_cnn)
        self.weight_decay, self.table, self.lr_schedule, self.lr_scale = weight_decay, table, lr_schedule, 1.0
        self.loss = None  # the last step's engine.Loss, kept ONLY to keep its tensors alive until the next (built for empty shards too)
        # the optimiser's range of the flat bucket is [n_frozen, n): everything, or everything behind the ROI CNN
        self.n_frozen = model.cnn_param_range() if freeze_cnn else 0
        self.step_count = 0
        self.rank = 0
        if world_size > 1:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized():
                self.rank = dist.get_rank(process_group)
        self._bind_bucket()
        self.micro_batches = max(1, int(micro_batches))
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(self.micro_batches)] if self.micro_batches > 1 else []
        self.ev_start = torch.cuda.Event()
        self.ev_done = [torch.cuda.Event() for _ in self.streams]

    def enable_sam(self, rho, adaptive: bool = False) -> None:
        """Switch sharpness-aware minimisation on for every following step (class docstring): ``rho`` finite and > 0 as float32,
        ``adaptive`` for ASAM.  The refusals -- a bad ``rho``, ``micro_batches`` > 1 -- are host code and come before anything
        touches a device.  Allocates, once, the bucket-sized ``backup``, the second pass's loss sum and hit count, and a third
        float behind ``[loss_sum, sumsq]`` for the first gradient's sum of squares; a second call only changes the two settings."""
        rho = check_sam_rho(rho)
        if rho is None:
            raise ValueError("sam_rho must be a number: a Trainer without enable_sam() is the one without SAM")
        if self.micro_batches > 1:
            raise ValueError("sam_rho does not combine with micro_batches > 1")
        if self.backup is None:
            flat = self.model.flat_params
            self.scal = torch.zeros(3, device=flat.device, dtype=torch.float32)
            self.backup = torch.empty_like(flat)
            self.sam_scal = torch.zeros(1, device=flat.device, dtype=torch.float32)
            self.sam_correct = torch.zeros(1, device=flat.device, dtype=torch.int32)
        self.sam_rho, self.sam_adaptive = rho, bool(adaptive)

    def enable_lamb(self, exclude=None) -> None:
        """Switch the layer-wise adaptive optimiser LAMB on for every following step (class docstring).  ``exclude``: name patterns
        with ``ParamGroup.match``'s semantics whose tensors take the trust ratio 1; None: what ``no_decay()`` matches.  The
        refusals -- bad patterns, more than 64 parameter tensors in the optimiser's range -- are host code and come before anything
        touches a device.  Allocates, once, the partial sums of the norms (``ss_lamb_scratch_bytes``), the norms and the ratios; a
        second call only changes the exclusion."""
        exclude = check_lamb_exclude(exclude)
        table = LambTable(self.model, self.param_groups, self.weight_decay, exclude, self.n_frozen)
        if self.lamb_ratio is None:
            dev, n_seg = self.model.flat_params.device, len(table.seg_end)
            size = C.c_long(0)
            L.call("ss_lamb_scratch_bytes", table.n, n_seg, C.addressof(size))
            self.lamb_scratch = torch.empty(size.value // 8, device=dev, dtype=torch.float64)
            self.lamb_norms = torch.zeros(2 * n_seg, device=dev, dtype=torch.float32)
            self.lamb_ratio = torch.ones(n_seg, device=dev, dtype=torch.float32)
        self.lamb = table

    def trust_ratios(self) -> torch.Tensor:
        """The trust ratios of the last step, one per tensor of ``lamb_segments()``: a device tensor (ones before the first step)."""
        if self.lamb is None:
            raise RuntimeError("trust_ratios() needs enable_lamb()")
        return self.lamb_ratio

    def lamb_segments(self) -> list:
        """The names of the parameter tensors LAMB rescales on their own, in the order of ``trust_ratios()``."""
        if self.lamb is None:
            raise RuntimeError("lamb_segments() needs enable_lamb()")
        return list(self.lamb.names)

    def _bind_bucket(self):
        """(Re)resolve everything that aliases the model's flat buckets.  ``model.to()/.cuda()/.float()`` keep the bucket
        when nothing moves; when they do re-allocate it (``model._bucket_version`` moves) the gradient views are taken
        again and the Adam moments follow the parameters to their device, so training carries on instead of
        accumulating into an orphaned bucket."""
        model = self.model
        flat = model.flat_params
        if self.m.device != flat.device or self.m.numel() != flat.numel():
            if self.m.numel() != flat.numel():
                raise RuntimeError("the model's parameter layout changed under the Trainer")
            self.m, self.v = self.m.to(flat.device), self.v.to(flat.device)
            if self.ema is not None:
                self.ema = self.ema.to(flat.device)
            self.scal, self.correct = self.scal.to(flat.device), self.correct.to(flat.device)
            if self.backup is not None:
                self.backup, self.sam_scal = self.backup.to(flat.device), self.sam_scal.to(flat.device)
                self.sam_correct = self.sam_correct.to(flat.device)
            if self.lamb_ratio is not None:
                self.lamb_scratch, self.lamb_norms = self.lamb_scratch.to(flat.device), self.lamb_norms.to(flat.device)
                self.lamb_ratio = self.lamb_ratio.to(flat.device)
            if self.cw is not None:
                self.cw, self.den = self.cw.to(flat.device), self.den.to(flat.device)
        self.G = model._views_of(model.flat_grads)
        model.attach_flat_grads()
        if self.n_frozen:  # never written by a frozen step and never read by its optimiser: zero, whatever was there
            model.flat_grads[:self.n_frozen].zero_()
        self._bucket_version = model._bucket_version

    def step(self, X: torch.Tensor, lengths: torch.Tensor, R: Optional[torch.Tensor], y: torch.Tensor,
             global_batch: Optional[int] = None, y_global: Optional[torch.Tensor] = None, mix=None, teacher_logits=None):
        """One optimiser step on this rank's shard.  Returns (loss, correct) device tensors:
        loss = this shard's contribution to the global mean loss (sum over ranks = global loss).
        ``global_batch`` = clips of ALL ranks in this step; needed only when the shards are unequal (``shard_range``
        with a world size that does not divide the batch): the loss is divided by it, so the summed bucket is the
        global-mean gradient whatever each rank holds.  Default: B * world_size (equal shards).
        An empty shard (``X.shape[0] == 0``; ``harness.epoch_shards`` deals them when a global batch has fewer clips than there
        are ranks) is a legal step: the bucket and the scalars are zeroed, forward and backward are skipped, and the rank joins
        the all-reduce, the clip and Adam like every other rank.  It returns zero loss and zero hits.
        ``y_global`` (class weights only): the int64 device labels of ALL ranks' clips of this step, in any one order that is the
        same on every rank; default ``y``, which is right for one process.  The loss is divided by the sum of w[label] over them
        instead of ``global_batch`` -- taken by one fixed-order launch, so every rank divides by the same bits -- and the returned
        loss is this rank's part of the global weighted mean.  Every micro-batch uses the same sum.
        ``mix`` = ``(y_b, lam)`` (a mixup batch: ``DeviceClipStore.mix[:2]``): the partners' labels (B,) int64 and the batch's factor
        (1,) f32, both on the device.  The loss is ``lam * CE(y) + (1 - lam) * CE(y_b)`` (``ss_tail_fwd_mix``), with class weights
        both terms over the one normaliser of ``y`` (``y_b`` is a permutation of it); ``correct`` counts ``argmax == y``.  Not with
        ``micro_batches`` > 1 (``ValueError``).
        ``teacher_logits`` (B, C) f32 contiguous on the device: the distillation loss of the class docstring.
        All of it reaches the engine as ONE ``engine.Loss`` (``self.loss``: it keeps its tensors alive until the next step)."""
        if self.freeze_cnn:
            raise RuntimeError("Trainer.step on a freeze_cnn trainer: it would train the ROI CNN (use step_embedded)")
        B = X.shape[0]
        y_b, lam = self._check_mix(mix, B, y) or (None, None)
        soft = self._check_teacher(teacher_logits, B)
        return self._step("step", B, lengths, y, global_batch, y_global, (y_b, lam, *soft), self._slices(B) == 1 and X.is_contiguous(),
                          self._prologue_args, self._fan_out, X, R)

    def _slices(self, B):
        """The micro-batches a batch of ``B`` clips travels in: ``micro_batches`` equal slices of at least 16 clips, or 1."""
        M = self.micro_batches
        return M if (M > 1 and B % M == 0 and B // M >= 16) else 1

    def _step(self, name, B, lengths, y, global_batch, y_global, labels_soft, may_fuse, prologue_args, fwd_bwd, *batch, prepare=None):
        """What ``step`` and ``step_embedded`` (``name``) share, behind their own refusals; nothing has been launched yet.
        ``labels_soft``: ``(y_b, lam)`` + ``_check_teacher``'s tuple, the tail of ``engine.Loss``.  ``batch``: the caller's input
        tensors; ``prepare(*batch)`` -> ``batch``, if given, is the caller's last refusal, which belongs behind the one of
        ``ema_weights()``.  The fused prologue (zero_grad, the scalars, the int32 lengths and, in ``step``, the landmark half of the
        GRU input: one launch instead of six) runs when the caller allows it (``may_fuse``) and the lengths are what it reads;
        ``prologue_args(*batch)`` are its arguments behind the lengths.  ``fwd_bwd(loss, train, seed, fused, lengths, *batch)`` is
        the caller's forward and backward."""
        model = self.model
        if self._ema_swapped:
            raise RuntimeError(f"Trainer.{name} inside ema_weights(): the parameters are the averaged ones there")
        if prepare is not None:
            batch = prepare(*batch)
        if model._bucket_version != self._bucket_version:
            self._bind_bucket()
        self.step_count += 1
        train = self.dropout and model.training
        # CE is divided by the GLOBAL clip count, so the summed bucket is the global-mean gradient
        denom = float(global_batch if global_batch is not None else B * self.world)
        # dropout streams must differ between ranks (clip b of every rank would otherwise draw the same Philox masks)
        seed = self.step_count * self.world + self.rank
        lo, grads = self.n_frozen, model.flat_grads  # (the trainable range [n_frozen, n): all of the bucket unless the CNN is frozen)
        fused = may_fuse and B > 0 and lengths.dtype == torch.int64 and lengths.is_cuda and lengths.is_contiguous()
        if fused:
            L.call("ss_train_prologue", grads.data_ptr() + 4 * lo, grads.numel() - lo, self.scal.data_ptr(), self.scal.numel(),
                   self.correct.data_ptr(), lengths.data_ptr(), *prologue_args(*batch), L.stream())
        else:
            (grads[lo:] if lo else grads).zero_()
            self.scal.zero_()
            self.correct.zero_()
        cw, den = self._weight_sum(B, y, y_global)
        self.loss = E.Loss(y, self.ls, denom, self.scal, self.correct, cw, den, *labels_soft)
        if B > 0:  # (an empty shard: this rank's gradient is the zero bucket)
            fwd_bwd(self.loss, train, seed, fused, lengths, *batch)
        if self.sam_rho is not None:
            self._sam_ascend()
            if B > 0:  # the same batch, loss description and dropout seed at w + e; its loss and hits go to scalars of their own
                fwd_bwd(dataclasses.replace(self.loss, loss_sum=self.sam_scal, correct=self.sam_correct), train, seed, fused, lengths,
                        *batch)
        self._reduce_clip_adam()
        return self.scal[0], self.correct[0]

    def _prologue_args(self, X, R):
        """``ss_train_prologue``'s arguments behind the lengths, for ``step``: the workspace's lengths, and the rows to place."""
        cfg, (B, T) = self.model.cfg, X.shape[:2]
        ws = self.model._workspace(X, R, train=True, slot=0)
        return (ws.lengths.data_ptr(), B, X.data_ptr() if cfg.use_roi else None, cfg.x_dim, L.ptr(ws.Z), cfg.in_dim, B * T, cfg.x_dim,
                L.ptr(ws.frames), cfg.roi_emb if cfg.use_roi else 0)

    def _fan_out(self, loss, train, base_seed, fused, lengths, X, R):
        """Forward and backward of ``step``: in one piece, or as ``_slices`` micro-batches on their own streams."""
        M = self._slices(X.shape[0])
        if M == 1:
            return self._fwd_bwd(X, lengths, R, loss, train, seed=base_seed, slot=0, phase="both", prologue_done=fused)
        model, cfg, y = self.model, self.model.cfg, loss.y
        n = X.shape[0] // M
        cur = torch.cuda.current_stream()
        self.ev_start.record(cur)
        L.call("ss_roi_cnn_set_max_workgroups", torch.cuda.get_device_properties(X.device).multi_processor_count - self.CNN_RESERVED_CUS)
        parts = [(X[m * n:(m + 1) * n], lengths[m * n:(m + 1) * n], None if R is None else R[m * n:(m + 1) * n],
                  y[m * n:(m + 1) * n]) for m in range(M)]
        # issue order fwd(0), fwd(1), ..., bwd(0), bwd(1), ...: the host never runs far ahead on one stream
        for phase in ("fwd", "bwd"):
            for m, (Xm, Lm, Rm, ym) in enumerate(parts):
                with torch.cuda.stream(self.streams[m]):
                    if phase == "fwd":
                        self.streams[m].wait_event(self.ev_start)
                        model._workspace(Xm, Rm, train=True, slot=m + 1).stagger = True  # the next slice waits for its CNN
                        if m > 0 and cfg.use_roi:
                            # stagger: slice m starts its ROI-CNN when slice m-1 has left it for the recurrence, so the
                            # chip-filling kernels of one slice run beside the 16-CU recurrence of the other
                            prev = model._workspace(parts[m - 1][0], parts[m - 1][2], train=True, slot=m)
                            self.streams[m].wait_event(prev.ev_cnn_fwd)
                    self._fwd_bwd(Xm, Lm, Rm, dataclasses.replace(loss, y=ym), train, seed=base_seed * M + m, slot=m + 1,
                                  phase=phase)
                    if phase == "bwd":
                        self.ev_done[m].record(self.streams[m])
        for ev in self.ev_done:
            cur.wait_event(ev)
        L.call("ss_roi_cnn_set_max_workgroups", 0)

    def _check_mix(self, mix, B, y):
        """``step(mix=)``, checked -> ``(y_b, lam)``, or None without mixup."""
        if mix is None:
            return None
        if self.micro_batches > 1:
            raise ValueError("Trainer.step(mix=) does not combine with micro_batches > 1")
        y_b, lam = mix
        if not (isinstance(y_b, torch.Tensor) and y_b.is_cuda and y_b.dtype == torch.int64 and y_b.is_contiguous()
                and y_b.shape == (B,)):
            raise ValueError("mix[0] must be a contiguous int64 device tensor of one partner label per clip")
        if not (isinstance(lam, torch.Tensor) and lam.is_cuda and lam.dtype == torch.float32 and lam.numel() == 1):
            raise ValueError("mix[1] must be a float32 device tensor of one element")
        if y.dtype != torch.int64:
            raise ValueError("Trainer.step(mix=) needs int64 labels")
        return y_b, lam

    def _check_teacher(self, teacher_logits, B):
        """``step(teacher_logits=)``, checked -> ``(t_logits, kd_alpha, kd_tau)`` for ``engine.Loss``, or ``()`` without a teacher."""
        if teacher_logits is None:
            return ()
        if self.micro_batches > 1:
            raise ValueError("teacher_logits does not combine with micro_batches > 1")
        t, C = teacher_logits, self.model.cfg.num_classes
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                and t.shape == (B, C)):
            raise ValueError(f"teacher_logits must be a contiguous float32 device tensor of shape ({B}, {C})")
        return t, self.distill_alpha, self.distill_temperature

    def _weight_sum(self, B, y, y_global):
        """Class weights: the step's normaliser, sum of w[label] over the global batch, by one launch -> ``(cw, den)`` or Nones."""
        if self.cw is not None and B > 0:
            yg = y if y_global is None else y_global
            if not yg.is_cuda or yg.dim() != 1 or yg.numel() == 0:
                raise ValueError("y_global must be a non-empty 1-D device tensor of labels")
            if yg.dtype != torch.int64 or not yg.is_contiguous():
                yg = yg.to(torch.int64).contiguous()
            # (before the micro-batch streams fork: they wait for ev_start, recorded behind this launch)
            L.call("ss_class_weight_sum", yg.data_ptr(), yg.numel(), self.cw.data_ptr(), self.model.cfg.num_classes,
                   self.den.data_ptr(), L.stream())
            return self.cw, self.den
        return None, None

    def _sam_ascend(self):
        """SAM, behind the first backward: the all-reduce of ``g``, its norm into ``scal[2]`` (zeroed with the other two), and the
        launch that saves ``w``, moves it to ``w + e``, clears ``g`` and the second pass's scalars -- on ``[n_frozen, n)``."""
        model, s, lo = self.model, L.stream(), self.n_frozen
        self._allreduce_grads()
        n_el, at = model.flat_grads.numel() - lo, 4 * lo
        w, g, norm = model.flat_params.data_ptr() + at, model.flat_grads.data_ptr() + at, self.scal.data_ptr() + 8
        if self.sam_adaptive:
            L.call("ss_sumsq_absw_f32", w, g, n_el, norm, s)
        else:
            L.call("ss_sumsq_f32", g, n_el, norm, s)
        L.call("ss_sam_perturb", w, g, self.backup.data_ptr() + at, n_el, norm, 1.0, self.sam_rho, int(self.sam_adaptive),
               self.sam_scal.data_ptr(), 1, self.sam_correct.data_ptr(), 1, s)

    def _allreduce_grads(self):
        """The all-reduce of the trainable range of the gradient bucket, if this trainer has one."""
        lo = self.n_frozen
        grads = self.model.flat_grads if lo == 0 else self.model.flat_grads[lo:]
        if self.world > 1 or self.always_allreduce:
            if self.allreduce_events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            allreduce_flat_grads(grads, self.group, always=self.always_allreduce)
            if self.allreduce_events is not None:
                e1.record()
                self.allreduce_events.append((e0, e1))

    def _reduce_clip_adam(self):
        """Behind backward: the gradient all-reduce, the global norm, clip + Adam (+ the weight average), each on elements
        ``[n_frozen, n)`` of the flat buckets -- all of them unless the ROI CNN is frozen.  SAM: the norm's launch also puts the
        weights back."""
        model, s, lo = self.model, L.stream(), self.n_frozen
        self._allreduce_grads()
        n_el, at = model.flat_grads.numel() - lo, 4 * lo
        sumsq = self.scal.data_ptr() + 4
        if self.sam_rho is None:
            L.call("ss_sumsq_f32", model.flat_grads.data_ptr() + at, n_el, sumsq, s)
        else:
            L.call("ss_sam_restore_sumsq", model.flat_params.data_ptr() + at, self.backup.data_ptr() + at,
                   model.flat_grads.data_ptr() + at, n_el, sumsq, s)
        # d_logits already carries 1/(B*world), so the summed bucket IS the global-mean gradient
        lr = self.lr if self.lr_schedule is None and self.lr_scale == 1.0 else self.current_lr()
        grouped, averaged = self.table is not None, self.ema is not None
        assert not grouped or self.table.n == n_el
        if self.lamb is not None:
            return self._lamb(n_el, at, sumsq, lr, s)
        # one pass over the range: Adam; Adam and the weight average; or AdamW with parameter groups, average or not
        entry = "ss_adamw_clip_groups" if grouped else "ss_adam_clip_ema" if averaged else "ss_adam_clip"
        ranges = [t.data_ptr() + at for t in (model.flat_params, model.flat_grads, self.m, self.v)]
        scalars = (n_el, sumsq, 1.0, self.max_norm, lr, self.betas[0], self.betas[1], self.eps, self.step_count)
        if grouped or averaged:  # these two take the average's range and the step's decay as well: NULL and 0 without an average
            ranges.append(self.ema.data_ptr() + at if averaged else None)
            scalars += (ema_decay_at(self.ema_decay, self.step_count, self.ema_warmup) if averaged else 0.0,)
        L.call(entry, *ranges, *scalars, *(self.table.args if grouped else ()), s)

    def _lamb(self, n_el, at, sumsq, lr, s):
        """LAMB in the place of the Adam launch: the moments and the per-tensor norms and ratios, then the update (and the weight
        average) -- three passes over ``[n_frozen, n)`` in two entry points, everything between them on the device."""
        model, t = self.model, self.lamb
        assert t.n == n_el
        p, g, m, v = (x.data_ptr() + at for x in (model.flat_params, model.flat_grads, self.m, self.v))
        averaged = self.ema is not None
        L.call("ss_lamb_moments", p, g, m, v, n_el, sumsq, 1.0, self.max_norm, self.betas[0], self.betas[1], self.eps, self.step_count,
               *t.args, self.lamb_scratch.data_ptr(), self.lamb_norms.data_ptr(), self.lamb_ratio.data_ptr(), s)
        L.call("ss_lamb_apply", p, m, v, self.ema.data_ptr() + at if averaged else None, n_el, self.betas[0], self.betas[1], self.eps,
               self.step_count, ema_decay_at(self.ema_decay, self.step_count, self.ema_warmup) if averaged else 0.0, lr, *t.args,
               self.lamb_ratio.data_ptr(), s)

    def current_lr(self, step: Optional[int] = None) -> float:
        """The learning rate of step ``step`` (default: the last one taken, ``step_count``): ``lr * lr_scale *
        lr_schedule(step)`` in float64; the launches take it as float32."""
        sched = 1.0 if self.lr_schedule is None else self.lr_schedule(self.step_count if step is None else step)
        return float(self.lr) * float(self.lr_scale) * sched

    def step_embedded(self, Z: torch.Tensor, lengths: torch.Tensor, y: torch.Tensor, global_batch: Optional[int] = None,
                      y_global: Optional[torch.Tensor] = None, mix=None, teacher_logits=None):
        """``step`` of a ``freeze_cnn`` trainer: ``Z`` (B, T, x_dim + roi_emb) f32 on the device already holds
        torch.cat((features, ROI embeddings)) (``store.batch(embedded=True)``).  Same returns, ``global_batch``, ``y_global`` and
        empty-shard rule and ``teacher_logits`` as ``step``; the dropout seeds are the same function of the step count, so with embeddings of the
        current CNN it is the step ``step`` takes, minus everything that belongs to the CNN (class docstring)."""
        if mix is not None:
            raise ValueError("Trainer.step_embedded(mix=): mixup of embedded batches is not built")
        if not self.freeze_cnn:
            raise RuntimeError("Trainer.step_embedded needs Trainer(freeze_cnn=True): this trainer updates the ROI CNN")
        soft = self._check_teacher(teacher_logits, Z.shape[0])
        return self._step("step_embedded", Z.shape[0], lengths, y, global_batch, y_global, (None, None, *soft), True,
                          self._prologue_args_embedded, self._fwd_bwd_embedded, Z, prepare=self._checked_Z)

    def _checked_Z(self, Z):
        """``step_embedded``'s ``Z``, tested and contiguous, as the batch of ``_step``."""
        cfg = self.model.cfg
        if Z.dim() != 3 or Z.shape[2] != cfg.in_dim or not Z.is_cuda or Z.dtype != torch.float32:
            raise RuntimeError(f"Z must be f32 (B,T,{cfg.in_dim}) on the HIP device")
        return (Z.contiguous(),)

    def _prologue_args_embedded(self, Z):
        """``ss_train_prologue``'s arguments behind the lengths for a landmark-only step: nothing to place, no frame list."""
        cfg, (B, T) = self.model.cfg, Z.shape[:2]
        return (self.model._workspace_embedded(Z, train=True).lengths.data_ptr(), B, None, cfg.x_dim, None, cfg.in_dim, B * T, cfg.x_dim,
                None, 0)

    def _fwd_bwd_embedded(self, loss, train, seed, fused, lengths, Z):
        """Forward and backward of ``step_embedded``: the ``z_ready`` forward and a backward that stops at the GRU input."""
        model, cfg = self.model, self.model.cfg
        ws = model._workspace_embedded(Z, train=True)
        P = model._param_dict()
        if not fused:
            ws.lengths.copy_(lengths.to(torch.int32), non_blocking=True)
        E.forward(P, cfg, ws, Z, None, train=train, stash=True, seed=seed, z_ready=True, ce=loss)
        E.backward(P, self.G, cfg, ws, Z, None, ws.d_logits, train=train, seed=seed, frozen_cnn=True)

    def _swap_ema(self):
        if self.model._bucket_version != self._bucket_version:
            self._bind_bucket()
        flat, lo = self.model.flat_params, self.n_frozen  # (the frozen range of the average IS the weights: nothing to exchange)
        L.call("ss_swap_f32", flat.data_ptr() + 4 * lo, self.ema.data_ptr() + 4 * lo, flat.numel() - lo, L.stream())

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the module's parameters ARE the averaged weights: one ``ss_swap_f32`` launch exchanges the flat
        bucket with ``self.ema`` in place on entry and one exchanges them back on exit (also when the block raises).  The
        parameters are views of the bucket, so no pointer changes and no workspace is rebuilt; neither engine keeps converted
        copies of the weights beyond a forward (the bf16 engine converts its GRU weights inside every forward), so there is
        nothing to invalidate.  Meanwhile ``self.ema`` holds the raw weights: ``step`` and ``state_dict`` raise inside the
        block, and so does a nested ``ema_weights()``."""
        if self.ema is None:
            raise RuntimeError("ema_weights() needs Trainer(ema_decay=)")
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest")
        self._swap_ema()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_swapped = False

    def state_dict(self) -> dict:
        """Everything a resumed run needs besides the model: copies (on the device) of the Adam moments and of the weight
        average (None without one), the step count -- the dropout seeds are a function of it -- and the hyperparameters the
        step uses.  Plain tensors, numbers and lists: ``torch.save`` writes it and ``torch.load(weights_only=True)`` reads it."""
        if self._ema_swapped:
            raise RuntimeError("Trainer.state_dict inside ema_weights(): the weights and their average are exchanged there")
        extra = {"freeze_cnn": True} if self.freeze_cnn else {}
        if self.table is not None or self.lr_schedule is not None or self.lr_scale != 1.0:  # (keys of trainers that use them only)
            extra.update(weight_decay=float(self.weight_decay), param_groups=None if self.table is None else self.table.plain(),
                         lr_schedule=None if self.lr_schedule is None else self.lr_schedule.plain(), lr_scale=float(self.lr_scale))
        if self.sam_rho is not None:  # (the backup is scratch: the weights are in the bucket whenever a state is taken)
            extra.update(sam_rho=float(self.sam_rho), sam_adaptive=bool(self.sam_adaptive))
        if self.lamb is not None:  # (the norms and ratios are each step's own: nothing of them to save)
            extra.update(lamb=True, lamb_exclude=list(self.lamb.exclude))
        return dict(m=self.m.detach().clone(), v=self.v.detach().clone(), ema=None if self.ema is None else self.ema.detach().clone(),
                    step_count=int(self.step_count), ema_decay=self.ema_decay, ema_warmup=bool(self.ema_warmup),
                    betas=[float(b) for b in self.betas], eps=float(self.eps), lr=float(self.lr), max_norm=float(self.max_norm),
                    numel=int(self.model.flat_params.numel()), **extra)

    def load_state_dict(self, state: dict) -> None:
        """Take over a ``state_dict()``: the tensors are copied into this trainer's device buffers (nothing is re-allocated), the
        step count and the hyperparameters are set.  ``ValueError`` when the bucket has another element count, when one side
        keeps a weight average and the other does not, when one side freezes the ROI CNN and the other does not, when the
        segment tables (groups, scales, decays) differ, or when the two sides disagree about ``sam_rho`` / ``sam_adaptive`` or
        about ``lamb`` / ``lamb_exclude``."""
        if self._ema_swapped:
            raise RuntimeError("Trainer.load_state_dict inside ema_weights()")
        if self.model._bucket_version != self._bucket_version:
            self._bind_bucket()
        n = self.model.flat_params.numel()
        if int(state["numel"]) != n or any(state[k].numel() != n for k in ("m", "v")):
            raise ValueError(f"the saved trainer state is for a bucket of {int(state['numel'])} elements, this model's has {n}")
        if bool(state.get("freeze_cnn", False)) != self.freeze_cnn:
            raise ValueError("the saved trainer state and this Trainer disagree about freeze_cnn: "
                             f"saved {bool(state.get('freeze_cnn', False))!r}, this one {self.freeze_cnn!r}")
        saved_table, table = state.get("param_groups"), None if self.table is None else self.table.plain()
        if saved_table != table:
            raise ValueError("the saved trainer state and this Trainer disagree about weight_decay / param_groups: "
                             f"saved table {saved_table!r}, this one {table!r}")
        saved_sam = (state.get("sam_rho"), bool(state.get("sam_adaptive", False)))
        if saved_sam != (self.sam_rho, self.sam_adaptive):
            raise ValueError("the saved trainer state and this Trainer disagree about sam_rho / sam_adaptive: "
                             f"saved {saved_sam!r}, this one {(self.sam_rho, self.sam_adaptive)!r}")
        saved_lamb = (bool(state.get("lamb", False)), None if state.get("lamb_exclude") is None else list(state["lamb_exclude"]))
        this_lamb = (self.lamb is not None, None if self.lamb is None else list(self.lamb.exclude))
        if saved_lamb != this_lamb:
            raise ValueError("the saved trainer state and this Trainer disagree about lamb / lamb_exclude: "
                             f"saved {saved_lamb!r}, this one {this_lamb!r}")
        if (state["ema"] is None) != (self.ema is None):
            raise ValueError("the saved trainer state and this Trainer disagree about ema_decay: "
                             f"saved {state['ema_decay']!r}, this one {self.ema_decay!r}")
        if self.ema is not None and state["ema"].numel() != n:
            raise ValueError("the saved weight average does not fit this model's bucket")
        self.m.copy_(state["m"].reshape(-1))
        self.v.copy_(state["v"].reshape(-1))
        if self.ema is not None:
            self.ema.copy_(state["ema"].reshape(-1))
            self.ema_decay, self.ema_warmup = float(state["ema_decay"]), bool(state["ema_warmup"])
        self.step_count = int(state["step_count"])
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        self.lr, self.max_norm = float(state["lr"]), float(state["max_norm"])
        self.lr_scale = float(state.get("lr_scale", 1.0))  # (the schedule is this trainer's own: a pure function of the step count)

    def _fwd_bwd(self, X, lengths, R, loss, train, seed, slot, phase, prologue_done=False):
        """Forward + CE ("fwd"), backward ("bwd") or both of one micro-batch on the current stream; ``loss``: its ``engine.Loss``."""
        model, cfg = self.model, self.model.cfg
        ws = model._workspace(X, R, train=True, slot=slot)
        P = model._param_dict()
        if phase in ("fwd", "both"):
            if not prologue_done:
                ws.lengths.copy_(lengths.to(torch.int32), non_blocking=True)
            E.forward(P, cfg, ws, X, R, train=train, stash=True, seed=seed, x_in_place=prologue_done, ce=loss)
        if phase in ("bwd", "both"):
            E.backward(P, self.G, cfg, ws, X, R, ws.d_logits, train=train, seed=seed)

    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the last step's (pre-clip) gradient (``freeze_cnn``: of the trainable parameters'; SAM: of the second
        pass's gradient, the one that is clipped)."""
        return self.scal[1].sqrt()
