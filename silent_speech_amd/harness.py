"""Training harness around the fused step: what ``main()`` of the reference does around its inner loop.

Counterparts, by reference line (/root/reference/train_model_official.py):
  scan_clips        :315-373   inventory of a clip directory, majority feature width, label tables, ROI decision
  split_by_label    :52-77     per-label validation split, reproducible from a seed
  class_balanced_indices :382-397   the WeightedRandomSampler draw (1 / class count, with replacement)
  evaluate          :449-475   loss / accuracy / predictions over a validation set, forward only
  top_confusions    :79-91     "actual→predicted(count)" strings of the most frequent errors
  fit               :417-506   epochs, save-best checkpoint (:486-500), early stopping (:501-505)
  fit_calibrated    (none)     ``fit``, then a softmax temperature fitted on the validation clips and stored in the checkpoint
  balanced_class_weights :406-412   the weights of the commented-out class-weighted loss (``fit(class_weights="balanced")``)

Data parallelism (the reference has none): ``fit(rank=, world_size=, process_group=)`` -- every rank holds
the whole store and draws the whole epoch order, ``epoch_shards`` gives it its rows of every global batch, the validation
state stays on the device (``evaluate_device``: ``ss_eval_accum``) in a form that ``reduce_epoch_metrics`` reduces with two
collectives per epoch, and ``top_confusions_from_matrix`` prints from the reduced matrices what ``top_confusions`` prints
from the lists.

The clips live in a ``DeviceClipStore`` (uploaded once), batches are assembled on the device, the step is
``Trainer.step``; nothing here touches the arithmetic of the hot path.  ``fit(plan="device")`` also draws the sample
order and plans every batch on the device (``sample_epoch``, ``batch(rng="philox")``): an epoch is enqueue-only.
"""
from __future__ import annotations

import collections
import contextlib
import copy
import dataclasses
import glob
import hashlib
import inspect
import os
import random
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .checkpoint import (TRAIN_STATE_FORMAT, add_calibration, fingerprint_difference, load_classifier, load_train_state,
                         save_checkpoint, save_train_state)
from .device_data import MASK_FIELDS, MIXUP_FIELDS, AugmentPolicy, DeviceClipStore
from .model import BiGRUClassifier, ParamGroup
from .train import (PlateauSchedule, Trainer, check_class_weights, check_distill, check_lamb_exclude, check_lr_schedule, check_sam_rho,
                    check_weight_decay, shard_range)

VAL_FRAC, SEED, PATIENCE, EPOCHS, BATCH_SIZE = 0.15, 42, 12, 80, 16
I32_MAX = 2 ** 31 - 1  # "no clip yet" in a first_seen matrix


def scan_clips(clip_dir: str):
    """-> dict(files, labels, x_dim, uniq, label_to_id, id_to_label, has_roi).  Clips whose feature width is not the most
    common one are left out, as the reference does (:347-358)."""
    files = sorted(glob.glob(os.path.join(clip_dir, "*.npz")))
    if not files:
        raise RuntimeError(f"No .npz files found in {clip_dir}")
    labels, dims, has_roi = [], [], 0
    for f in files:
        d = np.load(f, allow_pickle=True)
        labels.append(str(d["label"]))
        dims.append(int(d["X"].shape[1]))
        has_roi += int("roi" in d.files)
    x_dim = collections.Counter(dims).most_common(1)[0][0]
    keep = [k for k, dm in enumerate(dims) if dm == x_dim]
    files, labels = [files[k] for k in keep], [labels[k] for k in keep]
    uniq = sorted(set(labels))
    label_to_id = {lab: i for i, lab in enumerate(uniq)}
    return dict(files=files, labels=labels, x_dim=x_dim, uniq=uniq, label_to_id=label_to_id,
                id_to_label={i: lab for lab, i in label_to_id.items()}, has_roi=has_roi)


def split_by_label(files: Sequence[str], labels: Sequence[str], val_frac: float = VAL_FRAC, seed: int = SEED,
                   verbose: bool = False) -> Tuple[List[str], List[str]]:
    """Every label gives ``round(n * val_frac)`` clips (at least 1, at most n-1) to validation; one ``random.Random(seed)``
    drives, in this order, the shuffle inside each label (labels in first-seen order) and the two final shuffles."""
    rng = random.Random(seed)
    groups: Dict[str, List[str]] = {}
    for f, lab in zip(files, labels):
        groups.setdefault(lab, []).append(f)
    train: List[str] = []
    val: List[str] = []
    for lab, members in groups.items():
        rng.shuffle(members)
        n = len(members)
        n_val = min(max(1, int(round(n * val_frac))), n - 1)
        val += members[:n_val]
        train += members[n_val:]
        if verbose:
            print(f"{lab:>10}: total={n:4d}  train={n - n_val:4d}  val={n_val:4d}")
    rng.shuffle(train)
    rng.shuffle(val)
    return train, val


def top_confusions(y_true: Sequence[int], y_pred: Sequence[int], id_to_label: Dict[int, str], k: int = 8) -> List[str]:
    wrong = collections.Counter((t, p) for t, p in zip(y_true, y_pred) if t != p)
    return [f"{id_to_label[t]}→{id_to_label[p]}({n})" for (t, p), n in wrong.most_common(k)]


def class_balanced_indices(labels: Sequence[str], num_samples: Optional[int] = None,
                           generator: Optional[torch.Generator] = None) -> List[int]:
    """One epoch of the reference's WeightedRandomSampler: weight 1 / count(label), drawn with replacement."""
    counts = collections.Counter(labels)
    w = torch.tensor([1.0 / counts[lab] for lab in labels], dtype=torch.double)
    n = len(labels) if num_samples is None else num_samples
    return torch.multinomial(w, n, replacement=True, generator=generator).tolist()


def balanced_class_weights(train_labels: Sequence[str], id_to_label: Dict[int, str]) -> np.ndarray:
    """The class weights of the reference's commented-out loss (:407-412): float32 ``1 / count(label of class i)`` over the
    training clips, divided by its mean -- the average weight is 1."""
    counts = collections.Counter(train_labels)
    w = torch.tensor([1.0 / counts[id_to_label[i]] for i in range(len(id_to_label))], dtype=torch.float32)
    w = w / w.mean()
    return w.numpy()


@torch.no_grad()
def evaluate(model: BiGRUClassifier, store: DeviceClipStore, batch_size: int = BATCH_SIZE, label_smoothing: float = 0.05,
             plan: str = "host", class_weights=None):
    """-> (mean loss, accuracy, y_true, y_pred) over every clip of ``store``, in order, eval mode, no augmentation.
    ``plan="device"``: the batches are planned by the kernel (``store.batch(rng="philox")``) -- the same batches, since
    nothing is drawn without augmentation.
    ``class_weights`` (one finite positive number per class): the loss is that of ``CrossEntropyLoss(weight=, label_smoothing=)``
    over the WHOLE store, sum of the per-clip weighted losses / sum of w[label].  On purpose not the reference's average of
    per-batch means (:441 and its validation loop): that figure depends on how the store is cut into batches, and so on
    ``batch_size`` and, data parallel, on the world size; this one does not."""
    if plan not in ("host", "device"):
        raise ValueError(f"plan must be 'host' or 'device', not {plan!r}")
    cw = None if class_weights is None else check_class_weights(class_weights, model.cfg.num_classes)
    from . import _lib as L
    from .checkpoint import softmax_topk

    was_training = model.training
    model.eval()
    y_true, y_pred = [], []
    dev = model.flat_params.device
    loss_sum = torch.zeros(1, device=dev, dtype=torch.float32)   # sum of the per-clip losses (denom = 1)
    correct = torch.zeros(1, device=dev, dtype=torch.int32)
    every = torch.arange(len(store), dtype=torch.int32, device=store.device) if plan == "device" else None
    cw_d = one = None
    if cw is not None:
        cw_d, one = torch.from_numpy(cw).to(dev), torch.ones(1, device=dev, dtype=torch.float32)
    for lo in range(0, len(store), batch_size):
        if plan == "device":
            X, T, R, y = store.batch(every[lo:lo + batch_size], augment=False, rng="philox")
        else:
            idx = list(range(lo, min(len(store), lo + batch_size)))
            X, T, R, y = store.batch(idx, augment=False)
        logits = model(X, T, R if model.use_roi else None).contiguous()
        y = y.to(torch.int64).contiguous()
        # loss and hit count by the path's own cross-entropy kernel, predictions by its top-k kernel (no aten op)
        # (weighted: normaliser 1, the sum of the weighted per-clip losses)
        name, norm = _weighted_entry(cw_d, ("ss_ce_ls_fwd_bwd", (1.0,)), ("ss_ce_ls_w_fwd_bwd", (L.ptr(cw_d), L.ptr(one))))
        L.call(name, logits.data_ptr(), y.data_ptr(), logits.shape[0], logits.shape[1], label_smoothing, *norm, None,
               loss_sum.data_ptr(), correct.data_ptr(), L.stream())
        _, top = softmax_topk(logits, 1)
        y_true += y.cpu().tolist()
        y_pred += top[:, 0].cpu().tolist()
    model.train(was_training)
    model.check_health()  # the loop above has synchronised anyway
    n = max(1, len(store))
    if cw is not None:  # the labels are on the host already: their weights are summed there, in float64
        wsum = float(cw.astype(np.float64)[np.asarray(y_true, np.int64)].sum()) if y_true else 1.0
        return float(loss_sum) / wsum, int(correct) / n, y_true, y_pred
    return float(loss_sum) / n, int(correct) / n, y_true, y_pred


def _weighted_entry(cw_d, plain, weighted):
    """``plain`` or ``weighted``, each (entry point, the arguments in which the pair differs): the weighted one under class weights."""
    return plain if cw_d is None else weighted


def top_confusions_from_matrix(confusion, first_seen, id_to_label: Dict[int, str], k: int = 8) -> List[str]:
    """``top_confusions`` from the (C, C) ``[true][pred]`` counts and the position at which every cell first occurred: the
    off-diagonal cells by count descending, ties by first occurrence -- the order of ``Counter.most_common``."""
    confusion, first_seen = np.asarray(confusion), np.asarray(first_seen)
    cells = [(-int(confusion[t, p]), int(first_seen[t, p]), t, p) for t, p in zip(*np.nonzero(confusion)) if t != p]
    return [f"{id_to_label[int(t)]}→{id_to_label[int(p)]}({-n})" for n, _, t, p in sorted(cells)[:k]]


def epoch_shards(n_draws: int, batch_size: int, rank: int = 0, world_size: int = 1) -> Iterator[Tuple[int, int, int, int]]:
    """The steps of one epoch of ``n_draws`` rows for rank ``rank``: -> ``(lo, hi, first_row, global_batch)`` per step.  The
    global batches are ``[g, min(n_draws, g + batch_size))`` (``batch_size`` is the GLOBAL batch), of which the rank takes the
    ``shard_range`` rows ``[lo, hi)`` of the epoch order; ``first_row`` = position in the epoch of row ``lo`` (what
    ``store.batch(first_row=)`` wants, added to the rows of the epochs before), ``global_batch`` = rows of all ranks in the
    step (``Trainer.step(global_batch=)``).  ``hi == lo`` is a legal empty shard: the rank still takes the step, since the
    gradient all-reduce is collective.  Every rank takes the same number of steps."""
    if batch_size <= 0 or world_size <= 0 or not 0 <= rank < world_size:
        raise ValueError("epoch_shards: batch_size and world_size must be positive and rank inside [0, world_size)")
    for g in range(0, n_draws, batch_size):
        n = min(n_draws, g + batch_size) - g
        lo, hi = shard_range(n, rank, world_size)
        yield g + lo, g + hi, g + lo, n


def reduce_epoch_metrics(sums: torch.Tensor, confusion: torch.Tensor, first_seen: torch.Tensor, process_group=None) -> None:
    """Reduce an epoch's metrics over the ranks, in place, on whatever device the tensors are on: ``sums`` (any 1-D float64
    vector of things that add: loss sums, hit counts, clip counts, flags) and ``confusion`` (C, C) by SUM in ONE collective
    (the counts ride in the float64 vector: exact below 2^53), ``first_seen`` (C, C) by MIN in a second one.  Two
    collectives per epoch besides the per-step gradient all-reduce.  Without a group: nothing to do; a one-rank group still
    issues both (sums over one rank: the identity), like ``Trainer(always_allreduce=True)``."""
    if process_group is None:
        return
    import torch.distributed as dist

    if sums.dtype != torch.float64 or sums.dim() != 1:
        raise ValueError("sums must be a 1-D float64 tensor")
    packed = torch.cat([sums, confusion.reshape(-1).to(torch.float64)])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=process_group)
    dist.all_reduce(first_seen, op=dist.ReduceOp.MIN, group=process_group)
    sums.copy_(packed[:sums.numel()])
    confusion.copy_(packed[sums.numel():].reshape(confusion.shape))  # (float64 -> the matrix's integer type: exact)


@dataclasses.dataclass
class EvalResult:
    """What ``evaluate_device`` returns.  ``loss``, ``acc``, ``n``, ``confusion`` and ``first_seen`` are those of the whole
    store (reduced over the ranks); ``y_true`` / ``y_pred`` are device int32 tensors of THIS rank's shard, in store order."""
    loss: float
    acc: float
    n: int
    confusion: np.ndarray   # (C, C) int64, [true][pred], hits included
    first_seen: np.ndarray  # (C, C) int64, index in the store of the first clip of the cell; I32_MAX: none
    y_true: torch.Tensor
    y_pred: torch.Tensor
    bad_labels: bool = False  # a label outside the model's classes (always False on a result that was returned)
    extra: Optional[np.ndarray] = None  # the reduced ``extra_sums`` of the call, if any
    loss_sum: float = 0.0     # numerator of ``loss``: the sum of the per-clip (weighted) losses
    weight_sum: float = 0.0   # its denominator: ``n``, or under class weights the sum of w[label]


@torch.no_grad()
def evaluate_device(model: BiGRUClassifier, store: DeviceClipStore, batch_size: int = BATCH_SIZE, label_smoothing: float = 0.05,
                    rank: int = 0, world_size: int = 1, process_group=None,
                    extra_sums: Optional[torch.Tensor] = None, class_weights=None, embedded: bool = False) -> EvalResult:
    """``evaluate`` with the validation state kept on the device.  The rank evaluates the clips
    ``shard_range(len(store), rank, world_size)`` of the store, in order, eval mode, no augmentation: batches planned by
    ``store.batch(rng="philox")``, one ``ss_eval_accum`` launch per batch (``first_row`` = the clip's index in the store),
    nothing read back inside the loop.  Then ``reduce_epoch_metrics`` (two collectives when there is a group) and ONE host
    read of everything.  ``extra_sums`` (device float32 / float64 values that add over ranks, e.g. the epoch's train loss sum
    and hit count) ride in the same reduction and the same read: ``EvalResult.extra``.
    The kernel's bad-label flag travels in the same sum and the same read; if any rank saw a label outside the model's classes
    (such clips count nowhere) every rank raises ``ValueError`` here, the way ``store.check()`` raises for the store's flag.
    ``class_weights`` (one finite positive number per class): ``ss_eval_accum_w`` keeps two sums, the per-clip weighted losses
    and w[label]; both add over ranks (the second rides in the same ``sums`` vector: no new collective) and ``loss`` is their
    quotient over the whole store -- ``EvalResult.loss_sum / weight_sum``.  As in ``evaluate`` this is not the reference's
    average of per-batch means, which would change with the batch size and the world size.
    ``embedded`` (after ``store.embed(model)``; a frozen ROI CNN): the batches are ``store.batch(embedded=True)`` and the logits
    come from ``model.forward_embedded`` -- the ``z_ready`` forward, no CNN launch; the same logits while the embeddings are those
    of the model's CNN (``store.check()`` tells)."""
    from . import _lib as L

    cw = None if class_weights is None else check_class_weights(class_weights, model.cfg.num_classes)
    C, dev = model.cfg.num_classes, model.flat_params.device
    lo, hi = shard_range(len(store), rank, world_size)
    loss_sum = torch.zeros(1, device=dev, dtype=torch.float32)
    cw_d = wsum = None
    if cw is not None:
        cw_d, wsum = torch.from_numpy(cw).to(dev), torch.zeros(1, device=dev, dtype=torch.float32)
    counts = torch.zeros(2, device=dev, dtype=torch.int32)  # [correct, bad-label flag]
    confusion = torch.zeros(C, C, device=dev, dtype=torch.int32)
    first_seen = torch.full((C, C), I32_MAX, device=dev, dtype=torch.int32)
    y_true = torch.empty(hi - lo, device=dev, dtype=torch.int32)
    y_pred = torch.empty(hi - lo, device=dev, dtype=torch.int32)
    every = torch.arange(len(store), dtype=torch.int32, device=store.device)
    was_training = model.training
    model.eval()
    for b0 in range(lo, hi, batch_size):
        b1 = min(hi, b0 + batch_size)
        if embedded:
            Z, T, _, y = store.batch(every[b0:b1], augment=False, rng="philox", embedded=True)
            logits = model.forward_embedded(Z, T).contiguous()
        else:
            X, T, R, y = store.batch(every[b0:b1], augment=False, rng="philox")
            logits = model(X, T, R if model.use_roi else None).contiguous()
        name, sums = _weighted_entry(cw_d, ("ss_eval_accum", (loss_sum.data_ptr(),)),
                                     ("ss_eval_accum_w", (L.ptr(cw_d), loss_sum.data_ptr(), L.ptr(wsum))))
        L.call(name, logits.data_ptr(), y.data_ptr(), b1 - b0, C, label_smoothing, b0, *sums, counts.data_ptr(), confusion.data_ptr(),
               first_seen.data_ptr(), y_true.data_ptr() + 4 * (b0 - lo), y_pred.data_ptr() + 4 * (b0 - lo), counts.data_ptr() + 4,
               L.stream())
    model.train(was_training)
    n_extra = 0 if extra_sums is None else extra_sums.numel()
    # [loss sum, correct, bad-label flag, n] + extra_sums (+ under class weights, last: the sum of w[label])
    sums = torch.cat([loss_sum.double(), counts.double(), torch.full((1,), float(hi - lo), device=dev, dtype=torch.float64)]
                     + ([extra_sums.reshape(-1).to(device=dev, dtype=torch.float64)] if n_extra else [])
                     + ([wsum.double()] if cw is not None else []))
    reduce_epoch_metrics(sums, confusion, first_seen, process_group)
    host = torch.cat([sums, confusion.reshape(-1).double(), first_seen.reshape(-1).double()]).cpu().numpy()  # the one read
    model.check_health()  # (the read above has synchronised)
    tot_loss, correct, bad, n = float(host[0]), int(host[1]), int(host[2]), int(host[3])
    if bad:
        raise ValueError("evaluate_device: a label of the store is outside the model's %d classes" % C)
    n_sums = sums.numel()
    mats = host[n_sums:].astype(np.int64)
    weight_sum = float(host[n_sums - 1]) if cw is not None else float(n)
    return EvalResult(loss=tot_loss / (weight_sum if weight_sum > 0 else 1.0), acc=correct / max(1, n), n=n,
                      confusion=mats[:C * C].reshape(C, C), first_seen=mats[C * C:].reshape(C, C), y_true=y_true, y_pred=y_pred,
                      extra=host[4:4 + n_extra].copy() if n_extra else None, loss_sum=tot_loss, weight_sum=weight_sum)


def run_fingerprint(seed, batch_size, world_size, max_t, lr, labels, x_dim, use_roi, n_train, n_val, class_weights,
                    augment_policy, ema_decay, init_from=None, freeze_cnn=False, weight_decay=0.0, param_groups=None,
                    lr_schedule=None, lr_plateau=None, distill_from=None, distill_alpha=0.5, distill_temperature=2.0) -> dict:
    """What a resumable ``fit`` run depends on, as plain values (``checkpoint.FINGERPRINT_FIELDS``): a train-state file is
    resumed only by a call whose fingerprint equals the saved one.  ``epochs`` and ``patience`` are not part of it: a run may be
    resumed to train longer.  ``init_from`` (the sha256 of the checkpoint file the run started from, a hex string) and
    ``freeze_cnn`` are entries only when they are set: the fingerprint of a run without them is what it always was.  The same holds
    for the policy's mask fields (``AugmentPolicy.mask_fields``): each is an entry only where it differs from its default; and for
    its two mixup fields (``AugmentPolicy.mixup_fields``), which are entries only when mixup is on; and for ``weight_decay`` (when
    not 0), ``param_groups`` (the groups as written: patterns, scale, decay), ``lr_schedule`` (as written: a ``total_steps`` that
    ``fit`` fills in from ``epochs`` stays None, since ``epochs`` is no part of the fingerprint) and ``lr_plateau`` (its settings; its
    state travels in the train-state file); and for ``distill_from`` (the sha256 of the teacher's checkpoint file, or ``"module"``
    for a teacher handed over as a module), ``distill_alpha`` and ``distill_temperature``, all three entries only when
    ``distill_from`` is set.  (A ``fit_sam`` run adds ``sam_rho`` and ``sam_adaptive`` to what this returns: ``sam_fingerprint``.)"""
    extra = {}
    if float(weight_decay) != 0.0:
        extra["weight_decay"] = float(weight_decay)
    if param_groups is not None:
        extra["param_groups"] = [dict(match=list(g.match), lr_scale=g.lr_scale, weight_decay=g.weight_decay) for g in param_groups]
    if lr_schedule is not None:
        extra["lr_schedule"] = lr_schedule.plain()
    if lr_plateau is not None:
        extra["lr_plateau"] = lr_plateau.plain()
    if init_from is not None:
        extra["init_from"] = str(init_from)
    if freeze_cnn:
        extra["freeze_cnn"] = True
    if distill_from is not None:
        extra.update(distill_from=str(distill_from), distill_alpha=float(distill_alpha),
                     distill_temperature=float(distill_temperature))
    return dict(seed=int(seed), batch_size=int(batch_size), world_size=int(world_size), max_t=int(max_t), lr=float(lr),
                labels=[str(lab) for lab in labels], x_dim=int(x_dim), use_roi=bool(use_roi), n_train=int(n_train),
                n_val=int(n_val), class_weights=None if class_weights is None else [float(w) for w in class_weights],
                augment_policy=None if augment_policy is None else {
                    **{k: (list(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(augment_policy).items()
                       if k not in MASK_FIELDS + MIXUP_FIELDS}, **augment_policy.mask_fields(), **augment_policy.mixup_fields()},
                ema_decay=None if ema_decay is None else float(ema_decay), **extra)


def file_sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def load_init_checkpoint(path: str, x_dim: int, use_roi: bool, roi_emb: int, hidden: int) -> dict:
    """The checkpoint ``fit(init_from=)`` starts from (reference schema, read as ``load_classifier`` reads it), checked against the
    scanned clips: ``ValueError`` naming the first of ``x_dim``, ``use_roi``, ``roi_emb``, ``hidden`` that does not match.
    -> the checkpoint dict.  Host code only."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["model"]
    have = dict(x_dim=int(ckpt["x_dim"]), use_roi=bool(ckpt.get("use_roi", False)),
                roi_emb=int(sd["roi_cnn.fc.weight"].shape[0]) if "roi_cnn.fc.weight" in sd else roi_emb,
                hidden=int(sd["gru.weight_hh_l0"].shape[1]))
    want = dict(x_dim=int(x_dim), use_roi=bool(use_roi), roi_emb=int(roi_emb), hidden=int(hidden))
    for field in ("x_dim", "use_roi", "roi_emb", "hidden"):
        if have[field] != want[field]:
            raise ValueError(f"init_from {path}: {field} is {have[field]!r}, the clips need {want[field]!r}")
    return ckpt


def check_teacher(x_dim: int, use_roi: bool, num_classes: int, labels, clip_x_dim: int, run_use_roi: bool, clip_labels) -> None:
    """A distillation teacher against the run: ``ValueError`` naming ``x_dim``, ``use_roi`` or the labels -- a checkpoint teacher's
    list must be the clips', in content and order; a module teacher has none (``labels=None``) and its ``num_classes`` must be
    their count.  Host code."""
    if int(x_dim) != int(clip_x_dim):
        raise ValueError(f"distill_from: the teacher's x_dim is {int(x_dim)}, the clips' is {int(clip_x_dim)}")
    if bool(use_roi) != bool(run_use_roi):
        raise ValueError(f"distill_from: the teacher's use_roi is {bool(use_roi)}, the run's is {bool(run_use_roi)}")
    if labels is not None and list(labels) != list(clip_labels):
        raise ValueError(f"distill_from: the teacher's labels {list(labels)!r} differ from the clips' labels {list(clip_labels)!r} "
                         "(content and order must match)")
    if int(num_classes) != len(clip_labels):
        raise ValueError(f"distill_from: the teacher's num_classes is {int(num_classes)}, the clips have {len(clip_labels)} labels")


def _barrier(process_group) -> None:
    if process_group is not None:
        import torch.distributed as dist

        dist.barrier(group=process_group)


def fit(clip_dir: str, out_path: str, epochs: int = EPOCHS, batch_size: int = BATCH_SIZE, patience: int = PATIENCE,
        max_t: int = 90, lr: float = 3e-4, seed: int = SEED, use_roi_if_present: bool = True, device="cuda",
        log=print, plan: str = "host", rank: int = 0, world_size: int = 1, process_group=None,
        history: Optional[list] = None, class_weights=None, augment_policy=None, ema_decay: Optional[float] = None,
        state_path: Optional[str] = None, resume: bool = False, init_from: Optional[str] = None,
        freeze_cnn: bool = False, weight_decay: float = 0.0, param_groups=None, lr_schedule=None, lr_plateau=None,
        distill_from=None, distill_alpha: float = 0.5, distill_temperature: float = 2.0) -> float:
    """The reference's ``main()``: scan, split, train with class-balanced sampling and on-device augmentation, evaluate
    every epoch, keep the best checkpoint (reference schema), stop after ``patience`` epochs without improvement.

    ``plan="host"``: the sample order is a ``torch.multinomial`` on the CPU and every batch is planned in Python
    (``store.batch(rng="device")``).  ``plan="device"``: an epoch is enqueue-only -- one ``store.sample_epoch`` launch draws
    the order, every batch (validation too) is planned by ``ss_batch_plan``; draw ``epoch_base + lo`` belongs to row ``lo`` of
    the epoch (``epoch_base`` = clips drawn in the epochs before), so no two rows of a run share draws.  Validation is
    ``evaluate_device``: the epoch ends in one host read (the train scalars ride in it) and the store's out-of-range flag is
    read once per epoch.

    Data parallel (``world_size`` > 1 or a ``process_group``; needs ``plan="device"``): one process per GPU calls ``fit`` with
    its ``rank``.  Every rank holds the whole store and draws the whole epoch order (same seed, same ``first``), walks
    ``epoch_shards`` -- ``batch_size`` is the GLOBAL batch -- and trains on its rows of every global batch, which together
    are the batch a single process would have drawn, clip for clip and draw for draw.  Parameters are broadcast from rank 0
    before the first step, the gradients are summed per step (``Trainer``), the epoch's scalars and confusion matrices per
    epoch (``reduce_epoch_metrics``); every rank then holds the same metrics and takes the same save / early-stop decisions
    without another exchange.  Rank 0 alone logs and writes the checkpoint; all ranks pass a barrier before ``fit``
    returns, and all return ``best``.  (Verified on one rank over RCCL and on two over gloo; more than one GPU is unmeasured.)

    ``history``: a list that gets one ``dict(epoch, train_loss, train_acc, val_loss, val_acc)`` per epoch, unrounded.

    ``class_weights``: None (the reference's live loss, :405), ``"balanced"`` (``balanced_class_weights`` of the training clips:
    the reference's commented-out loss, :406-414) or one finite positive number per class.  Training and validation then use
    ``CrossEntropyLoss(weight=, label_smoothing=0.05)``.  In the device-planned loop every rank passes the labels of the step's
    whole global batch to ``Trainer.step(y_global=)`` -- gathered once per epoch from the store's device label table by the
    epoch order, nothing read back -- so the weighted mean is that of the global batch whatever the world size.  The logged
    train loss stays the sum of loss x batch over the clip count, as the reference logs it (:441); the validation loss is
    the weighted mean over the whole validation set (``evaluate``).

    ``augment_policy``: an ``AugmentPolicy`` for the training batches (time warp, scale jitter, ROI shift, and the masks: time
    mask, feature band, ROI cutout; all planned on the device); needs ``plan="device"``.  Validation batches are never augmented.  None: the reference's two augmentations only.
    With ``mixup_prob`` > 0 every training batch is planned with mixup (``store.mix`` goes to ``Trainer.step(mix=)``; the logged train
    accuracy counts ``argmax == y``, the rows' own labels, as inactive/train_reduced.py logs it) and validation is never mixed.  The
    plan is a pure function of (seed, the batch's first row), so a resumed run draws the partners and factors of the uninterrupted
    one.  Mixup with ``world_size`` > 1 or a ``process_group`` is a ``ValueError``: a row's partner may lie in another rank's shard,
    and exchanging partners across ranks is a later piece of work.  So is mixup with ``freeze_cnn`` (embedded batches are not mixed).

    ``ema_decay`` (``d`` in [0, 1); the reference has no averaged model): ``Trainer(ema_decay=d)`` keeps an exponential moving
    average of the weights inside the Adam launch.  Every epoch's validation, under both plans, runs on the AVERAGED weights
    (``trainer.ema_weights()``), the checkpoint written on improvement holds them -- in the reference schema, so
    ``load_classifier`` and the reference's live script read it unchanged -- and early stopping follows their accuracy.  The
    train loss and accuracy stay those of the raw weights, which are what the steps run on.

    ``state_path`` (needs ``plan="device"``, where an epoch is a pure function of (seed, draw index) and the dropout seeds one
    of the step count): after every epoch rank 0 writes one train-state file there, atomically (``save_train_state``): the raw
    ``model.state_dict()``, ``trainer.state_dict()``, the epoch just finished, ``best``, ``bad``, whether the run has stopped
    early, and ``run_fingerprint``.  ``resume=True`` with such a file: every rank loads it, a fingerprint that differs from this
    call's raises ``ValueError`` naming the first differing field, model, trainer, ``best`` and ``bad`` are restored and the run
    continues at the next epoch -- up to the order of the float atomics it is the uninterrupted run.  A saved run that had
    reached ``epochs`` or had stopped early returns ``best`` without training.  ``resume=True`` without a file starts fresh.
    ``history`` gets only the epochs this call ran.

    ``init_from`` (the reference trains from scratch only): a checkpoint in the reference schema, loaded as ``load_classifier``
    reads it, to start from -- adapting a shipped model to a new speaker or word list.  Its ``x_dim``, ``use_roi``, ``roi_emb``
    and ``hidden`` must match the scanned clips (``ValueError`` naming the field).  Every tensor is copied; if the label list
    differs, ``head.4.weight`` and ``head.4.bias`` keep their fresh initialisation, which is logged.  Data parallel, the broadcast
    from rank 0 follows the load.

    ``freeze_cnn`` (needs ``plan="device"``, clips with ROI frames and ``init_from``: a frozen random CNN is a mistake): the ROI
    CNN is not trained.  Both stores run it over their frames once (``store.embed(model)``), the training batches are
    ``batch(embedded=True)`` into ``Trainer.step_embedded`` and validation is ``evaluate_device(embedded=True)``: no step and no
    validation batch launches the CNN or moves a pixel.  ``store.check()`` (once per epoch) also verifies that the CNN still is
    the one the embeddings were made with.  The checkpoint written is the full model in the reference schema.  ``ROI shift`` in
    an ``augment_policy`` is refused (it acts on pixels).

    ``state_path``: the fingerprint holds ``init_from`` (the file's sha256) and ``freeze_cnn`` only when they are set, so the
    files of runs without them are unchanged.

    ``weight_decay``, ``param_groups`` (``ParamGroup``, ``no_decay()``): AdamW with per-group learning-rate scales and decays
    (``Trainer``): inactive/train_model_1130pm.py:191 trains with ``AdamW(weight_decay=1e-3)``.  ``lr_schedule`` (``LrSchedule``): a
    warm-up and a linear or cosine decay by the step count; a ``total_steps=None`` becomes ``epochs`` x the batches of an epoch.
    ``lr_plateau`` (``PlateauSchedule``; ``fit`` works on a copy that starts fresh): stepped once per epoch behind the validation,
    on its accuracy (mode "max", as inactive/train_reduced.py:199,242 steps ``ReduceLROnPlateau``) or its loss (mode "min"); the
    scale it arrives at multiplies the learning rate of the following epochs.  Data parallel, every rank holds the same reduced
    metrics and takes the same decision; rank 0 logs a reduction.  The learning rate of a step is ``lr * plateau scale *
    lr_schedule(step count)``.  With a schedule or a plateau the ``history`` dicts gain ``lr``, the rate of the epoch's last step.
    ``state_path``: the train-state file carries the plateau's state (best, bad count, scale) and the fingerprint these four
    settings, each only when it is set: files and fingerprints of runs without them are unchanged.

    ``distill_from`` (knowledge distillation; needs ``plan="device"``; the reference has no teacher): a checkpoint path, read by
    ``load_classifier``, or a ``BiGRUClassifier`` already on the device -- any width, depth or precision, which is how a large
    bf16 model teaches the shipped one.  The teacher is put in ``eval()`` and is never trained, saved or averaged.  Every
    training step runs ``teacher(X, T, R)`` under ``no_grad`` on the batch the student sees (augmented and mixed included) and
    hands its logits to ``Trainer.step(teacher_logits=)`` with ``distill_alpha`` and ``distill_temperature`` (``Trainer``):
    enqueue-only, nothing is read back.  Its ``x_dim`` and ``use_roi`` must be the run's and a checkpoint teacher's label list the
    clips', in content and order (``ValueError`` naming the field).  Not with ``freeze_cnn`` (embedded batches hold no pixels for
    the teacher).  Data parallel, every rank holds the teacher and runs it on its own shard: no collective is added.  Validation,
    the checkpoint, the weight average, the schedules and the logged train accuracy are as without; the logged train loss is the
    blended one.  ``state_path``: the fingerprint holds ``distill_from`` (the file's sha256, or ``"module"``), ``distill_alpha`` and
    ``distill_temperature`` only when ``distill_from`` is set; a resumed run must be given the same teacher.

    ``fit_sam(clip_dir, out_path, sam_rho, sam_adaptive=False, **fit_args)`` is this function with sharpness-aware minimisation
    (SAM, or its scale-invariant form ASAM) in every training step; this signature is what it always was.

    ``fit_lamb(clip_dir, out_path, lamb_exclude=None, **fit_args)`` is this function with the layer-wise adaptive optimiser LAMB in
    every training step; this signature is what it always was."""
    return _fit(None, False, **locals())


def sam_fingerprint(fingerprint: dict, sam_rho, sam_adaptive=False) -> dict:
    """``run_fingerprint``'s dict for a ``fit_sam`` run: with ``sam_rho`` and ``sam_adaptive``, both only when ``sam_rho`` is set,
    so the fingerprints and state files of runs without SAM are what they always were, and a run with and one without (or with
    another radius) cannot resume each other."""
    if sam_rho is None:
        return dict(fingerprint)
    return dict(fingerprint, sam_rho=float(sam_rho), sam_adaptive=bool(sam_adaptive))


def fit_sam(clip_dir: str, out_path: str, sam_rho: float, sam_adaptive: bool = False, **fit_args) -> float:
    """``fit(clip_dir, out_path, **fit_args)`` with sharpness-aware minimisation in every training step
    (``Trainer.enable_sam(sam_rho, sam_adaptive)``: SAM, or with ``sam_adaptive`` its scale-invariant form ASAM, whose radius is
    relative to the weights): the gradient that Adam applies is taken at the worst nearby point ``w + e`` of the step's batch, for a
    second forward and backward per step.  ``sam_rho`` must be finite and > 0 as float32 (``ValueError``, before anything touches a
    device or the clips); ``fit_args`` are checked against ``fit``'s signature first (``TypeError`` for a name it does not have).
    Works under both plans and with everything ``fit`` takes -- class weights, the policy and mixup, the weight average,
    ``freeze_cnn``, AdamW groups and schedules, a teacher (whose logits serve both passes), data parallel (two all-reduces per step;
    the perturbation is the global batch's).  The logged train loss and accuracy are the first pass's: those of the unperturbed
    weights, as a run without SAM logs them.  ``state_path``: the fingerprint holds ``sam_rho`` and ``sam_adaptive``
    (``sam_fingerprint``), so a resumed run must be a ``fit_sam`` run with the same two; the second pass reuses the step's dropout
    seed, a function of the step count, so a resumed run is the uninterrupted one as closely as it is without SAM.
    ``fit_calibrated(..., sam_rho=, sam_adaptive=)`` comes here."""
    sam_rho = check_sam_rho(sam_rho)
    if sam_rho is None:
        raise ValueError("fit_sam needs sam_rho (fit is the run without)")
    bound = inspect.signature(fit).bind(clip_dir, out_path, **fit_args)
    bound.apply_defaults()
    return _fit(sam_rho, bool(sam_adaptive), **bound.arguments)


def lamb_fingerprint(fingerprint: dict, lamb_exclude) -> dict:
    """A run fingerprint for a ``fit_lamb`` run: with ``lamb`` and ``lamb_exclude`` (the patterns as a list), both only when
    ``lamb_exclude`` is not None -- ``fit_lamb`` hands over the checked patterns, ``fit`` None -- so the fingerprints and state files
    of runs without LAMB are what they always were, and a run with and one without cannot resume each other."""
    if lamb_exclude is None:
        return dict(fingerprint)
    return dict(fingerprint, lamb=True, lamb_exclude=[str(p) for p in lamb_exclude])


def fit_lamb(clip_dir: str, out_path: str, lamb_exclude=None, **fit_args) -> float:
    """``fit(clip_dir, out_path, **fit_args)`` with the layer-wise adaptive optimiser LAMB in every training step
    (``Trainer.enable_lamb(lamb_exclude)``): the Adam direction plus the weight decay, rescaled per parameter tensor by ``|w| /
    |update|`` -- the usual tool when the global batch grows (``batch_size``, ``world_size``) and the learning rate should not be
    retuned per layer by hand.  ``lamb_exclude``: name patterns with ``ParamGroup.match``'s semantics whose tensors take the ratio 1;
    None: what ``no_decay()`` matches, the biases and the LayerNorm.  Bad patterns are a ``ValueError`` before anything touches a
    device or the clips; ``fit_args`` are checked against ``fit``'s signature first (``TypeError`` for a name it does not have),
    except ``sam_rho`` / ``sam_adaptive``, which switch SAM on as ``fit_sam`` does (its streams run in front of the optimiser).
    Works under both plans and with everything ``fit`` takes: ``lr``, the schedules, ``weight_decay`` (inside the update here),
    ``param_groups``, the weight average, ``freeze_cnn``, data parallel (the gradient is all-reduced before the optimiser, so every
    rank computes the same ratios).  The per-epoch log line gains the smallest, the median and the largest trust ratio of the
    epoch's last step over the tensors that adapt -- one read per epoch, behind the validation -- and ``history`` gets them as
    ``trust_ratio``.  ``state_path``: the fingerprint holds ``lamb`` and ``lamb_exclude`` (``lamb_fingerprint``), so a resumed run
    must be a ``fit_lamb`` run with the same exclusion; LAMB keeps no state beyond Adam's moments."""
    lamb_exclude = check_lamb_exclude(lamb_exclude)
    sam_rho = check_sam_rho(fit_args.pop("sam_rho", None))
    sam_adaptive = bool(fit_args.pop("sam_adaptive", False))
    bound = inspect.signature(fit).bind(clip_dir, out_path, **fit_args)
    bound.apply_defaults()
    return _fit(sam_rho, sam_adaptive, **bound.arguments, lamb_exclude=lamb_exclude)


def _fit(sam_rho, sam_adaptive, clip_dir, out_path, epochs, batch_size, patience, max_t, lr, seed, use_roi_if_present, device, log, plan,
         rank, world_size, process_group, history, class_weights, augment_policy, ema_decay, state_path, resume, init_from, freeze_cnn,
         weight_decay, param_groups, lr_schedule, lr_plateau, distill_from, distill_alpha, distill_temperature,
         lamb_exclude=None) -> float:
    """The body of ``fit`` (its docstring), ``fit_sam`` and ``fit_lamb``; ``sam_rho`` None: no SAM; ``lamb_exclude`` None: no LAMB."""
    if distill_from is not None:  # (host code, before anything touches a device or the clips)
        distill_alpha, distill_temperature = check_distill(distill_alpha, distill_temperature)
        if not isinstance(distill_from, (str, os.PathLike, BiGRUClassifier)):
            raise TypeError("distill_from must be a checkpoint path or a BiGRUClassifier")
        if plan != "device":
            raise ValueError("distill_from needs plan='device': the teacher's forward joins the enqueue-only epoch")
        if freeze_cnn:
            raise ValueError("distill_from does not combine with freeze_cnn: embedded batches hold no pixels for the teacher")
    check_lr_schedule(lr_schedule)
    if lr_plateau is not None and not isinstance(lr_plateau, PlateauSchedule):
        raise TypeError("lr_plateau must be a PlateauSchedule")
    check_weight_decay(weight_decay)
    if param_groups is not None:
        param_groups = tuple(param_groups)
        if not all(isinstance(g, ParamGroup) for g in param_groups):
            raise TypeError("param_groups must be ParamGroup objects")
    if plan not in ("host", "device"):
        raise ValueError(f"plan must be 'host' or 'device', not {plan!r}")
    if freeze_cnn:  # (before anything touches a device or the clips)
        if plan != "device":
            raise ValueError("freeze_cnn needs plan='device': the embedded batches are planned on the device")
        if init_from is None:
            raise ValueError("freeze_cnn needs init_from: a frozen, randomly initialised ROI CNN is a mistake")
        if augment_policy is not None and isinstance(augment_policy, AugmentPolicy) and augment_policy.roi_shift_prob > 0:
            raise ValueError("freeze_cnn cannot apply roi_shift_prob > 0: the shift acts on pixels")
        if augment_policy is not None and isinstance(augment_policy, AugmentPolicy) and augment_policy.cutout_prob > 0:
            raise ValueError("freeze_cnn cannot apply cutout_prob > 0: the cutout acts on pixels")
    if augment_policy is not None:
        if not isinstance(augment_policy, AugmentPolicy):
            raise TypeError("augment_policy must be an AugmentPolicy")
        if plan != "device":
            raise ValueError("augment_policy needs plan='device': the policy is drawn by the planning kernel")
        if augment_policy.mixup_on:
            if world_size > 1 or process_group is not None:
                raise ValueError("mixup_prob > 0 does not combine with data-parallel fit: a row's partner may lie in another rank's shard")
            if freeze_cnn:
                raise ValueError("mixup_prob > 0 does not combine with freeze_cnn: embedded batches are not mixed")
            if batch_size > 1024:
                raise ValueError("mixup_prob > 0 plans batches of at most 1024 clips")
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} is outside world_size {world_size}")
    parallel = world_size > 1 or process_group is not None
    if parallel and plan != "device":
        raise ValueError("data-parallel fit needs plan='device': only there is an epoch a pure function of (seed, draw index)")
    if (state_path is not None or resume) and plan != "device":
        raise ValueError("state_path / resume need plan='device': the sample order of plan='host' lives in the host's global "
                         "random state, which is not saved")
    if resume and state_path is None:
        raise ValueError("resume=True needs state_path")
    if rank != 0:
        log = lambda *a, **k: None  # noqa: E731  (rank 0 alone logs)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    info = scan_clips(clip_dir)
    if class_weights is not None and not (isinstance(class_weights, str) and class_weights == "balanced"):
        class_weights = check_class_weights(class_weights, len(info["uniq"]))  # (before anything is uploaded)
    train_files, val_files = split_by_label(info["files"], info["labels"], VAL_FRAC, seed=seed)
    use_roi = use_roi_if_present and info["has_roi"] > 0
    train_labels = [str(np.load(f, allow_pickle=True)["label"]) for f in train_files]
    if isinstance(class_weights, str):
        class_weights = check_class_weights(balanced_class_weights(train_labels, info["id_to_label"]), len(info["uniq"]))
    if freeze_cnn and not use_roi:
        raise ValueError("freeze_cnn needs clips with ROI frames (and use_roi_if_present)")
    init_ckpt = None
    if init_from is not None:  # (host code: the mismatches raise before anything is uploaded)
        init_ckpt = load_init_checkpoint(init_from, info["x_dim"], use_roi, 32, 192)
    module_teacher = isinstance(distill_from, BiGRUClassifier)
    if module_teacher:  # (host code again: the mismatches raise before anything is uploaded)
        cfg_t = distill_from.cfg
        check_teacher(cfg_t.x_dim, cfg_t.use_roi, cfg_t.num_classes, None, info["x_dim"], use_roi, info["uniq"])
    elif distill_from is not None:
        teacher_ckpt = torch.load(distill_from, map_location="cpu", weights_only=False)
        check_teacher(teacher_ckpt["x_dim"], teacher_ckpt.get("use_roi", False), len(teacher_ckpt["labels"]),
                      teacher_ckpt["labels"], info["x_dim"], use_roi, info["uniq"])
    saved, fingerprint = None, None
    if state_path is not None:
        fingerprint = run_fingerprint(seed, batch_size, world_size, max_t, lr, info["uniq"], info["x_dim"], use_roi,
                                      len(train_files), len(val_files), class_weights, augment_policy, ema_decay,
                                      init_from=None if init_from is None else file_sha256(init_from), freeze_cnn=freeze_cnn,
                                      weight_decay=weight_decay, param_groups=param_groups, lr_schedule=lr_schedule,
                                      lr_plateau=lr_plateau,
                                      distill_from=None if distill_from is None else
                                      ("module" if module_teacher else file_sha256(distill_from)),
                                      distill_alpha=distill_alpha, distill_temperature=distill_temperature)
        fingerprint = lamb_fingerprint(sam_fingerprint(fingerprint, sam_rho, sam_adaptive), lamb_exclude)
        if resume and os.path.exists(state_path):
            saved = load_train_state(state_path)
            field = fingerprint_difference(saved["fingerprint"], fingerprint)
            if field is not None:
                raise ValueError(f"cannot resume from {state_path}: {field} differs (saved {saved['fingerprint'].get(field)!r}, "
                                 f"this call {fingerprint.get(field)!r})")
            if saved["stopped"] or saved["epoch"] >= epochs:  # nothing left to train: no store, no model
                log(f"Nothing to resume: {state_path} ends at epoch {saved['epoch']}. Best val acc: {saved['best']:.3f}")
                _barrier(process_group)
                return float(saved["best"])
    train_store = DeviceClipStore(train_files, info["label_to_id"], max_t=max_t, use_roi=use_roi, device=device)
    val_store = DeviceClipStore(val_files, info["label_to_id"], max_t=max_t, use_roi=use_roi, device=device)
    model = BiGRUClassifier(info["x_dim"], len(info["uniq"]), use_roi=use_roi, roi_emb=32, hidden=192,
                            gru_layers=2 if init_ckpt is None else int(init_ckpt.get("gru_layers", 2))).to(device).train()
    if init_ckpt is not None:
        sd = dict(init_ckpt["model"])
        if list(init_ckpt["labels"]) != list(info["uniq"]):
            log(f"init_from {init_from}: its {len(init_ckpt['labels'])} labels differ from the clips' {len(info['uniq'])}; "
                "head.4.weight and head.4.bias keep their fresh initialisation")
            fresh = model.state_dict()
            sd["head.4.weight"], sd["head.4.bias"] = fresh["head.4.weight"], fresh["head.4.bias"]
        model.load_state_dict(sd)
    if process_group is not None:
        import torch.distributed as dist

        dist.broadcast(model.flat_params, src=dist.get_global_rank(process_group, 0), group=process_group)
    if lr_schedule is not None and lr_schedule.decay != "none" and lr_schedule.total_steps is None:
        lr_schedule = dataclasses.replace(lr_schedule, total_steps=epochs * -(-len(train_files) // batch_size))
    plateau = None
    if lr_plateau is not None:  # (a copy that starts fresh: the caller's object may have served another run)
        plateau = copy.copy(lr_plateau)
        plateau.reset()
    trainer = Trainer(model, lr=lr, world_size=world_size, process_group=process_group,
                      always_allreduce=process_group is not None, class_weights=class_weights, ema_decay=ema_decay,
                      freeze_cnn=freeze_cnn, weight_decay=weight_decay, param_groups=param_groups, lr_schedule=lr_schedule,
                      **({} if distill_from is None else dict(distill_alpha=distill_alpha, distill_temperature=distill_temperature)))
    trainer.rank = rank
    if sam_rho is not None:
        trainer.enable_sam(sam_rho, sam_adaptive)
    if lamb_exclude is not None:
        trainer.enable_lamb(lamb_exclude)
    teacher = None
    if distill_from is not None:
        teacher = distill_from if module_teacher else load_classifier(distill_from, device=device)[0]
        if teacher.flat_params is None or not teacher.flat_params.is_cuda:
            raise ValueError("distill_from: a module teacher must already be on the device")
        teacher.eval()
    # validation and the checkpoint see the averaged weights when there are any (two swap launches around each)
    averaged = trainer.ema_weights if ema_decay is not None else contextlib.nullcontext
    roi_hw = train_store.roi_hw or (48, 96)
    gen = np.random.default_rng(seed)
    best, bad, first_epoch = 0.0, 0, 1
    if saved is not None:  # (every rank: the file overrides the broadcast above with the same bits everywhere)
        model.load_state_dict(saved["model"])
        trainer.load_state_dict(saved["trainer"])
        best, bad, first_epoch = float(saved["best"]), int(saved["bad"]), int(saved["epoch"]) + 1
        if plateau is not None:
            plateau.load_state_dict(saved["plateau"])
            trainer.lr_scale = plateau.scale
        log(f"Resuming from {state_path} at epoch {first_epoch} (best val acc {best:.3f})")
    if freeze_cnn:  # (behind the load, the broadcast and a resume: the CNN is final now, and the same on every rank)
        train_store.embed(model)
        val_store.embed(model)
    mixup = augment_policy is not None and augment_policy.mixup_on
    for ep in range(first_epoch, epochs + 1):
        epoch_base = (ep - 1) * len(train_store)
        if plan == "device":
            order = train_store.sample_epoch(seed=seed, first=epoch_base)
        else:
            order = class_balanced_indices(train_labels)
        tr_loss = torch.zeros((), device=device)
        tr_ok = torch.zeros((), device=device, dtype=torch.int64)
        if plan == "device":
            # class weights: the labels of the whole epoch order, one gather on the device; a step's global batch is a slice
            y_epoch = train_store.y[order.long()] if class_weights is not None else None
            for k, (lo, hi, first_row, global_batch) in enumerate(epoch_shards(len(order), batch_size, rank, world_size)):
                if hi > lo:
                    X, T, R, y = train_store.batch(order[lo:hi], augment=True, rng="philox", seed=seed,
                                                   first_row=epoch_base + first_row,
                                                   batch_first_row=epoch_base + lo - lo % batch_size, policy=augment_policy,
                                                   embedded=freeze_cnn)
                else:
                    X, T, R, y = train_store.empty_batch(embedded=freeze_cnn)
                # (the loss is this rank's part of the global mean: the parts of all ranks sum to it)
                y_glob = None if y_epoch is None else y_epoch[k * batch_size:k * batch_size + global_batch]
                if freeze_cnn:  # (X is Z: the rows features | embedding)
                    loss, correct = trainer.step_embedded(X, T, y, global_batch=global_batch, y_global=y_glob)
                else:
                    mix = train_store.mix[:2] if mixup and hi > lo else None
                    t_logits = None
                    if teacher is not None and hi > lo:  # (the batch the student sees; enqueue-only: T is on the device)
                        with torch.no_grad():
                            t_logits = teacher(X, T, R if use_roi else None)
                    loss, correct = trainer.step(X, T, R if use_roi else None, y, global_batch=global_batch, y_global=y_glob, mix=mix,
                                                 teacher_logits=t_logits)
                tr_loss += loss * global_batch
                tr_ok += correct
            with averaged():
                res = evaluate_device(model, val_store, batch_size, rank=rank, world_size=world_size, process_group=process_group,
                                      extra_sums=torch.stack([tr_loss.double(), tr_ok.double()]), class_weights=class_weights,
                                      embedded=freeze_cnn)
            train_store.check()  # (the evaluation above has synchronised)
            val_store.check()
            va_loss, va_acc, tr_loss, tr_ok = res.loss, res.acc, res.extra[0], res.extra[1]
            confs = top_confusions_from_matrix(res.confusion, res.first_seen, info["id_to_label"], k=6)
        else:
            for lo in range(0, len(order), batch_size):
                idx = order[lo:lo + batch_size]
                X, T, R, y = train_store.batch(idx, augment=True, rng="device", generator=gen)
                loss, correct = trainer.step(X, T, R if use_roi else None, y)
                tr_loss += loss * len(idx)
                tr_ok += correct
            with averaged():
                va_loss, va_acc, y_true, y_pred = evaluate(model, val_store, batch_size, plan=plan, class_weights=class_weights)
            confs = top_confusions(y_true, y_pred, info["id_to_label"], k=6)
        n = max(1, len(order))
        trust = None
        if lamb_exclude is not None:  # (one read per epoch, behind the validation's: the last step's ratios of the tensors that adapt)
            r = trainer.trust_ratios()[torch.tensor(trainer.lamb.adapt, dtype=torch.bool, device=trainer.lamb_ratio.device)]
            trust = tuple(torch.stack([r.min(), r.median(), r.max()]).tolist()) if r.numel() else (1.0, 1.0, 1.0)
        if history is not None:
            history.append(dict(epoch=ep, train_loss=float(tr_loss) / n, train_acc=int(tr_ok) / n, val_loss=va_loss, val_acc=va_acc,
                                **({} if lr_schedule is None and plateau is None else {"lr": trainer.current_lr()}),
                                **({} if trust is None else {"trust_ratio": trust})))
        log(f"ep {ep:02d} | train loss {float(tr_loss) / n:.4f} acc {int(tr_ok) / n:.3f} | val loss {va_loss:.4f} acc {va_acc:.3f}"
            + ("" if trust is None else f" | trust ratio min {trust[0]:.3g} med {trust[1]:.3g} max {trust[2]:.3g}")
            + ((" | top confusions: " + ", ".join(confs)) if confs else ""))
        if plateau is not None:  # (every rank holds the same reduced metrics: the same decision everywhere)
            if plateau.step(va_acc if plateau.mode == "max" else va_loss):
                log(f"  lr plateau: scale {trainer.lr_scale:g} -> {plateau.scale:g}")
            trainer.lr_scale = plateau.scale
        stop = False
        if va_acc > best:
            best, bad = va_acc, 0
            if rank == 0:
                with averaged():
                    save_checkpoint(out_path, model, info["uniq"], max_t=max_t, roi_w=roi_hw[1], roi_h=roi_hw[0], seed=seed)
            log(f"  saved {out_path} (best val acc {best:.3f})")
        else:
            bad += 1
            stop = bad >= patience
        if state_path is not None and rank == 0:
            save_train_state(state_path, dict(format=TRAIN_STATE_FORMAT, model=model.state_dict(), trainer=trainer.state_dict(),
                                              epoch=ep, best=float(best), bad=int(bad), stopped=bool(stop), fingerprint=fingerprint,
                                              **({} if plateau is None else {"plateau": plateau.state_dict()})))
        if stop:
            log(f"Early stopping. Best val acc: {best:.3f}")
            break
    _barrier(process_group)
    return best


def calibrate_checkpoint(out_path: str, val_store: DeviceClipStore, batch_size: int = BATCH_SIZE, device="cuda", log=print):
    """The weights of the checkpoint at ``out_path`` -- of a ``fit`` run: the best epoch's, under ``ema_decay`` the averaged ones --
    are loaded into a model (``load_classifier``), ``calibrate.calibrate`` runs over the whole of ``val_store``, and the file is
    rewritten atomically with the keys ``"temperature"`` and ``"calibration"`` and its weights bit for bit.  One line is logged:
    T, NLL and ECE before and after, top-3 accuracy.  -> the ``Calibration``, or None when there is no checkpoint."""
    from .calibrate import calibrate as run_calibration

    if not os.path.exists(out_path):
        return None
    model = load_classifier(out_path, device=device)[0]
    cal = run_calibration(model, val_store, batch_size)
    add_calibration(out_path, cal.temperature, cal.plain())
    top3 = cal.topk_acc[min(3, len(cal.topk_acc)) - 1]
    log(f"calibrated {out_path}: T {cal.temperature:.4f} | val NLL {cal.nll_before:.4f} -> {cal.nll_after:.4f} | "
        f"ECE {cal.ece_before:.4f} -> {cal.ece_after:.4f} | top-3 acc {top3:.3f}")
    return cal


def fit_calibrated(clip_dir: str, out_path: str, **fit_args) -> float:
    """``fit(clip_dir, out_path, **fit_args)``, then calibrated confidences for the checkpoint it left (the reference prints
    uncalibrated probabilities): when training is over -- after the last epoch, an early stop, or for a resumed run that had already
    finished -- rank 0, if ``out_path`` exists, fits a softmax temperature on the whole validation store of the run's split with the
    checkpoint's weights and rewrites the checkpoint with the keys ``"temperature"`` and ``"calibration"`` (``calibrate_checkpoint``);
    the other ranks wait at a barrier, and every rank returns ``fit``'s ``best``.  ``fit`` itself is called as it is: nothing about
    training, the run fingerprint or the train-state file changes, and the weights in the checkpoint keep their bits.
    ``fit_args`` are checked against ``fit``'s signature before any work (``TypeError`` for a name it does not have)."""
    sam = {k: fit_args.pop(k) for k in ("sam_rho", "sam_adaptive") if k in fit_args}  # (fit_sam's two: not names of fit)
    bound = inspect.signature(fit).bind(clip_dir, out_path, **fit_args)
    bound.apply_defaults()
    a = bound.arguments
    best = fit_sam(clip_dir, out_path, **sam, **fit_args) if sam.get("sam_rho") is not None else fit(clip_dir, out_path, **fit_args)
    if a["rank"] == 0 and os.path.exists(out_path):
        # the validation clips of the run: the same scan and the same split by the same seed
        info = scan_clips(clip_dir)
        _, val_files = split_by_label(info["files"], info["labels"], VAL_FRAC, seed=a["seed"])
        use_roi = a["use_roi_if_present"] and info["has_roi"] > 0
        val_store = DeviceClipStore(val_files, info["label_to_id"], max_t=a["max_t"], use_roi=use_roi, device=a["device"])
        calibrate_checkpoint(out_path, val_store, a["batch_size"], a["device"], a["log"])
    _barrier(a["process_group"])
    return best
