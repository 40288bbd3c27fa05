"""Helper of test_gpu_trainer_trace.py: what one ``Trainer`` step, and one ``harness.fit`` call, hand to the device queues.

``run_config(mp, name)`` builds the model and the trainer of ``CONFIGS[name]``, takes one warm-up step and returns the
``launch_trace.traced`` list of the second, with one more kind of entry:

    ["zero", element count]    a ``Tensor.zero_()`` of the step (the unfused prologue's three zeroings), at its place among the
                               launches, records and waits

``run_fit(mp, name, work, clip_dir)`` runs the ``fit`` calls of ``FIT_CASES[name]`` on the clip directory ``write_clips`` made under
``work`` and returns, per call, the ordered ``[entry point, timing tag]`` of every ``_lib.call`` -- no argument: the listed-frames choice of
the CNN launch rests on an unsynchronised pinned read, so a pointer argument may differ between two runs.

Run as a program it records both of the tree it is in:  python tests/trainer_trace.py tests/trainer_trace_parent.json
"""
import json
import os
import sys
import tempfile

import torch

import gpu_support as GS
import launch_trace as LT

F32 = dict(x_dim=84, num_classes=5, use_roi=True)
BF16 = dict(x_dim=84, num_classes=5, hidden=128, gru_layers=2, precision="bf16")
WEIGHTS = [1.0, 2.0, 0.5, 1.5, 1.0]
GROUPS = dict(weight_decay=1e-3, param_groups="no_decay")  # ("no_decay": [ss.no_decay()], made when the package is there)
# name -> model keywords, Trainer keywords, B, and what the step is given besides the batch:
#   mix / teacher: step(mix=) / step(teacher_logits=); empty: the shard X[:0] of a global batch of B; int32: int32 lengths (the
#   unfused prologue); embedded: step_embedded on a random Z
CONFIGS = {
    "default": (F32, {}, 4, ()),
    "class_weights": (F32, dict(class_weights=WEIGHTS), 4, ()),
    "ema": (F32, dict(ema_decay=0.9), 4, ()),
    "groups": (F32, GROUPS, 4, ()),
    "groups_ema": (F32, dict(GROUPS, ema_decay=0.9), 4, ()),
    "lr_schedule": (F32, dict(lr_schedule=dict(warmup_steps=3)), 4, ()),
    "mix": (F32, {}, 4, ("mix",)),
    "teacher": (F32, {}, 4, ("teacher",)),
    "weights_mix_teacher": (F32, dict(class_weights=WEIGHTS), 4, ("mix", "teacher")),
    "empty_shard": (F32, {}, 4, ("empty",)),
    "int32_lengths": (F32, {}, 4, ("int32",)),
    "frozen": (F32, dict(freeze_cnn=True), 4, ("embedded",)),
    "frozen_int32_lengths": (F32, dict(freeze_cnn=True), 4, ("embedded", "int32")),
    "frozen_groups_ema": (F32, dict(GROUPS, freeze_cnn=True, ema_decay=0.9), 4, ("embedded",)),
    # B = 32: the smallest batch at which the fan-out is taken (16 clips per slice)
    "micro_batches": (F32, dict(micro_batches=2), 32, ()),
    "bf16_landmarks": (BF16, {}, 4, ()),
}
T, ROI = LT.T_F32, (32, 32)


def _zeroings_in(mp, fn):
    """``fn`` that also notes every ``Tensor.zero_()`` among the entries of the running ``traced`` list (``.marks``: None per entry
    of that list, an element count per zeroing).  The list is private to ``traced``, but its three replacements are in place when
    ``fn`` runs: they are what is counted."""
    from silent_speech_amd import _lib

    def wrapped():
        real_zero, marks = torch.Tensor.zero_, []
        traced_call, traced_record, traced_wait = _lib.call, torch.cuda.Event.record, torch.cuda.Stream.wait_event

        def call(name, *args, tag=None):
            marks.append(None)
            return traced_call(name, *args, tag=tag)

        def record(self, stream=None):
            marks.append(None)
            return traced_record(self, stream)

        def wait_event(self, event):
            marks.append(None)
            return traced_wait(self, event)

        def zero_(self):
            marks.append(self.numel())
            return real_zero(self)

        with mp.context() as m:
            m.setattr(_lib, "call", call)
            m.setattr(torch.cuda.Event, "record", record)
            m.setattr(torch.cuda.Stream, "wait_event", wait_event)
            m.setattr(torch.Tensor, "zero_", zero_)
            fn()
        wrapped.marks = marks

    return wrapped


def _with_zeroings(log, marks):
    """``log`` with a ["zero", element count] entry where each zeroing took place (``marks``: None per entry of ``log``)."""
    entries = iter(log)
    out = [next(entries) if mark is None else ["zero", mark] for mark in marks]
    assert next(entries, None) is None
    return out


def run_config(mp, name):
    import silent_speech_amd as ss

    kw, tkw, B, extra = CONFIGS[name]
    tkw = dict(tkw)
    if tkw.get("param_groups") == "no_decay":
        tkw["param_groups"] = [ss.no_decay()]
    if "lr_schedule" in tkw:
        tkw["lr_schedule"] = ss.LrSchedule(**tkw["lr_schedule"])
    dev, C = torch.device("cuda"), kw["num_classes"]
    g = torch.Generator().manual_seed(5)
    hw = ROI if kw.get("use_roi") else None
    X = torch.randn(B, T, kw["x_dim"], generator=g).to(dev)
    R = torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8).to(dev) if hw else None
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    Z = torch.randn(B, T, kw["x_dim"] + 32, generator=g).to(dev)
    teacher = torch.randn(B, C, generator=g).to(dev)
    # ragged, as launch_trace.run_case builds them
    lengths = torch.tensor([max(1, T - b % 3) for b in range(B)], dtype=torch.int32 if "int32" in extra else torch.int64, device=dev)
    model = ss.BiGRUClassifier(**kw).to(dev).train()
    tr = ss.Trainer(model, dropout=True, **tkw)
    step_kw = {}
    if "mix" in extra:
        step_kw["mix"] = (y.flip(0).contiguous(), torch.tensor([0.75], device=dev))
    if "teacher" in extra:
        step_kw["teacher_logits"] = teacher
    if "empty" in extra:
        X, lengths, R, y, step_kw["global_batch"] = X[:0], lengths[:0], R[:0], y[:0], B
    if "embedded" in extra:
        step = lambda: tr.step_embedded(Z, lengths, y, **step_kw)  # noqa: E731
    else:
        step = lambda: tr.step(X, lengths, R, y, **step_kw)  # noqa: E731
    step()
    fn = _zeroings_in(mp, step)
    log = LT.traced(mp, model, fn)
    assert tr.step_count == 2
    return _with_zeroings(log, fn.marks)


# ------------------------------------------------------------------------------------------------ fit
FIT = dict(epochs=1, batch_size=4, max_t=16, log=lambda *a: None)
# name -> the fit calls of the case, in order: keywords on top of FIT.  "init": the checkpoint of a plain one-epoch run (made once,
# untraced); "policy" / "teacher": made when the package is there
FIT_CASES = {
    "host": [dict(plan="host")],
    "device": [dict(plan="device")],
    "policy_masks_mixup": [dict(plan="device", augment_policy="policy")],
    "weights_ema_resume": [dict(plan="device", class_weights="balanced", ema_decay=0.9, state_path="state"),
                           dict(plan="device", class_weights="balanced", ema_decay=0.9, state_path="state", resume=True, epochs=2)],
    "init_freeze_cnn": [dict(plan="device", init_from="init", freeze_cnn=True)],
    "distill_module": [dict(plan="device", distill_from="teacher")],
    "weight_decay_plateau": [dict(plan="device", weight_decay=1e-3, lr_plateau="plateau")],
}


def write_clips(work):
    """12 clips, 3 labels, 6 to 14 frames, 32 x 32 ROI frames -> the directory; and the checkpoint ``init`` of one plain epoch."""
    from silent_speech_amd import harness as Hn

    clip_dir = GS.write_clips(os.path.join(work, "clips_npz"), GS.WORDS, n=12, roi=ROI, frames=(6, 15))
    Hn.fit(clip_dir, os.path.join(work, "init.pt"), **dict(FIT, plan="device"))
    return clip_dir


def run_fit(mp, name, work, clip_dir):
    import silent_speech_amd as ss
    from silent_speech_amd import _lib
    from silent_speech_amd import harness as Hn

    made = {"policy": lambda: ss.AugmentPolicy.lineage(time_mask_prob=1.0, time_mask_max=3, feat_mask_prob=1.0, feat_mask_max=4,
                                                       cutout_prob=1.0, cutout_max=(8, 8), mixup_prob=1.0),
            "teacher": lambda: ss.BiGRUClassifier(20, 3, use_roi=True, gru_layers=3).cuda(),
            "plateau": lambda: ss.PlateauSchedule(patience=0),
            "init": lambda: os.path.join(work, "init.pt"),
            "state": lambda: os.path.join(work, name + ".state")}
    out = []
    for kw in FIT_CASES[name]:
        kw = {k: made[v]() if isinstance(v, str) and v in made else v for k, v in kw.items()}
        log, real_call = [], _lib.call

        def call(entry, *args, tag=None):
            log.append([entry, tag or entry])
            return real_call(entry, *args, tag=tag)

        with mp.context() as m:
            m.setattr(_lib, "call", call)
            Hn.fit(clip_dir, os.path.join(work, name + ".pt"), **dict(FIT, **kw))
        torch.cuda.synchronize()
        out.append(log)
    return out


def dumps(doc):
    """JSON with one trace entry per line: a launch that moved is one changed line of the file."""
    c = dict(separators=(",", ":"))

    def block(v, pad):
        return "[\n" + ",\n".join(pad + json.dumps(e, **c) for e in v) + "\n" + pad[:-1] + "]"

    steps = ",\n".join(f' {json.dumps(k)}:' + block(v, "  ") for k, v in doc["steps"].items())
    fits = ",\n".join(f' {json.dumps(k)}:[\n' + ",\n".join("  " + block(v, "   ") for v in calls) + "\n ]" for k, calls in doc["fits"].items())
    return '{"header":' + json.dumps(doc["header"], indent=1) + ',\n"steps":{\n' + steps + '\n},\n"fits":{\n' + fits + "\n}}\n"


if __name__ == "__main__":
    import pytest

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    mp = pytest.MonkeyPatch()
    doc = {"header": {"what": "launch traces of tests/test_gpu_trainer_trace.py, recorded on one MI355X",
                      "recorded_with": "python tests/trainer_trace.py tests/trainer_trace_parent.json",
                      "tree": sys.argv[2] if len(sys.argv) > 2 else "unnamed"},
           "steps": {n: run_config(mp, n) for n in CONFIGS}}
    with tempfile.TemporaryDirectory() as work:
        clip_dir = write_clips(work)
        doc["fits"] = {n: run_fit(mp, n, work, clip_dir) for n in FIT_CASES}
    with open(sys.argv[1], "w") as f:
        f.write(dumps(doc))
