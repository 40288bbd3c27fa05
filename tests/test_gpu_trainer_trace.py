"""GPU: what ``Trainer.step`` / ``step_embedded`` and ``harness.fit`` hand to the device queues, entry for entry.

``trainer_trace_parent.json`` holds what ``trainer_trace`` saw on an MI355X at the commit before the trainer's two steps got one
skeleton (its header names the command).  The second step of every configuration of
``trainer_trace.CONFIGS`` -- the default trainer; class weights; the weight average; parameter groups, alone and with the average;
a schedule; ``mix=``; ``teacher_logits=``; all three of the loss; an empty shard; int32 lengths (the unfused prologue, whose three
zeroings the trace shows); ``freeze_cnn`` with both prologues, and with groups and the average; two micro-batches at B = 32; a bf16
landmark model -- must be the recorded one: every launch (entry point, timing tag, stream, every argument by value, pointers as
"ptr" / "null"), every event record and wait and every zeroing, in the recorded order.  Of one epoch of ``fit`` on a synthetic
directory (``trainer_trace.FIT_CASES``) the ordered (entry point, timing tag) pairs must be the recorded ones; their arguments are
left out, since the listed-frames choice of the CNN launch rests on an unsynchronised pinned read."""
import json
import os

import pytest
import torch

import trainer_trace as TT
from test_gpu_launch_trace import first_difference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_trace_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def clips(parent, tmp_path_factory):
    work = str(tmp_path_factory.mktemp("fit_trace"))
    return work, TT.write_clips(work)


@pytest.mark.parametrize("name", list(TT.CONFIGS))
def test_second_step_is_the_recorded_one(parent, monkeypatch, name):
    got, want = TT.run_config(monkeypatch, name), parent["steps"][name]
    names = [e[1] for e in got if e[0] == "launch"]
    print(f"{name}: {len(names)} launches, {sum(e[0] == 'zero' for e in got)} zeroings, {len(got)} entries")
    assert len(want) > 0
    assert got == want, f"{name}: " + first_difference(got, want)
    # the trace does see what the configuration is about
    extra = TT.CONFIGS[name][3]
    assert ("ss_train_prologue" in names) == (not {"empty", "int32"} & set(extra) and name != "micro_batches")
    assert sum(e[0] == "zero" for e in got) >= (0 if "ss_train_prologue" in names else 3)
    assert ("ss_class_weight_sum" in names) == ("class_weights" in TT.CONFIGS[name][1])
    adam = [n for n in names if n in ("ss_adam_clip", "ss_adam_clip_ema", "ss_adamw_clip_groups")]
    tkw = TT.CONFIGS[name][1]
    assert adam == ["ss_adamw_clip_groups" if "param_groups" in tkw else "ss_adam_clip_ema" if "ema_decay" in tkw else "ss_adam_clip"]
    assert ("ss_roi_cnn_set_max_workgroups" in names) == (name == "micro_batches")
    if "embedded" in extra:  # a frozen CNN is never launched
        assert not any(n.startswith("ss_roi_cnn") for n in names)
    if name == "micro_batches":
        assert any(e[0] == "launch" and e[3] == "side" for e in got) and sum(e[0] == "wait" for e in got) >= 4


@pytest.mark.parametrize("name", list(TT.FIT_CASES))
def test_fit_launches_are_the_recorded_ones(parent, clips, monkeypatch, name):
    got, want = TT.run_fit(monkeypatch, name, *clips), parent["fits"][name]
    assert len(got) == len(want) == len(TT.FIT_CASES[name])
    for call, (g, w) in enumerate(zip(got, want)):
        print(f"{name} call {call}: {len(g)} launches")
        assert len(w) > 0
        assert g == w, f"{name} call {call}: " + first_difference(g, w)
