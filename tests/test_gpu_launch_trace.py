"""GPU: the launch sequence of a training step, an evaluation and an autograd pass, entry for entry.

``launch_trace_parent.json`` holds what ``launch_trace.run_case`` saw on an MI355X at the commit before the engines' shared tail,
head and fork code moved into one place (its header names the command).  With the side stream on, every launch (entry point,
timing tag, stream, every argument) and every event record and wait must be the recorded one, in the recorded order; with both
engines' ``USE_SIDE_STREAM`` off (bench.py's per-kernel timing pass) the launches must be -- that mode runs the side work inline
and leaves the events out.

Cases (launch_trace.CASES): the f32 engine with the fused 32 x 32 ROI CNN (inter-layer dropout inside the multi-CU recurrence);
without ROI, plus an autograd pass that asks for d X; at the smallest batch that has no multi-CU recurrence (ss_dropout as its own
launch); the bf16 engine with K a multiple of 64 (grouped weight gradients and their flush schedule over three layers), with K
not one (three launches per layer), and with the 96 x 96 ROI CNN (the fc fork).  Lengths are ragged and dropout is on."""
import json
import os

import pytest
import torch

import launch_trace as LT

pytestmark = pytest.mark.gpu

# the multi-CU recurrence wants ceil(B / 16) slices x 2 directions x 6 parts co-resident on 256 - 16 CUs (gru_split.h): B <= 320
F32_ONE_CU_BATCH = 321


@pytest.fixture(scope="module")
def parent():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_trace_parent.json")) as f:
        return json.load(f)


def first_difference(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"entry {i}:\n  got  {a}\n  want {b}"
    return f"{len(got)} entries, {len(want)} recorded"


@pytest.mark.parametrize("side_stream", [True, False], ids=["side", "one_stream"])
@pytest.mark.parametrize("name", list(LT.CASES))
def test_launch_sequence_is_the_recorded_one(parent, monkeypatch, name, side_stream):
    if name == "f32_one_cu":
        assert LT.smallest_batch_without_gru_sync() == F32_ONE_CU_BATCH == parent["header"]["f32_one_cu_batch"]
    got = LT.run_case(monkeypatch, name, side_stream)
    want = parent["traces"][LT.key(name, side_stream)]
    assert sorted(got) == sorted(want) and got["gru_sync"] == want["gru_sync"]
    if name in ("f32_roi32", "f32", "f32_one_cu"):  # the fused-dropout arm needs the multi-CU recurrence, the ss_dropout arm its absence
        assert got["gru_sync"] == (name != "f32_one_cu")
    for call in LT.CASES[name][4]:
        print(f"{name} {call}: {len(LT.launches(got[call]))} launches, {len(got[call]) - len(LT.launches(got[call]))} event entries")
        assert len(want[call]) > 0
        assert got[call] == want[call], f"{name} {call}: " + first_difference(got[call], want[call])
    if side_stream:
        assert any(e[0] == "wait" and e[2] == "side" for e in got["step"])  # the trace does see the fork
        assert any(e[0] == "launch" and e[3] == "side" for e in got["step"])
    else:
        assert all(e[3] == "main" for e in got["step"])
