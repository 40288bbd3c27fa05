"""Time the two LAMB entry points -- ss_lamb_moments (its stream and its per-segment reduction), ss_lamb_apply (without and with
the weight average) -- beside ss_adam_clip, ss_adam_clip_ema and ss_adamw_clip_groups on the flat buckets of BASELINE configs 2
and 5, each with its model's one-segment-per-tensor table, and a LAMB step against the plain step at the config-2 and the shipped
batch-16 shapes.

    python tools/lamb_bench.py [--rounds 20] [--launches 50] [--steps 30]

One process, warm, HIP events.  Kernels: the entry points alternate in rounds of ``launches`` back-to-back calls on one stream,
each round between two events; the figure is the median over the rounds of (round time / launches), with the bytes each call must
move (streams of the bucket x 4 n) and the rate that makes; ss_adam_clip is timed twice per round, the second window is the A/A
row.  Steps: a plain trainer, a LAMB trainer and the plain trainer again (the A/A window) take ``steps`` steps each per round on the
same batch, dropout on; median ms per step."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import silent_speech_amd as ss  # noqa: E402
from silent_speech_amd import _lib as L  # noqa: E402
from silent_speech_amd.train import LambTable, SegmentTable, check_lamb_exclude  # noqa: E402
from sam_bench import ADAM, SHAPES, models, timed  # noqa: E402


def kernels(model, a):
    n = model.flat_params.numel()
    groups = SegmentTable(model, [ss.no_decay()], 1e-2)
    lamb = LambTable(model, [ss.no_decay()], 1e-2, check_lamb_exclude(None))
    g = torch.Generator().manual_seed(0)
    p, gr, m, ema = (torch.randn(n, generator=g).cuda() for _ in range(4))
    gr *= 0.01
    v = torch.rand(n, generator=g).cuda() * 1e-4
    ssq = torch.zeros(1, device="cuda")
    L.call("ss_sumsq_f32", gr.data_ptr(), n, ssq.data_ptr(), L.stream())
    n_seg = len(lamb.seg_end)
    size = C.c_long(0)
    L.call("ss_lamb_scratch_bytes", n, n_seg, C.addressof(size))
    scratch = torch.empty(size.value // 8, dtype=torch.float64, device="cuda")
    norms, ratio = torch.zeros(2 * n_seg, device="cuda"), torch.ones(n_seg, device="cuda")
    s, step = L.stream(), [0]
    P, G, M, V, E, S = (t.data_ptr() for t in (p, gr, m, v, ema, ssq))

    def adam(name, *extra, tail=()):
        def fn():
            step[0] += 1
            L.call(name, P, G, M, V, *extra[:1], n, S, *ADAM, step[0], *extra[1:], *tail, s)
        return fn

    def moments():
        step[0] += 1
        L.call("ss_lamb_moments", P, G, M, V, n, S, ADAM[0], ADAM[1], *ADAM[3:], step[0], *lamb.args, scratch.data_ptr(),
               norms.data_ptr(), ratio.data_ptr(), s)

    def apply(e, d):
        def fn():  # (the ratios of the last ss_lamb_moments call; lr = 0 would skip nothing: the kernel does not look at it)
            L.call("ss_lamb_apply", P, M, V, e, n, *ADAM[3:], max(step[0], 1), d, ADAM[2], *lamb.args, ratio.data_ptr(), s)
        return fn

    # name -> (call, streams of the bucket it must move)
    windows = {"ss_adam_clip": (adam("ss_adam_clip"), 7),
               "ss_lamb_moments": (moments, 6),
               "ss_lamb_apply": (apply(None, 0.0), 4),
               "ss_adam_clip_again": (adam("ss_adam_clip"), 7),
               "ss_adam_clip_ema": (adam("ss_adam_clip_ema", E, 0.999), 9),
               "ss_lamb_apply_ema": (apply(E, 0.999), 6),
               "ss_adamw_clip_groups": (adam("ss_adamw_clip_groups", None, 0.999, tail=groups.args), 7)}
    times = {k: [] for k in windows}
    for rnd in range(-2, a.rounds):
        for key, (fn, _) in windows.items():
            t = timed(fn, a.launches) * 1e3
            if rnd >= 0:
                times[key].append(t)
    row = {"floats": n, "lamb_segments": n_seg, "groups_segments": len(groups.seg_end), "scratch_bytes": size.value}
    for key, (_, streams) in windows.items():
        us = statistics.median(times[key])
        row[key] = {"us": round(us, 3), "us_min_max": [round(min(times[key]), 3), round(max(times[key]), 3)],
                    "mbytes": round(streams * 4 * n * 1e-6, 2), "gbytes_per_s": round(streams * 4 * n / us * 1e-3, 1)}
    row["lamb_over_adam_clip"] = round((row["ss_lamb_moments"]["us"] + row["ss_lamb_apply"]["us"]) / row["ss_adam_clip"]["us"], 3)
    row["lamb_ema_over_adam_clip_ema"] = round((row["ss_lamb_moments"]["us"] + row["ss_lamb_apply_ema"]["us"]) / row["ss_adam_clip_ema"]["us"], 3)
    row["a_a"] = round(row["ss_adam_clip_again"]["us"] / row["ss_adam_clip"]["us"], 3)
    return row


def steps(B, T, D, hw, C, a):
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, T, D, generator=g).cuda()
    R = torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    lengths = torch.full((B,), T, dtype=torch.int64).cuda()
    trainers = {}
    for key in ("plain", "lamb", "plain_again"):
        torch.manual_seed(0)
        trainers[key] = ss.Trainer(ss.BiGRUClassifier(D, C, use_roi=True).cuda().train(), dropout=True)
        if key == "lamb":
            trainers[key].enable_lamb()
    times = {k: [] for k in trainers}
    for rnd in range(-2, a.rounds):
        for key, tr in trainers.items():
            t = timed(lambda: tr.step(X, lengths, R, y), a.steps)
            if rnd >= 0:
                times[key].append(t)
    row = {"shape": dict(B=B, T=T, D=D, roi=list(hw), classes=C)}
    for key, ts in times.items():
        row[key + "_ms"] = round(statistics.median(ts), 4)
        row[key + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
    row["lamb_over_plain"] = round(row["lamb_ms"] / row["plain_ms"], 3)
    row["a_a"] = round(row["plain_again_ms"] / row["plain_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    L.load()
    out = {"kernels": {name: kernels(model, a) for name, model in models().items()},
           "steps": {name: steps(a=a, **shape) for name, shape in SHAPES.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
