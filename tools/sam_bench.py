"""Time the three streams of the sharpness-aware step -- ss_sumsq_absw_f32, ss_sam_perturb (plain and adaptive),
ss_sam_restore_sumsq -- beside ss_sumsq_f32, ss_adam_clip and ss_adam_clip_ema on the flat buckets of BASELINE configs 2 and 5, and
a SAM step against the plain step at the config-2 and the shipped batch-16 shapes.

    python tools/sam_bench.py [--rounds 20] [--launches 50] [--steps 30]

One process, warm, HIP events.  Kernels: the entry points alternate in rounds of ``launches`` back-to-back launches on one stream,
each round between two events; the figure is the median over the rounds of (round time / launches), with the bytes each launch
must move (streams of the bucket x 4 n) and the rate that makes.  Steps: a plain trainer, a SAM trainer, an ASAM trainer and the
plain trainer again (the A/A window) take ``steps`` steps each per round on the same batch, dropout on; median ms per step."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import silent_speech_amd as ss  # noqa: E402
from silent_speech_amd import _lib as L  # noqa: E402

ADAM = (1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8)
RHO = 0.05
SHAPES = {"config2": dict(B=256, T=30, D=84, hw=(64, 64), C=5), "shipped_b16": dict(B=16, T=90, D=180, hw=(48, 96), C=10)}


def models():
    c2 = ss.BiGRUClassifier(84, 5, use_roi=True)
    c5 = ss.BiGRUClassifier(84, 100, use_roi=True, precision="bf16", roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96))
    return {"config2": c2, "config5": c5}


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / count


def kernels(model, a):
    n = model.flat_params.numel()
    g = torch.Generator().manual_seed(0)
    p, gr, m, ema, backup = (torch.randn(n, generator=g).cuda() for _ in range(5))
    gr *= 0.01
    v = torch.rand(n, generator=g).cuda() * 1e-4
    ssq, zf, zi = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    s, step = L.stream(), [0]
    P, G, M, V, E, B, S = (t.data_ptr() for t in (p, gr, m, v, ema, backup, ssq))

    def adam(name, *extra):
        def fn():
            step[0] += 1
            L.call(name, P, G, M, V, *extra[:1], n, S, *ADAM, step[0], *extra[1:], s)
        return fn

    def perturb(adaptive):  # (the gradient is put back by nobody: the launch moves the same bytes whatever it holds)
        return lambda: L.call("ss_sam_perturb", P, G, B, n, S, 1.0, RHO, adaptive, zf.data_ptr(), 1, zi.data_ptr(), 1, s)

    # name -> (launch, streams of the bucket it must move)
    windows = {"ss_sumsq_f32": (lambda: L.call("ss_sumsq_f32", G, n, S, s), 1),
               "ss_sumsq_absw_f32": (lambda: L.call("ss_sumsq_absw_f32", P, G, n, S, s), 2),
               "ss_sam_perturb": (perturb(0), 5),
               "ss_sam_perturb_adaptive": (perturb(1), 5),
               "ss_sam_restore_sumsq": (lambda: L.call("ss_sam_restore_sumsq", P, B, G, n, S, s), 3),
               "ss_adam_clip": (adam("ss_adam_clip"), 7),
               "ss_adam_clip_ema": (adam("ss_adam_clip_ema", E, 0.999), 9),
               "ss_sumsq_f32_again": (lambda: L.call("ss_sumsq_f32", G, n, S, s), 1)}
    times = {k: [] for k in windows}
    for rnd in range(-2, a.rounds):
        for key, (fn, _) in windows.items():
            t = timed(fn, a.launches) * 1e3
            if rnd >= 0:
                times[key].append(t)
    row = {"floats": n}
    for key, (_, streams) in windows.items():
        us = statistics.median(times[key])
        row[key] = {"us": round(us, 3), "us_min_max": [round(min(times[key]), 3), round(max(times[key]), 3)],
                    "mbytes": round(streams * 4 * n * 1e-6, 2), "gbytes_per_s": round(streams * 4 * n / us * 1e-3, 1)}
    return row


def steps(B, T, D, hw, C, a):
    g = torch.Generator().manual_seed(1)
    X = torch.randn(B, T, D, generator=g).cuda()
    R = torch.randint(0, 256, (B, T) + hw, generator=g, dtype=torch.uint8).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    lengths = torch.full((B,), T, dtype=torch.int64).cuda()
    trainers = {}
    for key, sam in (("plain", None), ("sam", (RHO, False)), ("asam", (10 * RHO, True)), ("plain_again", None)):
        torch.manual_seed(0)
        trainers[key] = ss.Trainer(ss.BiGRUClassifier(D, C, use_roi=True).cuda().train(), dropout=True)
        if sam is not None:
            trainers[key].enable_sam(*sam)
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
    row["sam_over_plain"] = round(row["sam_ms"] / row["plain_ms"], 3)
    row["asam_over_plain"] = round(row["asam_ms"] / row["plain_ms"], 3)
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
