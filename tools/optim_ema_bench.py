"""Time ss_adam_clip against ss_adam_clip_ema, and ss_adamw_clip_groups (without and with the average, each model's two-group
no_decay() table) against both, on the flat buckets of BASELINE configs 2 and 5.

    python tools/optim_ema_bench.py [--rounds 20] [--launches 50]

One process, warm, HIP events: the entry points alternate in rounds of ``launches`` back-to-back launches on one stream,
each round between two events; the figure is the median over the rounds of (round time / launches).  By traffic the fused
kernel moves nine streams of the bucket against seven; the grouped launch moves what its ungrouped sibling moves, which is timed
twice per round: the second window is the A/A row."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import silent_speech_amd as ss  # noqa: E402
from silent_speech_amd import _lib as L  # noqa: E402
from silent_speech_amd.train import SegmentTable  # noqa: E402

ADAM = (1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8)


def models():
    c2 = ss.BiGRUClassifier(84, 5, use_roi=True)
    c5 = ss.BiGRUClassifier(84, 100, use_roi=True, precision="bf16", roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96))
    return {"config2": c2, "config5": c5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    L.load()
    out = {}
    for name, model in models().items():
        n = model.flat_params.numel()
        table = SegmentTable(model, [ss.no_decay()], 1e-2)  # the model's real two-group table: biases and LayerNorm undecayed
        g = torch.Generator().manual_seed(0)
        p, gr, m, ema = (torch.randn(n, generator=g).cuda() for _ in range(4))
        gr *= 0.01
        v = torch.rand(n, generator=g).cuda() * 1e-4
        ssq = torch.zeros(1, device="cuda")
        L.call("ss_sumsq_f32", gr.data_ptr(), n, ssq.data_ptr(), L.stream())
        s = L.stream()

        def plain(step):
            L.call("ss_adam_clip", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, ssq.data_ptr(), *ADAM, step, s)

        def fused(step):
            L.call("ss_adam_clip_ema", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(), n, ssq.data_ptr(),
                   *ADAM, step, 0.999, s)

        def grouped(step, e=None):
            L.call("ss_adamw_clip_groups", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), e, n, ssq.data_ptr(), *ADAM, step,
                   0.999, *table.args, s)

        # every round times each window once, in this order; the *_again windows are the A/A rows: the ungrouped kernels against
        # themselves in the same run, the margin the grouped launch is read against
        windows = (("ss_adam_clip", plain), ("ss_adamw_clip_groups", grouped), ("ss_adam_clip_again", plain),
                   ("ss_adam_clip_ema", fused), ("ss_adamw_clip_groups_ema", lambda st: grouped(st, ema.data_ptr())),
                   ("ss_adam_clip_ema_again", fused))
        times = {key: [] for key, _ in windows}
        step = 0
        for rnd in range(-2, a.rounds):  # two warm-up rounds of each
            for key, fn in windows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    step += 1
                    fn(step)
                e1.record()
                e1.synchronize()
                if rnd >= 0:
                    times[key].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        row = {"floats": n, "segments": len(table.seg_end), "groups": len(table.lr_scale)}
        for key, ts in times.items():
            row[key + "_us"] = round(statistics.median(ts), 3)
            row[key + "_us_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        row["ratio"] = round(row["ss_adam_clip_ema_us"] / row["ss_adam_clip_us"], 3)
        row["grouped_ratio"] = {"plain": round(row["ss_adamw_clip_groups_us"] / row["ss_adam_clip_us"], 3),
                                "plain_a_a": round(row["ss_adam_clip_again_us"] / row["ss_adam_clip_us"], 3),
                                "ema": round(row["ss_adamw_clip_groups_ema_us"] / row["ss_adam_clip_ema_us"], 3),
                                "ema_a_a": round(row["ss_adam_clip_ema_again_us"] / row["ss_adam_clip_ema_us"], 3)}
        streams = {"ss_adam_clip": 7, "ss_adamw_clip_groups": 7, "ss_adam_clip_ema": 9, "ss_adamw_clip_groups_ema": 9}
        row["gbytes_per_s"] = {key: round(k * 4 * n / row[key + "_us"] * 1e-3, 1) for key, k in streams.items()}
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
