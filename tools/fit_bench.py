"""What the training loop of ``harness.fit`` costs around the step: batches planned on the host (``rng="device"``) against
batches planned by the kernel (``rng="philox"``), with ``Trainer.step`` on a resident batch as the yardstick.

    python tools/fit_bench.py [--steps 200] [--windows 5] [--warmup 20] [--mixup]

One JSON line.  Per shape (config 2: B=256, T=30, D=84, 64x64 ROI; shipped: B=16, T=90, D=180, 48x96 ROI):
  clips_per_s.{resident, host_plan, device_plan, device_plan_policy, device_plan_policy_masks}
                                                  median (min, max) over the windows; the five loops alternate window by window
                                                  inside this one process, every window ends in a device synchronise.
                                                  device_plan_policy: ``batch(policy=AugmentPolicy.lineage(roi_shift_prob=0.5,
                                                  roi_shift_max=(4, 2)))`` -- time warp, scale jitter and ROI shift
                                                  device_plan_policy_masks: the same policy with the three masks on (time mask 0.5 / 8
                                                  frames, feature band 0.5 / 16 columns, ROI cutout 0.5 / 16 x 16 pixels)
  policy_of_device_plan                           median device_plan_policy / median device_plan of this run, and device_plan's own
                                                  (max - min) / median beside it: the yardstick is this run's device_plan loop
  masks_of_policy                                 median device_plan_policy_masks / median device_plan_policy of this run, and
                                                  device_plan_policy's own (max - min) / median beside it
  clips_per_s.device_plan_policy_mixup, mixup_of_policy, mixup_blend
                                                  (--mixup) one more loop in the same alternation: device_plan_policy's policy with
                                                  ``mixup_prob=1.0`` and ``Trainer.step(mix=store.mix[:2])``; its median over
                                                  device_plan_policy's of this run with that loop's spread beside it; and what the
                                                  blend launch moves -- two reads and one write of X and R -- over its kernels_ms, in
                                                  bytes per second
  clips_per_s.resident_weighted, class_weight_us  (--class-weights) the resident loop through ``Trainer(class_weights=)``, a fourth loop
                                                  in the same alternation, and what its step costs more than the unweighted one
                                                  (the one ``ss_class_weight_sum`` launch): median over the windows of the difference
                                                  in us per step between neighbouring windows
  assemble_ms.{host_plan, device_plan, device_plan_policy, device_plan_policy_masks}
                                                  the batch() calls alone (no step), same alternation: ms per batch
  enqueue_ms.{host_plan, device_plan}             host wall time of one batch() call while the GPU is idle (no synchronise
                                                  inside the timed region: what the call costs the Python thread)
  kernels_ms.{host_plan, device_plan, device_plan_policy, device_plan_policy_masks}
                                                  HIP-event time per launch of the kernels batch() enqueues (L.PROFILE); the policy's
                                                  are ss_batch_plan_aug, ss_batch_gather_f32_aug and ss_batch_gather_u8_shift, the
                                                  masks add ss_batch_plan_mask and ss_batch_mask_apply
  validation_ms.{evaluate, evaluate_device}       (config2 only, --eval-clips N, 0 = skip) one validation pass over N clips in batches of
                                                  B: ``harness.evaluate`` (two read-backs per batch, confusions counted on the host)
                                                  against ``harness.evaluate_device`` (``ss_eval_accum``, one read at the end);
                                                  wall ms per pass, the two alternating pass by pass
The synthetic clip directory is the one ``bench.py --mode assemble`` builds: 64 clips, ragged lengths in [T, T + 8).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import silent_speech_amd as ss  # noqa: E402
from silent_speech_amd import _lib as L  # noqa: E402
from silent_speech_amd import data as Dm  # noqa: E402

SHAPES = {"config2": dict(B=256, T=30, D=84, roi=(64, 64), C=5), "shipped": dict(B=16, T=90, D=180, roi=(48, 96), C=10)}
SEED = 1


def make_store(T, D, roi, C, dev, n_clips=64):
    rs = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k in range(n_clips):
            Tk = int(rs.integers(T, T + 8))
            p = os.path.join(tmp, f"c{k}.npz")
            Dm.save_clip(p, rs.normal(size=(Tk, D)).astype("float32"), range(Tk), "w%d" % (k % C), "me", range(4),
                         rs.integers(0, 256, (Tk,) + tuple(roi), dtype="uint8"))
            files.append(p)
        return ss.DeviceClipStore(files, {"w%d" % c: c for c in range(C)}, max_t=T, device=dev)


def summary(vals, digits=1):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def time_validation(model, B, T, D, roi, C, n_clips, windows, dev):
    from silent_speech_amd import harness as Hn

    store = make_store(T, D, roi, C, dev, n_clips)
    passes = {"evaluate": lambda: Hn.evaluate(model, store, batch_size=B), "evaluate_device": lambda: Hn.evaluate_device(model, store, batch_size=B)}
    ms = {k: [] for k in passes}
    for it in range(2 + max(3, windows)):  # two warm-up rounds, then alternate
        for k, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= 2:
                ms[k].append(1000 * (time.perf_counter() - t0))
    model.train()
    return {"clips": n_clips, "batches": -(-n_clips // B), **{k: summary(v, 3) for k, v in ms.items()}}


def run_shape(name, B, T, D, roi, C, steps, windows, warmup, dev, eval_clips=0, class_weights=False, mixup=False):
    store = make_store(T, D, roi, C, dev)
    model = ss.BiGRUClassifier(D, C, use_roi=True, roi_emb=32, hidden=192).to(dev).train()
    trainer = ss.Trainer(model)
    # (a second trainer on the same model: its own Adam moments, the same buckets and workspaces)
    weighted = ss.Trainer(model, class_weights=np.linspace(0.5, 1.5, C)) if class_weights else None
    gen = np.random.default_rng(SEED)
    host_order = [[int(v) for v in gen.integers(0, len(store), B)] for _ in range(steps)]  # drawn outside the timed loops
    dev_order = store.sample_epoch(num_samples=B * steps, seed=SEED)
    resident = tuple(t.clone() for t in store.batch(host_order[0], augment=True, rng="device", generator=gen))
    row = [0]  # rows drawn so far: no two device-planned batches of the run share draws

    def host_batch(i):
        return store.batch(host_order[i], augment=True, rng="device", generator=gen)

    def dev_batch(i):
        row[0] += B
        return store.batch(dev_order[i * B:(i + 1) * B], augment=True, rng="philox", seed=SEED, first_row=row[0])

    policy = ss.AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(4, 2))

    def policy_batch(i):
        row[0] += B
        return store.batch(dev_order[i * B:(i + 1) * B], augment=True, rng="philox", seed=SEED, first_row=row[0], policy=policy)

    masks = ss.AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(4, 2), time_mask_prob=0.5, time_mask_max=8, feat_mask_prob=0.5,
                                     feat_mask_max=16, cutout_prob=0.5, cutout_max=(16, 16))

    def masks_batch(i):
        row[0] += B
        return store.batch(dev_order[i * B:(i + 1) * B], augment=True, rng="philox", seed=SEED, first_row=row[0], policy=masks)

    mixed = ss.AugmentPolicy.lineage(roi_shift_prob=0.5, roi_shift_max=(4, 2), mixup_prob=1.0)

    def mixup_batch(i):
        row[0] += B
        return store.batch(dev_order[i * B:(i + 1) * B], augment=True, rng="philox", seed=SEED, first_row=row[0], policy=mixed)

    def window(make_batch, step, n):
        tr = weighted if step == "weighted" else trainer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            Xb, Tb, Rb, yb = make_batch(i % steps) if make_batch else resident
            if step:
                tr.step(Xb, Tb, Rb, yb, mix=store.mix[:2] if make_batch is mixup_batch else None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    loops = {"resident": (None, True), "host_plan": (host_batch, True), "device_plan": (dev_batch, True),
             "device_plan_policy": (policy_batch, True), "device_plan_policy_masks": (masks_batch, True)}
    if weighted is not None:
        loops = {"resident": (None, True), "resident_weighted": (None, "weighted"), **loops}
    asm = {"host_plan": (host_batch, False), "device_plan": (dev_batch, False), "device_plan_policy": (policy_batch, False),
           "device_plan_policy_masks": (masks_batch, False)}
    if mixup:
        loops["device_plan_policy_mixup"] = (mixup_batch, True)
        asm["device_plan_policy_mixup"] = (mixup_batch, False)
    for mk, st in list(loops.values()) + list(asm.values()):  # every shape and code path of the timed windows, warmed up
        window(mk, st, warmup)
    rate = {k: [] for k in loops}
    asm_ms = {k: [] for k in asm}
    for _ in range(windows):  # alternate: a drift of the box hits every loop alike
        for k, (mk, st) in loops.items():
            rate[k].append(B * steps / window(mk, st, steps))
        for k, (mk, st) in asm.items():
            asm_ms[k].append(1000 * window(mk, st, steps) / steps)
    enq, kern = {}, {}
    for k, (mk, _) in asm.items():
        per_call = []
        for _ in range(windows):
            torch.cuda.synchronize()  # GPU idle: the time below is the host's alone
            t0 = time.perf_counter()
            for i in range(20):
                mk(i)
            per_call.append(1000 * (time.perf_counter() - t0) / 20)
            torch.cuda.synchronize()
        enq[k] = summary(per_call, 4)
        L.PROFILE = {}
        for i in range(min(steps, 50)):
            mk(i)
        torch.cuda.synchronize()
        prof, L.PROFILE = L.PROFILE, None
        kern[k] = {tag: round(sum(a.elapsed_time(b) for a, b in evs) / len(evs), 4) for tag, evs in prof.items()}
    store.check()
    med = {k: statistics.median(v) for k, v in rate.items()}
    if weighted is not None:
        extra_us = [1e6 * B * (1 / w - 1 / u) for u, w in zip(rate["resident"], rate["resident_weighted"])]
    extra = {} if not (eval_clips and name == "config2") else {"validation_ms": time_validation(model, B, T, D, roi, C, eval_clips, windows, dev)}
    if weighted is not None:
        extra["class_weight_us"] = summary(extra_us, 2)
    if mixup:
        moved = 3 * B * store.max_t * (4 * D + roi[0] * roi[1])
        blend_ms = kern["device_plan_policy_mixup"]["ss_batch_mixup"]
        extra["mixup_of_policy"] = {"ratio": round(med["device_plan_policy_mixup"] / med["device_plan_policy"], 4),
                                    "device_plan_policy_spread": round((max(rate["device_plan_policy"]) - min(rate["device_plan_policy"]))
                                                                       / med["device_plan_policy"], 4)}
        extra["mixup_blend"] = {"bytes": moved, "ms": blend_ms, "bytes_per_s": round(moved / (1e-3 * blend_ms), 0)}
    return {**extra, "shape": dict(B=B, T=T, D=D, roi="%dx%d" % tuple(roi), classes=C),
            "clips_per_s": {k: summary(v) for k, v in rate.items()},
            "of_resident": {k: round(med[k] / med["resident"], 4) for k in ("host_plan", "device_plan", "device_plan_policy",
                                                                            "device_plan_policy_masks")},
            "policy_of_device_plan": {"ratio": round(med["device_plan_policy"] / med["device_plan"], 4),
                                      "device_plan_spread": round((max(rate["device_plan"]) - min(rate["device_plan"])) / med["device_plan"], 4)},
            "masks_of_policy": {"ratio": round(med["device_plan_policy_masks"] / med["device_plan_policy"], 4),
                                "device_plan_policy_spread": round((max(rate["device_plan_policy"]) - min(rate["device_plan_policy"]))
                                                                   / med["device_plan_policy"], 4)},
            "assemble_ms": {k: summary(v, 4) for k, v in asm_ms.items()},
            "enqueue_ms": enq, "kernels_ms": kern}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per loop (alternating)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", default="config2,shipped")
    ap.add_argument("--class-weights", action="store_true", help="also time the resident loop with class weights")
    ap.add_argument("--mixup", action="store_true", help="also time the device-planned policy loop with mixup on")
    ap.add_argument("--eval-clips", type=int, default=1024, help="clips of the timed validation pass (config2; 0 = skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda")
    out = {"metric": "clips/s of the training loop: resident batch, host-planned batches, device-planned batches, device-planned with an AugmentPolicy, the same with its masks on",
           "steps_per_window": args.steps, "windows": args.windows, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name in args.shapes.split(","):
        out[name] = run_shape(name, steps=args.steps, windows=args.windows, warmup=args.warmup, dev=dev, eval_clips=args.eval_clips, class_weights=args.class_weights,
                              mixup=args.mixup,
                              **SHAPES[name])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
