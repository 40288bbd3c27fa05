"""Time the frozen-CNN training step against the full step, the one-off embedding pass and the embedded gather.

    python tools/finetune_bench.py [--rounds 12] [--steps 40] [--launches 200]

Two shapes: BASELINE config 2 (B = 256, T = 30, D = 84, 64 x 64 ROI, 5 classes) and the reference's shipped shape at its batch size
(B = 16, T = 90, D = 180, 48 x 96 ROI, 10 classes).  For each, a synthetic store of B full-length clips is written to a temporary
directory and uploaded; one planned batch stays resident, as pixels (X, R) and embedded (Z), and
  * ``Trainer.step(X, T, R, y)`` and ``Trainer(freeze_cnn=True).step_embedded(Z, T, y)`` alternate in rounds of ``steps`` steps, each
    round between two HIP events that end in a synchronise; the figure is the median over the rounds of round time / steps, with
    the minimum and the maximum beside it.  Two warm-up rounds of each come first.  The baseline is ``Trainer.step`` in the same
    process, not a number from another run;
  * ``store.embed(model)`` is timed the same way (one warm-up pass) and reported per 10 000 frames;
  * ``ss_batch_gather_z`` against ``ss_batch_gather_f32`` + ``ss_batch_gather_u8`` through the same maps, ``launches`` launches back
    to back per round: microseconds per launch, the bytes each must move (rows read and rows written; the maps are left out) and
    the rate that gives.
One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import silent_speech_amd as ss  # noqa: E402
from silent_speech_amd import _lib as L  # noqa: E402
from silent_speech_amd.data import NOISE_STD  # noqa: E402

SHAPES = {"config2": dict(B=256, T=30, D=84, hw=(64, 64), C=5), "shipped_b16": dict(B=16, T=90, D=180, hw=(48, 96), C=10)}


def write_clips(d, B, T, D, hw, C):
    rng = np.random.default_rng(0)
    files = []
    for k in range(B):
        f = os.path.join(d, f"{k:04d}.npz")
        np.savez(f, X=(0.3 * rng.normal(size=(T, D))).astype(np.float32), ts=np.arange(T), label="w%d" % (k % C), speaker="me",
                 idxs=np.arange(4), roi=rng.integers(0, 256, (T,) + hw, dtype=np.uint8))
        files.append(f)
    return files


def timed(fn, n):
    """ms per call of ``fn`` over ``n`` back-to-back calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, rounds, n, warmup=2):
    times = {k: [] for k in fns}
    for rnd in range(-warmup, rounds):
        for k, fn in fns.items():
            t = timed(fn, n)
            if rnd >= 0:
                times[k].append(t)
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}


def run_shape(name, B, T, D, hw, C, a):
    with tempfile.TemporaryDirectory() as d:
        store = ss.DeviceClipStore(write_clips(d, B, T, D, hw, C), {"w%d" % c: c for c in range(C)}, max_t=T)
    full, frozen = (ss.BiGRUClassifier(D, C, use_roi=True).cuda().train() for _ in range(2))
    frozen.load_state_dict(full.state_dict())
    store.embed(frozen)
    torch.cuda.synchronize()
    frames = store.R.shape[0]
    embed_ms = statistics.median(timed(lambda: store.embed(frozen), 1) for _ in range(5))
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    kw = dict(augment=True, rng="philox", seed=1, first_row=0)
    X, Tl, R, y = store.batch(idx, **kw)
    X, Tl, R, y = X.clone(), Tl.clone(), R.clone(), y.clone()
    Z = store.batch(idx, embedded=True, **kw)[0].clone()
    t_full, t_frozen = ss.Trainer(full), ss.Trainer(frozen, freeze_cnn=True)
    steps = alternate({"step": lambda: t_full.step(X, Tl, R, y), "step_embedded": lambda: t_frozen.step_embedded(Z, Tl, y)},
                      a.rounds, a.steps)
    store.check()  # (the frozen trainer has left the CNN alone)
    # the gathers, through the maps of the batch above
    xmap, nmap, rmap = store._plan_bufs[B][:3]
    rows, Eo, HW = B * T, store.E.shape[1], hw[0] * hw[1]
    Xo, Ro, Zo = torch.empty_like(X), torch.empty_like(R), torch.empty_like(Z)
    s = L.stream()
    g = alternate({
        "ss_batch_gather_z": lambda: L.call("ss_batch_gather_z", store.X.data_ptr(), D, xmap.data_ptr(), store.E.data_ptr(), Eo,
                                            rmap.data_ptr(), store.E0.data_ptr(), rows, nmap.data_ptr(), float(NOISE_STD), 1, 0, None, 1,
                                            Zo.data_ptr(), D + Eo, s),
        "ss_batch_gather_f32": lambda: L.call("ss_batch_gather_f32", store.X.data_ptr(), D, xmap.data_ptr(), rows, None, nmap.data_ptr(),
                                              float(NOISE_STD), 1, Xo.data_ptr(), s),
        "ss_batch_gather_u8": lambda: L.call("ss_batch_gather_u8", store.R.data_ptr(), HW, rmap.data_ptr(), rows, Ro.data_ptr(), s),
    }, a.rounds, a.launches)
    nbytes = {"ss_batch_gather_z": 2 * rows * (D + Eo) * 4, "ss_batch_gather_f32": 2 * rows * D * 4, "ss_batch_gather_u8": 2 * rows * HW}
    r3 = lambda v: round(v, 4)  # noqa: E731
    return {
        "shape": dict(B=B, T=T, D=D, roi=list(hw), classes=C),
        "ms_per_step": {k: dict(median=r3(v["median"]), min=r3(v["min"]), max=r3(v["max"])) for k, v in steps.items()},
        "frozen_over_full": round(steps["step_embedded"]["median"] / steps["step"]["median"], 4),
        "embed": dict(frames=frames, ms=r3(embed_ms), ms_per_10000_frames=r3(embed_ms * 10000 / frames)),
        "gather": {k: dict(us=round(v["median"] * 1e3, 2), us_min_max=[round(v["min"] * 1e3, 2), round(v["max"] * 1e3, 2)],
                           bytes=nbytes[k], gbytes_per_s=round(nbytes[k] / (v["median"] * 1e-3) * 1e-9, 1)) for k, v in g.items()},
        "batch_bytes_per_frame": dict(pixels=D * 4 + HW, embedded=(D + Eo) * 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    L.load()
    print(json.dumps({name: run_shape(name, a=a, **SHAPES[name]) for name in a.shapes.split(",")}))


if __name__ == "__main__":
    main()
