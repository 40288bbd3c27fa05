"""Time what knowledge distillation touches, at BASELINE config 2 shapes (B = 256, T = 30, 84 features + 64x64 ROI, 2-layer
BiGRU(192), 5 words):

  * ``ss_tail_fwd`` of this tree against ``ss_tail_fwd`` of a library built from the parent commit (``--parent-lib``: a
    ``libss_hotpath.so`` of that commit, e.g. from a second work tree; without it these windows are left out) -- the new kernel
    argument must not move the existing instantiations;
  * ``ss_tail_fwd_kd`` (tau = 2, alpha = 0.5) against ``ss_tail_fwd``;
  * a whole ``Trainer.step`` without a teacher against a step with a same-architecture teacher's forward in front of it.

    python tools/distill_bench.py [--rounds 20] [--launches 50] [--steps 10] [--parent-lib PATH]

One process, warm, HIP events, as tools/optim_ema_bench.py: the windows alternate in rounds, each window ``launches`` back-to-back
launches (or ``steps`` steps) between two events; the figure is the median over the rounds.  Every reference window is timed twice
per round: the second one is its A/A row, the margin the others are read against.  Prints one JSON line."""
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

B, T, X_DIM, WORDS, ROI = 256, 30, 84, 5, (64, 64)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n  # us per call


def measure(windows, rounds, n):
    times = {key: [] for key, _ in windows}
    for rnd in range(-2, rounds):  # two warm-up rounds of each
        for key, fn in windows:
            t = window(fn, n)
            if rnd >= 0:
                times[key].append(t)
    row = {}
    for key, ts in times.items():
        row[key + "_us"] = round(statistics.median(ts), 3)
        row[key + "_us_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.load()
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.ss_tail_fwd.argtypes, parent.ss_tail_fwd.restype = L.SIGNATURES["ss_tail_fwd"], C.c_int
        assert not hasattr(parent, "ss_tail_fwd_kd"), "--parent-lib already has ss_tail_fwd_kd: not the parent commit's library"
    g = torch.Generator().manual_seed(0)
    model = ss.BiGRUClassifier(X_DIM, WORDS, use_roi=True).cuda().train()
    P = model._param_dict()
    D, MID = 2 * model.cfg.hidden, model.cfg.head_mid
    f = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    h = torch.randn(B, T, D, generator=g).cuda()
    lens = torch.randint(T // 2, T + 1, (B,), generator=g, dtype=torch.int32).cuda()
    y = torch.randint(0, WORDS, (B,), generator=g).cuda()
    t_logits = (torch.randn(B, WORDS, generator=g) * 3).cuda()
    outs = [f(B, T), f(B, D), f(B), f(B, D), f(B, MID), f(B, MID), f(B, WORDS), f(B, WORDS), torch.zeros(1, device="cuda"),
            torch.zeros(1, device="cuda", dtype=torch.int32)]
    head = [h.data_ptr(), lens.data_ptr()] + [P[k].data_ptr() for k in ("pool.score.weight", "pool.score.bias", "head.0.weight",
                                                                        "head.0.bias", "head.1.weight", "head.1.bias",
                                                                        "head.4.weight", "head.4.bias")]
    dims = [B, T, D, MID, WORDS, model.cfg.ln_eps, model.cfg.head_dropout, 1, 7 << 40, 0.05, float(B)]
    out_ptrs = [t.data_ptr() for t in outs]
    s = L.stream()
    plain_args = (*head, y.data_ptr(), *dims, *out_ptrs, s)
    kd_args = (*head, y.data_ptr(), None, None, *dims, None, None, *out_ptrs, t_logits.data_ptr(), WORDS, 0.5, 2.0, s)

    def check(st):
        assert st == 0, st

    branch = lambda: check(lib.ss_tail_fwd(*plain_args))  # noqa: E731
    kd = lambda: check(lib.ss_tail_fwd_kd(*kd_args))  # noqa: E731
    windows = [("ss_tail_fwd", branch)]
    if parent is not None:
        old = lambda: check(parent.ss_tail_fwd(*plain_args))  # noqa: E731
        windows += [("parent_ss_tail_fwd", old)]
    windows += [("ss_tail_fwd_kd", kd), ("ss_tail_fwd_again", branch)]
    if parent is not None:
        windows += [("parent_ss_tail_fwd_again", old)]
    out = {"shape": dict(B=B, T=T, D=D, MID=MID, C=WORDS), "rounds": a.rounds, "launches": a.launches, "steps": a.steps}
    tail = measure(windows, a.rounds, a.launches)
    tail["kd_over_plain"] = round(tail["ss_tail_fwd_kd_us"] / tail["ss_tail_fwd_us"], 4)
    tail["plain_a_a"] = round(tail["ss_tail_fwd_again_us"] / tail["ss_tail_fwd_us"], 4)
    if parent is not None:
        tail["branch_over_parent"] = round(tail["ss_tail_fwd_us"] / tail["parent_ss_tail_fwd_us"], 4)
        tail["parent_a_a"] = round(tail["parent_ss_tail_fwd_again_us"] / tail["parent_ss_tail_fwd_us"], 4)
    out["tail"] = tail

    # ---- a whole step, without and with a same-architecture teacher's forward
    teacher = ss.BiGRUClassifier(X_DIM, WORDS, use_roi=True).cuda().eval()
    trainer = ss.Trainer(model)
    X = (torch.randn(B, T, X_DIM, generator=g) * 0.7).cuda()
    R = torch.randint(0, 256, (B, T) + ROI, generator=g, dtype=torch.uint8).cuda()
    lengths = lens.long()

    def plain_step():
        trainer.step(X, lengths, R, y)

    def kd_step():
        with torch.no_grad():
            t = teacher(X, lengths, R)
        trainer.step(X, lengths, R, y, teacher_logits=t)

    step = measure([("step", plain_step), ("step_with_teacher", kd_step), ("step_again", plain_step)], max(3, a.rounds // 2), a.steps)
    step["teacher_over_plain"] = round(step["step_with_teacher_us"] / step["step_us"], 4)
    step["plain_a_a"] = round(step["step_again_us"] / step["step_us"], 4)
    out["step"] = step
    print(json.dumps(out))


if __name__ == "__main__":
    main()
