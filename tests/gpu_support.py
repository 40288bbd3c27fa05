"""What the GPU test files share: the ``L`` and ``ss`` fixtures, the small device helpers, the synthetic clip directory of the
``fit`` tests, and the one spelling of the fused tail's argument list outside ``engine.tail_fwd``.

A plain module, imported like ``flat_ref`` or ``launch_trace``.  A fixture becomes visible to a test file by importing its name:
``from gpu_support import L, ss  # noqa: F401``; being module-scoped, each importing file gets its own instance."""
import os

import numpy as np
import pytest
import torch

WORDS = ["aura", "no", "yes"]
STASH = ("attn", "xhat", "rstd", "ln", "mid", "mid_d")


@pytest.fixture(scope="module")
def L():
    """``silent_speech_amd._lib`` with the library loaded."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from silent_speech_amd import _lib

    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def ss():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import silent_speech_amd as ss_

    return ss_


def cuda(t):
    return t.contiguous().cuda()


def sync():
    torch.cuda.synchronize()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def make_weights(g, C):
    """Class weights in [0.2, 3) with mean 1: one ``torch.rand(C)`` from ``g``."""
    w = torch.rand(C, generator=g) * 2.8 + 0.2
    return (w / w.mean()).float()


def write_clips(clip_dir, words, n=45, D=20, roi=(32, 32), frames=(14, 22), seed=0, counts=None):
    """The synthetic directory of the ``fit`` tests: separable 'words' (a constant offset per class in four features), ragged
    lengths in ``range(*frames)``, random ROI frames (none with ``roi=None``).  Clip k is word ``k % len(words)``; with ``counts``,
    ``counts[c]`` clips of word c in an order shuffled first.  tests/test_gpu_support_cpu.py pins the default's draws."""
    from silent_speech_amd import data as Dm

    rng = np.random.default_rng(seed)
    os.makedirs(clip_dir)
    if counts is None:
        labels = [k % len(words) for k in range(n)]
    else:
        labels = sum(([c] * m for c, m in enumerate(counts)), [])
        rng.shuffle(labels)
    for k, c in enumerate(labels):
        T = int(rng.integers(*frames))
        X = (0.05 * rng.normal(size=(T, D))).astype(np.float32)
        X[:, c * 4:c * 4 + 4] += 0.5
        r = rng.integers(0, 256, (T,) + roi, dtype=np.uint8) if roi else None
        Dm.save_clip(os.path.join(clip_dir, f"{k:03d}.npz"), X, np.arange(T), words[c], "me", np.arange(4), r)
    return clip_dir


def tail_call(L, name, P, h_d, len_d, y_d, dims, eps, norm, mix=(), soft=(), status=False, fill=3.0, drop=(0.0, 0, 0)):
    """ss_tail_fwd (``norm`` = (denom,)), ss_tail_fwd_w ((w, den)), ss_tail_fwd_mix ((denom, w, den), ``mix`` = (y_b, lam)) or
    ss_tail_fwd_kd (the same, and ``soft`` = (teacher, ld, alpha, tau)) on output buffers filled with ``fill``; loss and correct
    start at zero.  ``status``: call without the check and return the status under "status".  ``drop``: (p, seed, offset) of the dropout."""
    B, T, Dm, MID, C = dims
    f = lambda *s: torch.full(s, fill, device="cuda")  # noqa: E731
    out = dict(attn=f(B, T), xhat=f(B, Dm), rstd=f(B), ln=f(B, Dm), mid=f(B, MID), mid_d=f(B, MID), logits=f(B, C),
               d_logits=f(B, C), loss=torch.zeros(1, device="cuda"), correct=torch.zeros(1, device="cuda", dtype=torch.int32))
    args = (h_d.data_ptr(), len_d.data_ptr(), P["pool.score.weight"].data_ptr(), P["pool.score.bias"].data_ptr(),
            P["head.0.weight"].data_ptr(), P["head.0.bias"].data_ptr(), P["head.1.weight"].data_ptr(), P["head.1.bias"].data_ptr(),
            P["head.4.weight"].data_ptr(), P["head.4.bias"].data_ptr(), y_d.data_ptr(), *mix, B, T, Dm, MID, C, 1e-5, *drop, eps,
            *norm, *(out[k].data_ptr() for k in STASH + ("logits", "d_logits", "loss", "correct")), *soft, L.stream())
    if status:
        out["status"] = getattr(L.load(), name)(*args)
    else:
        L.call(name, *args)
    torch.cuda.synchronize()
    return out
