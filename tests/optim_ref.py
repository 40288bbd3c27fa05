"""NumPy restatement of the flat-bucket optimiser step with a weight average (``ss_adam_clip_ema``), float64 throughout: the
global-norm clip of ``clip_grad_norm_`` folded into torch's default Adam, then ``ema = d * ema + (1 - d) * p_new``.  Test
infrastructure: ``tests/test_ema_resume_cpu.py`` checks it against ``torch.optim.Adam`` itself."""
import numpy as np


def f32_ulp(x):
    """Spacing of float32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def ema_expected(ema_old, p_new, decay):
    """What the kernel is asked to compute, in float64 on the float32 values it saw: ``d * ema_old + float32(1 - d) * p_new``
    with ``d = float32(decay)`` -> (expected, bound); the bound is 2 float32 ulp of ``max(|ema_old|, |p_new|)`` (two rounded
    products and one rounded sum, each at most half an ulp of that magnitude: 1.5 ulp, with or without contraction)."""
    d = np.float32(decay)
    omd = np.float32(1.0) - d
    ema_old, p_new = np.asarray(ema_old, np.float32), np.asarray(p_new, np.float32)
    e = np.float64(d) * ema_old.astype(np.float64) + np.float64(omd) * p_new.astype(np.float64)
    return e, 2.0 * f32_ulp(np.maximum(np.abs(ema_old), np.abs(p_new)))


def adam_clip_ema_step(p, g, m, v, ema, step, decay, lr=3e-4, max_norm=1.0, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """One step on float64 arrays, in place; -> the pre-clip gradient norm."""
    total = float(np.sqrt(np.sum(g * g))) * grad_scale
    g = g * (grad_scale * min(1.0, max_norm / (total + 1e-6)))
    m *= beta1
    m += (1.0 - beta1) * g
    v *= beta2
    v += (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    ema *= decay
    ema += (1.0 - decay) * p
    return total
