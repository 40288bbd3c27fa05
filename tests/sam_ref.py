"""NumPy restatement of the sharpness-aware step (``Trainer(sam_rho=)``: ``ss_sumsq_f32`` / ``ss_sumsq_absw_f32``,
``ss_sam_perturb``, ``ss_sam_restore_sumsq``, then the clip + Adam launch), float64 throughout, with the formulas of the widely
used torch SAM optimiser (``adaptive=True`` for ASAM, no ``eta``):

    s  = sqrt(sum g^2) * grad_scale                 or  sqrt(sum (|w| g)^2) * grad_scale        (adaptive)
    e  = rho * grad_scale * g / (s + 1e-12)         or  rho * grad_scale * w^2 * g / (s + 1e-12)
    g' = gradient at w + e;   w, m, v <- clip + Adam of ``optim_ref.adam_clip_ema_step`` on (w, g')

Test infrastructure: ``tests/test_sam_cpu.py`` checks it against a two-pass SAM written with torch autograd,
``clip_grad_norm_`` and ``torch.optim.Adam`` / ``AdamW`` without a GPU, ``tests/test_gpu_sam.py`` holds the kernels and the trainer
to it.  Error bounds count rounded float32 operations as ``flat_ref`` explains."""
import numpy as np

import flat_ref as FR
import optim_ref as OR
from optim_ref import f32_ulp

EPS = 1e-12


def sam_norm(w, g, adaptive, grad_scale=1.0):
    """The norm the perturbation is scaled by, on float64 arrays."""
    t = np.abs(w) * g if adaptive else g
    return float(np.sqrt(np.sum(t * t))) * grad_scale


def sam_perturbation(w, g, rho, adaptive, grad_scale=1.0):
    """``e``, on float64 arrays."""
    scale = rho * grad_scale / (sam_norm(w, g, adaptive, grad_scale) + EPS)
    return scale * g * (w * w) if adaptive else scale * g


def sam_step(p, grad_fn, rho, adaptive, update, grad_scale=1.0):
    """One step on the float64 array ``p``, in place: ``g = grad_fn(p)``, ``g' = grad_fn(p + e)``, then ``update(p, g')``, the
    caller's clip + Adam on the UNPERTURBED weights -> (g, e, g', what ``update`` returns)."""
    g = grad_fn(p)
    e = sam_perturbation(p, g, rho, adaptive, grad_scale)
    g2 = grad_fn(p + e)
    return g, e, g2, update(p, g2)


def adam_update(m, v, ema, step, decay=0.0, **adam):
    """``update`` of ``sam_step``: ``optim_ref.adam_clip_ema_step`` with these moments (and average) at this step."""
    return lambda p, g: OR.adam_clip_ema_step(p, g, m, v, ema, step, decay, **adam)


# ---------------------------------------------------------------------------------------------- what the kernels are held to
def perturb_scale(sumsq_f32, rho, grad_scale=1.0):
    """``rho * grad_scale / (sqrt(sumsq) * grad_scale + 1e-12)`` in float64 on the float32 arguments the kernel sees."""
    gs, r = float(np.float32(grad_scale)), float(np.float32(rho))
    return r * gs / (float(np.sqrt(np.float64(np.float32(sumsq_f32)))) * gs + float(np.float32(EPS)))


def perturb_expected(w, g, sumsq_f32, rho, adaptive, grad_scale=1.0):
    """``ss_sam_perturb``'s new weights evaluated in float64 on the float32 values the kernel sees (the arrays, the accumulated
    sumsq word, the float32 scalars) -> ``(want, bound)``.

    Bound, counted in rounded float32 operations (``flat_ref``; one more is added for the second-order terms of ``(1 + u)**k``):

      scale  sqrtf, * grad_scale, + 1e-12f (a sum of non-negative terms keeps the relative error), rho * grad_scale, the
             division                                                                                                  5
      e      plain:    scale * g -- the product, rounded on its own or fused into the sum behind it                    5 + 1 = 6
             adaptive: (scale * g) * (w * w) -- two more products, whichever way they are associated                   5 + 3 = 8
      w + e  the term e is off by at most (6 | 8) + 1 ulp of e; the sum rounds once more, by at most one ulp of the larger of
             |w| and |e|.  A kernel that fuses the last product into the sum (fma) only drops one of the roundings counted."""
    w, g = (np.asarray(a, np.float32).astype(np.float64) for a in (w, g))
    scale = perturb_scale(sumsq_f32, rho, grad_scale)
    e = scale * g * (w * w) if adaptive else scale * g
    k = (8 if adaptive else 6) + 1
    return w + e, k * f32_ulp(e) + f32_ulp(np.maximum(np.abs(w), np.abs(e)))


def sumsq_bound(n, want, extra_ops=0):
    """The float32 summation bound of ``sumsq_kernel``'s walk on ``n`` non-negative terms whose float64 sum is ``want``:
    ``k u / (1 - k u) * want`` with ``k = flat_ref.sumsq_chain(n)`` + ``extra_ops``.  ``ss_sumsq_absw_f32``: each term |w| g is a
    rounded product before it is squared -- relative error u on the term, 2 u on its square -- so ``extra_ops=2``."""
    k = FR.sumsq_chain(n) + extra_ops
    return k * FR.U / (1 - k * FR.U) * want
