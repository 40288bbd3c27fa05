"""NumPy restatement of the layer-wise adaptive step LAMB (``ss_lamb_moments`` + ``ss_lamb_apply``; You et al., "Large Batch
Optimization for Deep Learning", ICLR 2020), float64 throughout: the global-norm clip of ``clip_grad_norm_``, Adam's moments with
bias correction, the weight decay inside the update, and one trust ratio per segment (a parameter tensor):

    g'   = g * coef                                   coef: the clip coefficient over the whole range (``flat_ref.clip_coef``)
    m    = beta1 m + (1 - beta1) g'                   v = beta2 v + (1 - beta2) g' g'
    u    = wd_s p + bc1 * m / (sqrt(v) * inv_sqrt_bc2 + eps)            bc1 = 1 / (1 - beta1^step)
    P_s  = sum p^2,  U_s = sum u^2 over segment s
    r_s  = sqrt(P_s / U_s) where the segment adapts and both sums are positive, else 1
    p    = p - (lr_s r_s) u

No clamp on |w|, no eta, no clipping of the ratio.  Test infrastructure: ``tests/test_lamb_cpu.py`` checks it against a
per-parameter LAMB written with torch, ``tests/test_gpu_lamb.py`` holds the kernels and the trainer to it.

Error bounds count rounded float32 operations as ``flat_ref`` explains (``u32 = 2**-24``; a term that went through ``k`` rounded
operations is off by at most ``k`` ulp of itself, one more for the second-order terms; a sum rounds by at most one ulp of its larger
term).  The kernels form ``u`` from the float32 ``m`` and ``v`` they store -- the apply pass reads them back -- so the bounds below
take those stored moments as inputs; that they are ``ss_adam_clip``'s bits is a test of its own."""
import numpy as np

import flat_ref as FR
from adamw_ref import per_element
from optim_ref import f32_ulp

U32 = FR.U


def segments(seg_end):
    """-> [(lo, hi)] of the segments ``[seg_end[s-1], seg_end[s])``."""
    return list(zip([0] + [int(e) for e in seg_end[:-1]], [int(e) for e in seg_end]))


# ------------------------------------------------------------------------------------------------ the step, scalars unrounded
def lamb_step(p, g, m, v, step, seg_end, seg_group, lr_scale, weight_decay, adapt, lr=3e-4, max_norm=1.0, beta1=0.9, beta2=0.999,
              eps=1e-8, grad_scale=1.0):
    """One step on float64 arrays, in place, every scalar unrounded -> (the pre-clip gradient norm, the ratio of every segment)."""
    total = float(np.sqrt(np.sum(g * g))) * grad_scale
    gc = g * (grad_scale * min(1.0, max_norm / (total + 1e-6)))
    m *= beta1
    m += (1.0 - beta1) * gc
    v *= beta2
    v += (1.0 - beta2) * gc * gc
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    u = per_element(seg_end, seg_group, np.asarray(weight_decay, np.float64)) * p + (m / bc1) / (np.sqrt(v) / np.sqrt(bc2) + eps)
    ratios = []
    for s, (lo, hi) in enumerate(segments(seg_end)):
        P, U = float(np.sum(p[lo:hi] ** 2)), float(np.sum(u[lo:hi] ** 2))
        r = float(np.sqrt(P / U)) if adapt[s] and P > 0.0 and U > 0.0 else 1.0
        p[lo:hi] -= lr * float(lr_scale[seg_group[s]]) * r * u[lo:hi]
        ratios.append(r)
    return total, ratios


# ---------------------------------------------------------------------------------------------- what the kernels are held to
def lamb_scalars(step, beta1=0.9, beta2=0.999, eps=1e-8):
    """The scalars the host code of the two entry points hands to the kernels, each exactly a float32: ``flat_ref.adam_scalars``'
    and ``bc1 = float32(1 / (1 - double(beta1)^step))``."""
    s = FR.adam_scalars(step, 0.0, beta1, beta2, eps)
    s["bc1"] = float(np.float32(1.0 / (1.0 - float(np.float32(beta1)) ** int(step))))
    return s


def direction_expected(p, m, v, step, seg_end, seg_group, weight_decay, beta1=0.9, beta2=0.999, eps=1e-8):
    """``u`` in float64 from the float32 arrays ``p`` and the STORED moments ``m``, ``v`` -> ``(u, bound, t)``, ``t = bc1 * quot``.

      denom  sqrtf (1), * inv_sqrt_bc2 (2), + eps: a sum of non-negative terms keeps the relative error (3)
      quot   the division                                                                                    4
      t      bc1 * quot, rounded on its own                                                                  5, + 1 second order = 6 ulp of t
      u      fmaf(wd, p, t): the product is exact inside the fma, the sum rounds once: one ulp of the larger of |wd p| and |t|."""
    s = lamb_scalars(step, beta1, beta2, eps)
    p, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, m, v))
    wd = per_element(seg_end, seg_group, [float(np.float32(w)) for w in weight_decay])
    t = s["bc1"] * (m / (np.sqrt(v) * s["inv_sqrt_bc2"] + s["eps"]))
    return wd * p + t, 6.0 * f32_ulp(t) + f32_ulp(np.maximum(np.abs(wd * p), np.abs(t))), t


def norms_expected(p, m, v, step, seg_end, seg_group, weight_decay, adapt, **adam):
    """Per segment: ``sqrt P``, ``sqrt U`` and the ratio in float64, and a bound for the float32 the kernel writes of each ->
    three pairs ``(want, bound)`` of arrays (n_seg,).

      P     every square p^2 is one rounded float32 product (relative error u32); the float64 sum of n_s such terms adds at most
            n_s 2^-53 relatively.  dP = P (u32 + n_s 2^-53).
      U     the kernel squares its own u, off from the float64 u by at most d = direction_expected's bound:
            dU = sum (2 |u| d + d^2) + U' (u32 + n_s 2^-53) with U' = sum (|u| + d)^2.
      sqrt  of the float64 sum, correctly rounded in double, then rounded to float32: the sum's interval taken through the root,
            plus one float32 ulp (half an ulp of the conversion, the rest for the double operations).
      ratio sqrt(P / U) over the same intervals -- sqrt((P + dP) / (U - dU)) and sqrt((P - dP) / (U + dU)) -- plus one float32 ulp;
            exactly 1, bound 0, where the segment does not adapt or a sum is zero (a sum of squares is zero only if every term is)."""
    u, d, _ = direction_expected(p, m, v, step, seg_end, seg_group, weight_decay, **adam)
    p = np.asarray(p, np.float32).astype(np.float64)
    out = [[], [], [], [], [], []]
    for s, (lo, hi) in enumerate(segments(seg_end)):
        k = (hi - lo) * 2.0 ** -53 + U32
        P, U = float(np.sum(p[lo:hi] ** 2)), float(np.sum(u[lo:hi] ** 2))
        dP = P * k
        dU = float(np.sum(2.0 * np.abs(u[lo:hi]) * d[lo:hi] + d[lo:hi] ** 2)) + float(np.sum((np.abs(u[lo:hi]) + d[lo:hi]) ** 2)) * k
        for X, dX, want, bound in ((P, dP, out[0], out[1]), (U, dU, out[2], out[3])):
            root = np.sqrt(X)
            want.append(root)
            bound.append(max(np.sqrt(X + dX) - root, root - np.sqrt(max(X - dX, 0.0))) + float(f32_ulp(root)))
        if adapt[s] and P > 0.0 and U > 0.0:
            r = np.sqrt(P / U)
            hi_r = np.sqrt((P + dP) / (U - dU)) if U > dU else np.inf
            out[4].append(r)
            out[5].append(max(hi_r - r, r - np.sqrt(max(P - dP, 0.0) / (U + dU))) + float(f32_ulp(r)))
        else:
            out[4].append(1.0)
            out[5].append(0.0)
    a = [np.asarray(x, np.float64) for x in out]
    return (a[0], a[1]), (a[2], a[3]), (a[4], a[5])


def group_lr(lr, lr_scale):
    """``lr_s = float32(double(lr) * double(scale))`` as the host code takes it -> a Python float."""
    return float(np.float32(float(np.float32(lr)) * float(np.float32(lr_scale))))


def apply_expected(p, m, v, ratio_f32, step, seg_end, seg_group, lr_scale, weight_decay, lr=3e-4, **adam):
    """``ss_lamb_apply``'s new weights in float64 from the float32 arrays it reads -- ``p``, the stored ``m`` and ``v``, the ratios in
    device memory -- and the float32 scalars -> ``(want, bound)``.

      step   lr_s * r_s: one rounded product                                                                1
      x      step * u: the product (2) -- or fused into the difference -- and u's own error, |step| d;  + 1 second order: 3 ulp of x
      p - x  rounds once: one ulp of the larger of |p| and |x|."""
    u, d, _ = direction_expected(p, m, v, step, seg_end, seg_group, weight_decay, **adam)
    p = np.asarray(p, np.float32).astype(np.float64)
    r = np.asarray(ratio_f32, np.float32).astype(np.float64)
    step_s = per_element(seg_end, list(range(len(seg_end))), [group_lr(lr, lr_scale[G]) * r[s] for s, G in enumerate(seg_group)])
    x = step_s * u
    return p - x, step_s * d + 3.0 * f32_ulp(x) + f32_ulp(np.maximum(np.abs(p), np.abs(x)))


def adam_from_moments_expected(p, m, v, step, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """``ss_adam_clip``'s new weights in float64 from ``p`` and ITS stored moments: ``p - step_size * m / (sqrt(v) inv_sqrt_bc2 +
    eps)`` -> ``(want, bound, t)``.  Five rounded operations into ``t`` (the three of the denominator, the division, the product) and
    one for the second order: 6 ulp of t, and one ulp of the larger of |p| and |t| for the difference.  LAMB with every ratio 1 and
    no decay computes ``p - lr * (bc1 * quot)`` instead: its float64 value differs by the roundings of ``step_size`` and ``bc1``,
    2 u32 |t| < 2 ulp of t, which the caller adds."""
    s = FR.adam_scalars(step, lr, beta1, beta2, eps)
    p, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, m, v))
    t = s["step_size"] * (m / (np.sqrt(v) * s["inv_sqrt_bc2"] + s["eps"]))
    return p - t, 6.0 * f32_ulp(t) + f32_ulp(np.maximum(np.abs(p), np.abs(t))), t
