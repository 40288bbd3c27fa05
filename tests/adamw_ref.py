"""NumPy restatement of the grouped AdamW step (``ss_adamw_clip_groups``), float64 throughout: the global-norm clip of
``clip_grad_norm_`` folded into torch's decoupled ``AdamW`` with a learning rate and a weight decay per parameter group.  Test
infrastructure: ``tests/test_adamw_groups_cpu.py`` checks it against ``torch.optim.AdamW`` with real param groups without a GPU,
``tests/test_gpu_adamw_groups.py`` holds the kernel to it.

One update rule (``_update``) serves two callers that differ in their scalars only: ``adamw_groups_step`` takes them unrounded
(torch's own arithmetic in another order) and ``adamw_groups_expected`` as the host code of the entry point hands them to the
kernel, each a float32 (``flat_ref.adam_scalars`` / ``flat_ref.clip_coef`` and ``group_scalars`` below)."""
import numpy as np

import flat_ref as FR
from optim_ref import f32_ulp


def per_element(seg_end, seg_group, values):
    """``values[seg_group[s]]`` on every element of segment ``s`` = ``[seg_end[s-1], seg_end[s])`` -> float64 array (seg_end[-1],)."""
    out, lo = np.empty(int(seg_end[-1])), 0
    for end, G in zip(seg_end, seg_group):
        out[lo:end] = values[G]
        lo = end
    return out


def group_scalars(lr, lr_scale, weight_decay, step, beta1=0.9):
    """The three scalars of a group as the host code of ``ss_adamw_clip_groups`` takes them, each exactly a float32:
    ``lr_G = float32(double(lr) * double(scale))``, ``step_size_G = float32(double(lr_G) / bc1)`` -- ``adam_scalars`` with
    ``lr_G`` for ``lr`` -- and ``decay_G = float32(1 - double(lr_G) * double(weight_decay))`` -> dict of Python floats."""
    lr_g = np.float32(float(np.float32(lr)) * float(np.float32(lr_scale)))
    return dict(lr=float(lr_g), step_size=FR.adam_scalars(step, lr=float(lr_g), beta1=beta1)["step_size"],
                decay=float(np.float32(1.0 - float(lr_g) * float(np.float32(weight_decay)))))


def _update(p, g, m, v, coef, decay, step_size, s):
    """p1 = p * decay;  m' = beta1 m + (1 - beta1) g coef;  v' = beta2 v + (1 - beta2) (g coef)^2;
    p' = p1 - step_size * m' / (sqrt(v') * inv_sqrt_bc2 + eps)  -> (p', m', v', the terms the error bounds are made of)."""
    gc = g * coef
    m_a, m_b = s["beta1"] * m, s["omb1"] * gc
    v_a, v_b = s["beta2"] * v, s["omb2"] * gc * gc
    m_new, v_new = m_a + m_b, v_a + v_b
    denom = np.sqrt(v_new) * s["inv_sqrt_bc2"] + s["eps"]
    p1, t = p * decay, step_size * (m_new / denom)
    return p1 - t, m_new, v_new, dict(m_a=m_a, m_b=m_b, v_a=v_a, v_b=v_b, denom=denom, p1=p1, t=t)


def adamw_groups_step(p, g, m, v, step, seg_end, seg_group, lr_scale, weight_decay, lr=3e-4, max_norm=1.0, beta1=0.9, beta2=0.999,
                      eps=1e-8, grad_scale=1.0):
    """One step on float64 arrays, in place, every scalar unrounded; -> the pre-clip gradient norm."""
    total = float(np.sqrt(np.sum(g * g))) * grad_scale
    coef = grad_scale * min(1.0, max_norm / (total + 1e-6))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    lr_g = lr * np.asarray(lr_scale, np.float64)
    s = dict(beta1=beta1, omb1=1.0 - beta1, beta2=beta2, omb2=1.0 - beta2, eps=eps, inv_sqrt_bc2=1.0 / np.sqrt(bc2))
    decay = per_element(seg_end, seg_group, 1.0 - lr_g * np.asarray(weight_decay, np.float64))
    p[:], m[:], v[:], _ = _update(p, g, m, v, coef, decay, per_element(seg_end, seg_group, lr_g / bc1), s)
    return total


def adamw_groups_expected(p, g, m, v, sumsq_f32, step, seg_end, seg_group, lr_scale, weight_decay, lr=3e-4, max_norm=1.0, beta1=0.9,
                          beta2=0.999, eps=1e-8, grad_scale=1.0):
    """One launch of ``ss_adamw_clip_groups`` evaluated in float64 on the float32 values the kernel sees (arrays ``p, g, m, v``,
    the accumulated ``sumsq`` word, the float32 scalars) -> ``(want, bound)``, two dicts with the keys "p", "m", "v".

    Bounds.  The kernel's m' and v' are ``adam_clip_kernel``'s expressions on the same operands, so their bounds are
    ``flat_ref.adam_clip_expected``'s: 10 ulp of the larger term of m', 17 ulp of the larger term of v'.  For p', that docstring
    counts 13 rounded operations into ``t = step_size * quotient`` -- the count does not depend on the value of the step size,
    so ``step_size_G`` takes its place unchanged -- one for the difference and one for the second order: 15 ulp of
    max(|p|, |t|), plus ``step_size * bound(m') / denominator`` for the error m' carries.  Here the minuend is no longer an input:
    ``p1 = p * decay_G`` is ONE more correctly rounded product (``__fmul_rn``; decay_G itself is the float32 the kernel is
    handed, it has no error), off by at most 1 ulp of p1.  So: 13 (t) + 1 (p1) + 1 (the difference) + 1 (second order) = 16 ulp
    of max(|p1|, |t|), plus ``step_size_G * bound(m') / denominator``.  With decay_G = 1 the product is exact and the bound
    is one ulp wider than it need be."""
    s = FR.adam_scalars(step, lr, beta1, beta2, eps)
    groups = [group_scalars(lr, sc, wd, step, beta1) for sc, wd in zip(lr_scale, weight_decay)]
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    step_size = per_element(seg_end, seg_group, [G["step_size"] for G in groups])
    decay = per_element(seg_end, seg_group, [G["decay"] for G in groups])
    p_new, m_new, v_new, x = _update(p, g, m, v, FR.clip_coef(sumsq_f32, grad_scale, max_norm), decay, step_size, s)
    m_bound = 10.0 * f32_ulp(np.maximum(np.abs(x["m_a"]), np.abs(x["m_b"])))
    v_bound = 17.0 * f32_ulp(np.maximum(x["v_a"], x["v_b"]))
    p_bound = 16.0 * f32_ulp(np.maximum(np.abs(x["p1"]), np.abs(x["t"]))) + step_size * m_bound / x["denom"]
    return dict(p=p_new, m=m_new, v=v_new), dict(p=p_bound, m=m_bound, v=v_bound)
