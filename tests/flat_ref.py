"""Host references of the flat streaming kernels (csrc/optim.hip, csrc/step_helpers.hip, csrc/pool_head.hip) in NumPy, float64
or integers: the clip + Adam step (``ss_adam_clip``, ``ss_adam_clip_ema``), the dropout stream (``ss_dropout``), softmax + top-k
(``ss_softmax_topk``) and the list of frames that belong to a clip (``ss_train_prologue``, ``ss_roi_active_frames``).  Test
infrastructure: ``tests/test_flat_ref_cpu.py`` checks it against torch and Random123's known answers without a GPU,
``tests/test_gpu_flat_kernels.py`` holds the kernels to it.

Error bounds count rounded float32 operations.  ``u = 2**-24``; one correctly rounded operation (add, multiply, fused
multiply-add, divide, ``sqrtf``: hipcc rounds float32 divisions and square roots correctly by default) has a relative error of
at most ``u``, and ``u * |x| < ulp(x)`` (``optim_ref.f32_ulp``), so a term ``x`` that has gone through ``k`` such operations is
off by at most ``k`` ulp of ``x``, and the rounding of a sum of two terms by at most one ulp of the larger one.  Contraction
(``-ffp-contract=on``) fuses a product into the sum behind it and only removes roundings."""
import numpy as np

import batch_plan_ref as P
from optim_ref import f32_ulp

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_scalars(step, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """The scalars as the host code of ``ss_adam_clip`` hands them to the kernel: ``beta`` as float32, ``1 - beta`` taken in
    float32, ``step_size = float32(lr / bc1)`` and ``inv_sqrt_bc2 = float32(1 / sqrt(bc2))`` from double ``pow`` of the float32
    betas -> dict of Python floats (each exactly a float32)."""
    b1, b2, lr32 = np.float32(beta1), np.float32(beta2), np.float32(lr)
    bc1, bc2 = 1.0 - float(b1) ** int(step), 1.0 - float(b2) ** int(step)
    return dict(beta1=float(b1), omb1=float(np.float32(1.0) - b1), beta2=float(b2), omb2=float(np.float32(1.0) - b2),
                eps=float(np.float32(eps)), step_size=float(np.float32(float(lr32) / bc1)),
                inv_sqrt_bc2=float(np.float32(1.0 / np.sqrt(bc2))))


def clip_coef(sumsq_f32, grad_scale=1.0, max_norm=1.0):
    """``grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))`` in float64 on the float32 arguments."""
    gs, mn = float(np.float32(grad_scale)), float(np.float32(max_norm))
    total = float(np.sqrt(np.float64(np.float32(sumsq_f32)))) * gs
    return gs * min(1.0, mn / (total + float(np.float32(1e-6))))


def adam_clip_expected(p, g, m, v, sumsq_f32, step, lr=3e-4, max_norm=1.0, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """One step of ``adam_clip_kernel`` evaluated in float64 on the float32 values the kernel sees (arrays ``p, g, m, v``, the
    accumulated ``sumsq`` word, the scalars of ``adam_scalars``) -> ``(want, bound)``, two dicts with the keys "p", "m", "v".

        coef  = grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))
        g'    = g * coef
        m'    = beta1 * m + (1 - beta1) * g'
        v'    = beta2 * v + (1 - beta2) * g' * g'
        p'    = p - step_size * (m' / (sqrt(v') * inv_sqrt_bc2 + eps))

    Bounds, counted in rounded operations as the module docstring explains (each count has one more added for the second-order
    terms of ``(1 + u)**k``):

      coef   sqrtf, * grad_scale, + 1e-6f, the division, * grad_scale (``fminf`` is exact, and 1-Lipschitz)           5
      g'     coef's 5 and the product                                                                                6
      m'     beta1 * m: 1.  (1 - beta1) * g': 6 + 1 = 7.  The sum: 1.  9 + 1 = 10 ulp of the larger of the two terms.
      v'     beta2 * v: 1.  ((1 - beta2) * g') * g': 6 + 6 + 2 = 14.  The sum: 1.  16 + 1 = 17 ulp of the larger term.
      p'     both terms of v' are positive, so v' is off by at most 16 u relatively; sqrtf halves that and rounds (9), the
             product with inv_sqrt_bc2 (10), + eps, again a sum of positive terms (11); the quotient inherits those 11, rounds
             once (12), and carries the absolute error of m' divided by the denominator -- m' is a sum of terms of either
             sign, its relative error has no bound; the product with step_size (13).  With t = step_size * quotient:
             13 ulp of t, one for the difference, one for the second order: 15 ulp of max(|p|, |t|), plus
             step_size * bound(m') / denominator."""
    s = adam_scalars(step, lr, beta1, beta2, eps)
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    gc = g * clip_coef(sumsq_f32, grad_scale, max_norm)
    m_a, m_b = s["beta1"] * m, s["omb1"] * gc
    m_new = m_a + m_b
    m_bound = 10.0 * f32_ulp(np.maximum(np.abs(m_a), np.abs(m_b)))
    v_a, v_b = s["beta2"] * v, s["omb2"] * gc * gc
    v_new = v_a + v_b
    v_bound = 17.0 * f32_ulp(np.maximum(v_a, v_b))
    denom = np.sqrt(v_new) * s["inv_sqrt_bc2"] + s["eps"]
    t = s["step_size"] * (m_new / denom)
    p_new = p - t
    p_bound = 15.0 * f32_ulp(np.maximum(np.abs(p), np.abs(t))) + s["step_size"] * m_bound / denom
    return dict(p=p_new, m=m_new, v=v_new), dict(p=p_bound, m=m_bound, v=v_bound)


def optimiser_case(n, seed):
    """Inputs of one optimiser step on the host, float32 arrays: weights, a gradient, nonzero moments (the recipe of
    ``optimiser_inputs`` in tests/test_gpu_ema_resume.py, in NumPy so that the CPU suite can make them too)."""
    rng = np.random.default_rng(seed)
    p, g, m = rng.standard_normal(n), 0.05 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)
    v = 1e-4 * rng.random(n) + 1e-8
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


# ------------------------------------------------------------------------------------------- exact inputs of ss_sumsq_f32
# the tail alone; both sides of the capped grid's sweep (256 x 256 x 4); the first quad at which the four-loads-in-flight loop
# runs (n / 4 > 3 x 65 536) and the sizes around it; that loop + remainder + n & 3 = 3; several trips of it
SUMSQ_NS = [1, 3, 262143, 262144, 262149, 786432, 786436, 786439, 1048583, 1310723, 3145731]
SUMSQ_TWICE_MAX_N = 1310723  # up to here the test adds a second call onto the accumulated word


def sumsq_exact_input(n):
    """Random integers in {0, 1, 2} as float32: every square and every partial sum of squares is an integer, and while the
    total stays below 2**24 every float32 addition on the way is exact in whatever order the lanes, waves and atomics add."""
    return np.random.default_rng(1000 + n).integers(0, 3, n).astype(np.float32)


def sumsq_grid(n):
    """-> (workgroups, quads a sweep of the grid covers) of ``ss_sumsq_f32``."""
    blocks = min(max(((n >> 2) + 255) // 256, 1), 256)
    return blocks, blocks * 256


def sumsq_chain(n):
    """Length of the longest chain of rounded operations one term of ``sumsq_kernel`` goes through, from n and the grid: its own
    square (1); the sums inside an unrolled trip -- three inside its quad, three between the four quads -- (6) or inside a
    remainder trip (3); one ``acc +=`` per trip of thread 0, which takes the most; the tail's ``acc +=``; the wave tree (4 DPP
    levels + 2); the three adds over the four waves; one atomic per workgroup on the same word."""
    blocks, stride = sumsq_grid(n)
    n4, q, unrolled, rest = n >> 2, 0, 0, 0
    while q + 3 * stride < n4:
        q, unrolled = q + 4 * stride, unrolled + 1
    while q < n4:
        q, rest = q + stride, rest + 1
    return 1 + (6 if unrolled else 3) + unrolled + rest + 1 + 6 + 3 + blocks


# --------------------------------------------------------------------------------------------------------------- dropout
DROPOUT_PS = [0.0, 1e-10, 0.2, 0.5, float(np.nextafter(np.float32(1.0), np.float32(0.0)))]


def dropout_words(n, seed, offset):
    """The Philox word of each of the first n elements of the stream: element ``4 q + e`` draws word ``e`` of the counter
    ``offset + q`` (64 bits, wraps), key ``seed`` -> uint64 array (n,)."""
    quads = (n + 3) // 4
    index = np.full(quads, int(offset) & P.MASK64, np.uint64) + np.arange(quads, dtype=np.uint64)  # (arrays wrap silently)
    return np.stack(P.draw(index, 0, 0, seed), axis=1).reshape(-1)[:n]


def dropout_expected(x, n, p, seed, offset, relu_of=None):
    """``ss_dropout`` -> (keep, want, bound): ``keep`` (bool) is the exact pattern -- an element is kept if its word is at least
    ``int(float32(p) * 2**32)`` and, where ``relu_of`` is given, ``relu_of > 0``; every other element is +0.0.  ``want`` is the
    float64 value ``x * 1 / (1 - float32(p))`` of a kept element (0 elsewhere; p = 0: x itself), ``bound`` 2 float32 ulp of it:
    one rounded reciprocal and one rounded product.  (The kernel also rounds ``1 - p``; tests/test_flat_ref_cpu.py checks for
    every p of ``DROPOUT_PS`` that the float32 keep-scale is within ``u`` of the float64 one all the same, which leaves the
    product's rounding: 2 u |y| < 2 ulp.)"""
    p32 = float(np.float32(p))
    x = np.asarray(x, np.float32).reshape(-1)[:n].astype(np.float64)
    keep = dropout_words(n, seed, offset) >= np.uint64(int(p32 * 2 ** 32))
    if relu_of is not None:
        keep &= np.asarray(relu_of, np.float32).reshape(-1)[:n] > 0
    want = np.where(keep, x * (1.0 / (1.0 - p32)) if p32 > 0.0 else x, 0.0)
    return keep, want, 2.0 * f32_ulp(want)


# ------------------------------------------------------------------------------------------------------ softmax + top-k
def softmax_topk_expected(logits, k):
    """-> (probs (B, k) float64, idx (B, k) int32): the float64 softmax of every row, its entries in the order "logit
    descending, index ascending", the first k of them; slots past C hold (0.0, -1)."""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    B, C = lg.shape
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    sm = e / e.sum(axis=1, keepdims=True)
    probs, idx = np.zeros((B, k)), np.full((B, k), -1, np.int32)
    for b in range(B):
        order = np.lexsort((np.arange(C), -lg[b]))[:k]
        probs[b, :len(order)], idx[b, :len(order)] = sm[b, order], order
    return probs, idx


# -------------------------------------------------------------------------------------------------------- active frames
def active_frames_expected(lengths, B, T):
    """-> int32 array: how many rows (b, t) of a padded (B, T) batch belong to a clip, then their numbers ``b * T + t`` in
    ascending order; a length is clamped to [0, T]."""
    l = np.clip(np.asarray(lengths, np.int64)[:B], 0, T)
    rows = [b * T + np.arange(l[b]) for b in range(B)]
    return np.concatenate([[int(l.sum())]] + rows).astype(np.int32)
