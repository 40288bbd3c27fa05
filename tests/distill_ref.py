"""CPU restatement, in float64 NumPy, of the loss row with a teacher's soft targets (csrc/ce_row.h, KD = true) and a float32 error
bound for it that is DERIVED here from the kernels' operation count and the unit roundoff -- not fitted to any GPU output.

Row with student logits z, teacher logits t, temperature tau > 0, blend alpha in [0, 1]; q = softmax(z / tau), p = softmax(t / tau):

    loss      = (1 - alpha) * hard / hard_norm        + alpha * tau^2 * sum_c p_c (log p_c - log q_c) / denom
    d logit_c = (1 - alpha) * hard_grad_c / hard_norm + alpha * tau * (q_c - p_c) / denom

``hard`` is CrossEntropyLoss(weight=w, label_smoothing=eps) of the row, un-normalised, for label y -- or, with a second label y_b
and a factor lam, ``lam * hard(y) + (1 - lam) * hard(y_b)``.  The two normalisers: ``hard_norm`` is ``den`` (the sum of w[y] over
the normalising set, handed in as the number the device divides by) with weights and ``denom`` without; the soft term is always
divided by ``denom``.  The counting rule: without weights and second labels every row counts (the caller vouches for its labels);
with weights a row counts iff 0 <= y < C; with second labels iff both labels are inside.  A row that does not count has a zero
gradient row and adds nothing, soft term included.

The bound.  u = 2^-24 is the unit roundoff of float32 (+, -, * and a fused multiply-add round once: relative error <= u).  Assumed,
since no ulp table of the device's math library is at hand: expf and logf within 1 ulp (relative error DE = DL = 2u) and the
division within 2.5 ulp (DD = 5u; a correctly rounded one would be u).  First-order error propagation; the neglected second-order
terms are below 0.1 % of the bound as long as the largest exponent error stays under 1e-3, which ``evaluate`` asserts, and the
bound is multiplied by 1.001 for them.  Per row (m the row maximum, a_c = (x_c - m) / tau; absolute errors E, relative errors R):

    a_c          one subtraction, one division                         E_a = (u + DD) |a_c|
    e_c = exp a  argument error E_a -- this is where a wide row at a low temperature pays: |a_c| reaches span / tau --
                 plus expf                                             R_e = E_a + DE
    se = sum e   the e_c weighted by softmax, C - 1 inexact additions of positive terms, whatever the order (one thread's
                 chain or a wave's tree: an added zero is exact)       R_se = sum_c soft_c R_e + (C - 1) u
    ls = log se                                                        E_ls = R_se + DL |ls|
    lq_c = a - ls                                                      E_lq = E_a + E_ls + u |lq_c|
    q_c = exp lq                                                       E_q = q_c (E_lq + DE)
    q_c - p_c    both absolute errors and the subtraction's rounding: the cancellation costs nothing beyond them
    * tau / denom                                                      E_g = tau / denom (E_q + E_p) + (2u + DD) |g_c|
    KL term      p_c (lp_c - lq_c), C - 1 additions                    E_kl = sum_c [p_c (E_lp + E_lq + u |lp - lq|) + E_p |lp - lq|
                                                                              + u |term_c|] + (C - 1) u sum_c |term_c|
    soft loss    tau * tau * KL / denom                                E_soft = tau^2 / denom E_kl + (2u + DD) |soft|

The hard term goes the same way without the division (lse = m + log se adds one rounding, lp_c = z_c - lse), then: the target
tgt_c = (c == y) (1 - eps) w_y + (eps / C) w_c and the factor A = w_y + eps (sum_k w_k / C - w_y), blended over the two labels, carry
7u + DD and (C + 5) u + DD relative to the sum of the magnitudes of their terms (every operation counted once, generously); the
row's loss (1 - eps) w_y (lse - z_y) + eps (-sum_c w_c (z_c - lse) / C) is bounded term by term below.  The blend (1 - alpha) x +
alpha k adds 3u of (|(1 - alpha) x| + |alpha k|): 1 - alpha, two products, one sum.  The launch's loss is a sum of B row terms in an
order that is not fixed (a wave's tree and float atomics): (B - 1) u times the sum of their magnitudes.  Underflow: a float32
result below the smallest normal number, 2^-126, may come out as zero or denormal, an ABSOLUTE error of up to ETA = 2^-126 that no
relative term covers (a teacher probability exp(-400) is 1e-174 here and 0 there); it is added wherever a probability or a product
with one is formed.
"""
import numpy as np

U = 2.0 ** -24
DE = 2 * U   # expf: 1 ulp (assumed)
DL = 2 * U   # logf: 1 ulp (assumed)
DD = 5 * U   # division: 2.5 ulp (assumed; correctly rounded would be U)
ETA = 2.0 ** -126  # underflow: the absolute error of a result below the smallest normal float32
SLACK = 1.001


def counts(y, C, y_b=None, weighted=False):
    """The counting rule -> bool (B,)."""
    y = np.asarray(y, np.int64)
    ok = np.ones(len(y), bool)
    if y_b is not None:
        yb = np.asarray(y_b, np.int64)
        ok = (y >= 0) & (y < C) & (yb >= 0) & (yb < C)
    elif weighted:
        ok = (y >= 0) & (y < C)
    return ok


def _lsm(x, tau, soft):
    """log softmax of every row with the first-order float32 error of each step (module docstring) -> dict(lp, p, E_lp, E_p).
    ``soft``: softmax(x / tau) as the soft term computes it, lp = (x - m) / tau - log se; otherwise the hard term's arithmetic
    (tau is 1 and nothing is divided): lse = m + log se with one more rounding, lp = x - lse."""
    C = x.shape[1]
    m = x.max(1, keepdims=True)
    a = (x - m) / tau if soft else x - m
    E_a = (U + (DD if soft else 0.0)) * np.abs(a)
    e = np.exp(a)
    se = e.sum(1, keepdims=True)
    R_se = (e / se * (E_a + DE)).sum(1, keepdims=True) + (C - 1) * U
    ls = np.log(se)
    E_ls = R_se + DL * np.abs(ls)
    lp = a - ls
    if soft:
        E_lp = E_a + E_ls + U * np.abs(lp)
    else:
        E_lp = E_ls + U * np.abs(m + ls) + U * np.abs(lp)
    p = np.exp(lp)
    assert float(np.max(E_lp)) < 1e-3, "the first-order bound needs small exponent errors"
    return dict(lp=lp, p=p, E_lp=E_lp, E_p=p * (E_lp + DE) + ETA)


def _hard_label(S, z, lab, w, eps):
    """One label's hard loss and its pieces for every row, un-normalised: -> (loss, E_loss, tgt, A, A_mag); every term of tgt is
    non-negative, so it is its own magnitude."""
    B, C = z.shape
    rows = np.arange(B)
    lp, E_lp = S["lp"], S["E_lp"]
    wl = w[lab]
    slp = (w[None, :] * lp).sum(1)
    # (1 - eps) w_l (lse - z_l): lse - z_l = -lp_l with its error, then two products and the rounding of 1 - eps
    first = (1.0 - eps) * wl * -lp[rows, lab]
    E_first = (1.0 - eps) * wl * E_lp[rows, lab] + 3 * U * np.abs(first)
    # eps (-slp / C): every term w_c (z_c - lse) with its error and one product, C - 1 additions, a division, a product
    mag = (w[None, :] * np.abs(lp)).sum(1)
    E_slp = (w[None, :] * E_lp).sum(1) + U * mag + (C - 1) * U * mag
    second = eps * -slp / C
    E_second = eps / C * E_slp + (DD + U) * np.abs(second)
    loss = first + second
    E_loss = E_first + E_second + U * np.abs(loss)
    onehot = np.zeros((B, C))
    onehot[rows, lab] = 1.0
    tgt = onehot * ((1.0 - eps) * wl)[:, None] + (eps / C) * w[None, :]
    sw = w.sum()
    A = wl + eps * (sw / C - wl)
    A_mag = np.abs(wl) + eps * (sw / C + np.abs(wl))
    return loss, E_loss, tgt, A, A_mag


def evaluate(z, t, y, tau, alpha, eps, denom, w=None, den=None, y_b=None, lam=1.0):
    """The launch in float64 and its float32 bound.  z, t (B, C); y (and y_b) labels; ``w`` class weights with ``den`` the number
    the weighted hard term is divided by; ``denom`` divides the unweighted hard term and always the soft term.
    -> dict(loss, grad (B, C), loss_bound, grad_bound (B, C), correct)."""
    z, t = np.asarray(z, np.float64), np.asarray(t, np.float64)
    B, C = z.shape
    weighted = w is not None
    ok = counts(y, C, y_b, weighted)
    ww = np.ones(C) if w is None else np.asarray(w, np.float64)
    norm = float(den) if weighted else float(denom)
    ya = np.where(ok, np.asarray(y, np.int64), 0)
    H = _lsm(z, 1.0, soft=False)
    l1, E_l1, tgt, A, A_mag = _hard_label(H, z, ya, ww, eps)
    hard, E_hard = l1, E_l1
    if y_b is not None:
        yb = np.where(ok, np.asarray(y_b, np.int64), 0)
        l2, E_l2, tgt2, A2, Am2 = _hard_label(H, z, yb, ww, eps)
        oml = 1.0 - lam
        hard = lam * l1 + oml * l2
        E_hard = lam * E_l1 + oml * E_l2 + 3 * U * (lam * np.abs(l1) + oml * np.abs(l2))
        tgt, A, A_mag = lam * tgt + oml * tgt2, lam * A + oml * A2, lam * A_mag + oml * Am2
    A, A_mag = A[:, None], A_mag[:, None]
    E_A = ((C + 5) * U + DD) * A_mag if weighted else 0.0 * A_mag  # (unweighted: A is the constant 1)
    E_tgt = (7 * U + DD) * tgt
    num = H["p"] * A - tgt
    hg = num / norm
    E_hg = (H["E_p"] * np.abs(A) + H["p"] * E_A + E_tgt + U * np.abs(num)) / norm + DD * np.abs(hg)
    hl = hard / norm
    E_hl = E_hard / norm + DD * np.abs(hl)
    # ---- the soft term
    Q, P = _lsm(z, float(tau), soft=True), _lsm(t, float(tau), soft=True)
    diff = Q["p"] - P["p"]
    sg = tau * diff / denom
    E_sg = tau / denom * (Q["E_p"] + P["E_p"]) + (2 * U + DD) * np.abs(sg) + ETA
    dl = P["lp"] - Q["lp"]
    term = P["p"] * dl
    kl = term.sum(1)
    E_kl = (P["p"] * (P["E_lp"] + Q["E_lp"] + U * np.abs(dl)) + P["E_p"] * np.abs(dl) + U * np.abs(term)).sum(1) \
        + (C - 1) * U * np.abs(term).sum(1) + C * ETA
    soft = tau * tau * kl / denom
    E_soft = tau * tau / denom * E_kl + (2 * U + DD) * np.abs(soft)
    # ---- the blend, the counting rule, the launch's sum
    oma = 1.0 - alpha
    grad = oma * hg + alpha * sg
    E_grad = oma * E_hg + alpha * E_sg + 3 * U * (np.abs(oma * hg) + np.abs(alpha * sg)) + 2 * ETA
    row = oma * hl + alpha * soft
    E_row = oma * E_hl + alpha * E_soft + 3 * U * (np.abs(oma * hl) + np.abs(alpha * soft))
    grad, E_grad = grad * ok[:, None], E_grad * ok[:, None]
    row, E_row = row * ok, E_row * ok
    loss = row.sum()
    E_loss = E_row.sum() + (B - 1) * U * np.abs(row).sum()
    correct = int(((np.argmax(z, 1) == np.asarray(y, np.int64)) & ok).sum())
    return dict(loss=float(loss), grad=grad, loss_bound=SLACK * float(E_loss), grad_bound=SLACK * E_grad, correct=correct)
