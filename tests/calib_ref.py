"""CPU restatement, in float64 NumPy, of the calibration kernels (csrc/calib.hip): the row values of the temperature fit, the
bisection schedule of ``ss_calib_bisect``, the reliability bins and the rank rule of ``ss_calib_bins`` -- and float32 error bounds
for the sums of ``ss_calib_moments`` and for a row's confidence that are DERIVED here from the kernels' operation count and the
unit roundoff, not fitted to any GPU output.

Parametrised by the inverse temperature u = 1 / T.  Row with logits z (C floats), label y, m = max z, d_c = z_c - m <= 0:

    e_c = exp(u d_c)     S0 = sum e_c     S1 = sum e_c d_c
    nll = log S0 - u d_y                  g = d nll / du = S1 / S0 - d_y            dg / du = Var_p[z], p = softmax(u z)

sum nll is convex in u, so sum g is non-decreasing in u.  A row whose label is outside [0, C) counts nowhere.

The schedule (``fit``; include/ss_hotpath.h): iteration 0 evaluates u = 1 and records nll_at_1; iteration 1 evaluates U_MIN = 0.05
(g >= 0: the answer is U_MIN, at_bound = -1); iteration 2 evaluates U_MAX = 20 (g <= 0: the answer is U_MAX, at_bound = +1); then
32 steps u = sqrt(lo hi), g > 0 moves hi, otherwise lo.  After the last step u stays the point just evaluated, an end of the final
bracket, whose width in ln u is RESOLUTION = ln(U_MAX / U_MIN) / 2^32 = 1.4e-9 -- below the 2^-24 = 6e-8 a float32 temperature
resolves, which is why 32 steps, and so 35 evaluations, are enough and more would be wasted.

The bound.  U = 2^-24 is the unit roundoff of float32 (+, -, * and a fused multiply-add round once: relative error <= U).  Assumed,
as in distill_ref.py, since no ulp table of the device's math library is at hand: expf and logf within 1 ulp (relative error DE =
DL = 2U), the division within 2.5 ulp (DD = 5U).  First-order propagation; the neglected second-order terms are below 0.1 % while
the largest exponent error stays under 1e-3 (asserted), and the bound is multiplied by 1.001 for them.  Per row, absolute errors E,
relative errors R:

    d_c = z_c - m        one subtraction of exact inputs                     R_d = U
    a_c = u32 * d_c      u32 = float32(u) (the kernel reads the state's double and rounds it: U), R_d, one product
                                                                             E_a = 3U |a_c|
    e_c = expf(a_c)      argument error, then expf                           R_e = E_a + DE
    S0 = sum e_c         the e_c weighted by softmax, C - 1 inexact additions of positive terms in whatever order (a lane's
                         chain, the wave's tree)                             R_S0 = sum_c p_c R_e_c + (C - 1) U
    S1 = sum e_c d_c     every term carries R_e, R_d and one product (a fused multiply-add rounds less), all terms <= 0, C - 1
                         additions                                           E_S1 = sum_c |e_c d_c| (R_e_c + 2U) + (C - 1) U |S1|
    nll = logf(S0) - u32 d_y    logf of an inexact argument, the product u32 d_y (3U), one subtraction (or one fma: less)
                                                                             E_nll = R_S0 + DL |log S0| + 3U |u d_y| + U |nll|
    g = S1 / S0 - d_y    the quotient q                                      E_q = E_S1 / S0 + |q| (R_S0 + DD)
                         R_d on d_y, one subtraction                         E_g = E_q + U |d_y| + U |g|
    conf = 1 / S0                                                            E_conf = conf (R_S0 + DD)

Underflow: a float32 result below 2^-126 may come out as zero or denormal, an absolute error of up to ETA = 2^-126 per e_c that no
relative term covers; C ETA is added to S0's and C ETA |d|_max to S1's absolute error.  The sums over rows are float64 in a fixed
order: N 2^-53 of the sum of the magnitudes, added for completeness.
"""
import math

import numpy as np

U = 2.0 ** -24
DE = 2 * U   # expf: 1 ulp (assumed)
DL = 2 * U   # logf: 1 ulp (assumed)
DD = 5 * U   # division: 2.5 ulp (assumed; correctly rounded would be U)
ETA = 2.0 ** -126
SLACK = 1.001

U_MIN, U_MAX, FIT_ITERS = 0.05, 20.0, 35
RESOLUTION = math.log(U_MAX / U_MIN) / 2.0 ** 32  # width of the final bracket in ln u


def counts(y, C):
    """The label rule -> bool (N,)."""
    y = np.asarray(y, np.int64)
    return (y >= 0) & (y < C)


def _rows(z, y, u):
    z = np.asarray(z, np.float64)
    N, C = z.shape
    ok = counts(y, C)
    ya = np.where(ok, np.asarray(y, np.int64), 0)
    d = z - z.max(1, keepdims=True)
    e = np.exp(u * d)
    S0 = e.sum(1)
    S1 = (e * d).sum(1)
    dy = d[np.arange(N), ya]
    return dict(ok=ok, d=d, e=e, S0=S0, S1=S1, dy=dy, nll=np.log(S0) - u * dy, g=S1 / S0 - dy)


def row_values(z, y, u):
    """-> (nll (N,), g (N,), counts (N,)) in float64; rows that do not count hold 0."""
    R = _rows(z, y, u)
    return R["nll"] * R["ok"], R["g"] * R["ok"], R["ok"]


def moments(z, y, u):
    """-> (sum nll, sum g) over the rows that count."""
    nll, g, _ = row_values(z, y, u)
    return float(nll.sum()), float(g.sum())


def second_moment(z, y, u):
    """sum over the rows that count of Var_p[z], p = softmax(u z): the derivative of sum g with respect to u."""
    R = _rows(z, y, u)
    p = R["e"] / R["S0"][:, None]
    mean = (p * R["d"]).sum(1)
    var = (p * (R["d"] - mean[:, None]) ** 2).sum(1)
    return float((var * R["ok"]).sum())


def bounds(z, y, u):
    """The float32 error bounds of the module docstring at inverse temperature u -> dict(nll_sum, g_sum, conf (N,))."""
    R = _rows(z, y, u)
    N, C = R["d"].shape
    d, e, S0, S1, dy = R["d"], R["e"], R["S0"], R["S1"], R["dy"]
    a = u * d
    E_a = 3 * U * np.abs(a)
    assert float(E_a.max()) < 1e-3, "the first-order bound needs small exponent errors"
    R_e = E_a + DE
    p = e / S0[:, None]
    R_S0 = (p * R_e).sum(1) + (C - 1) * U + C * ETA / S0
    E_S1 = (np.abs(e * d) * (R_e + 2 * U)).sum(1) + (C - 1) * U * np.abs(S1) + C * ETA * np.abs(d).max(1)
    E_nll = R_S0 + DL * np.abs(np.log(S0)) + 3 * U * np.abs(u * dy) + U * np.abs(R["nll"])
    q = S1 / S0
    E_g = E_S1 / S0 + np.abs(q) * (R_S0 + DD) + U * np.abs(dy) + U * np.abs(R["g"])
    ok = R["ok"]
    f64 = N * 2.0 ** -53
    return dict(nll_sum=SLACK * float((E_nll * ok).sum() + f64 * np.abs(R["nll"] * ok).sum()),
                g_sum=SLACK * float((E_g * ok).sum() + f64 * np.abs(R["g"] * ok).sum()),
                conf=SLACK * (R_S0 + DD) / S0)


def softmax_bound(z, u):
    """softmax(u z) in float64 and the float32 bound of ss_softmax_topk_t's probabilities, expf(u d_c) / S0: the relative errors
    of e_c, of S0 and of the division -> (p (N, C), E_p (N, C))."""
    z = np.asarray(z, np.float64)
    R = _rows(z, np.zeros(len(z), np.int64), u)
    C = z.shape[1]
    R_e = 3 * U * np.abs(u * R["d"]) + DE
    p = R["e"] / R["S0"][:, None]
    R_S0 = (p * R_e).sum(1) + (C - 1) * U + C * ETA / R["S0"]
    return p, SLACK * (p * (R_e + R_S0[:, None] + DD) + ETA)


def fit(z, y, evaluate=None):
    """The schedule of ``ss_calib_bisect`` around ``evaluate(u) -> (sum nll, sum g)`` (default: ``moments`` of z, y)
    -> dict(u, lo, hi, nll, g, nll_at_1, iteration, at_bound)."""
    if evaluate is None:
        evaluate = lambda u: moments(z, y, u)  # noqa: E731
    st = dict(u=1.0, lo=U_MIN, hi=U_MAX, nll=0.0, g=0.0, nll_at_1=0.0, iteration=0, at_bound=0)
    for _ in range(FIT_ITERS):
        nll, g = evaluate(st["u"])
        it = st["iteration"]
        if st["at_bound"] != 0 or it >= FIT_ITERS:
            continue  # pinned: the state is left alone
        u = st["u"]
        st["nll"], st["g"] = nll, g
        if it == 0:
            st["nll_at_1"] = nll
            st["u"] = U_MIN
        elif it == 1:
            if g >= 0.0:
                st["at_bound"] = -1
            else:
                st["u"] = U_MAX
        elif it == 2:
            if g <= 0.0:
                st["at_bound"] = 1
            else:
                st["u"] = math.sqrt(st["lo"] * st["hi"])
        else:
            if g > 0.0:
                st["hi"] = u
            else:
                st["lo"] = u
            if it + 1 < FIT_ITERS:
                st["u"] = math.sqrt(st["lo"] * st["hi"])
        st["iteration"] = it + 1
    return st


def fit_tolerance(z, y, u_root):
    """How far, in u, a float32 fit may end from the float64 one: the bound on sum g at the root over the slope of sum g there
    (a root of the perturbed function lies within that of the true root, to first order), plus the width of the final bracket
    once for each of the two fits (each returns an END of its own bracket)."""
    slope = second_moment(z, y, u_root)
    return bounds(z, y, u_root)["g_sum"] / slope + 2.0 * u_root * RESOLUTION


def ranks(z, y):
    """The rank of the true class of every row: #{c: z_c > z_y, or z_c == z_y and c < y} (0 = the prediction is right, when
    no class ties below y).  Rows that do not count hold -1."""
    z = np.asarray(z, np.float64)
    N, C = z.shape
    ok = counts(y, C)
    ya = np.where(ok, np.asarray(y, np.int64), 0)
    zy = z[np.arange(N), ya][:, None]
    c = np.arange(C)[None, :]
    r = ((z > zy) | ((z == zy) & (c < ya[:, None]))).sum(1)
    return np.where(ok, r, -1)


def bins(z, y, u=1.0, n_bins=15, k_max=5):
    """``ss_calib_bins`` in float64 -> dict(bin_count, bin_hits (int64 (n_bins,)), bin_conf (float64 (n_bins,): the SUM of the
    confidences), rank_hist (int64 (k_max + 1,)), conf (N,), pred (N,))."""
    R = _rows(z, y, u)
    ok = R["ok"]
    conf = 1.0 / R["S0"]
    pred = np.argmax(np.asarray(z, np.float64), 1)  # (the lowest index among equal maxima)
    b = np.minimum(n_bins - 1, np.floor(conf * n_bins).astype(np.int64))
    hit = pred == np.asarray(y, np.int64)
    out = dict(bin_count=np.bincount(b[ok], minlength=n_bins), bin_hits=np.bincount(b[ok & hit], minlength=n_bins),
               bin_conf=np.bincount(b[ok], weights=conf[ok], minlength=n_bins).astype(np.float64),
               rank_hist=np.bincount(np.minimum(ranks(z, y)[ok], k_max), minlength=k_max + 1), conf=conf, pred=pred)
    return out


def ece_mce(bin_count, bin_hits, bin_conf):
    """Expected and maximum calibration error from the bins (``bin_conf`` the per-bin SUM of confidences)."""
    cnt = np.asarray(bin_count, np.float64)
    some = cnt > 0
    gap = np.abs(np.asarray(bin_hits, np.float64)[some] - np.asarray(bin_conf, np.float64)[some]) / cnt[some]
    if not some.any():
        return 0.0, 0.0
    return float((cnt[some] * gap).sum() / cnt.sum()), float(gap.max())


def bin_centre_rows(C, n_bins, j):
    """A logit row [a, 0, ..., 0] whose softmax confidence is the centre of bin j, p = (j + 1/2) / n_bins -- for the bins whose
    centre is above 1 / C, where such a row exists: a = ln(p (C - 1) / (1 - p)) > 0."""
    p = (j + 0.5) / n_bins
    assert p > 1.0 / C
    row = np.zeros(C, np.float32)
    row[0] = np.float32(math.log(p * (C - 1) / (1.0 - p)))
    return row
