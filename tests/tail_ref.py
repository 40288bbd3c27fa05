"""CPU restatement of the fused classifier tail (csrc/tail.hip: AttnPool -> LayerNorm -> Linear -> ReLU -> Dropout -> Linear -> CE)
with everything the two kernels stash and return, in float32 or float64 -- plus the seeded builders of the weights and inputs the
edge tests run on.

Plain torch ops only.  The arithmetic is ``oracle.model_ref.attn_pool``, ``head`` and ``ce_label_smoothing`` statement by
statement, so the float32 form at MID = 128 without dropout is bit-equal to them (tests/test_tail_ref_cpu.py pins that) and the
float64 form is the same function with 29 more bits: the difference of the two is the reference's own error, the yardstick every
tolerance of tests/test_gpu_tail_edges.py is a multiple of (``roi_cnn_ref.bound``).  The dropout is an INPUT here: a ``keep`` mask
times ``1 / (1 - float32(p))``, never a draw.  MID comes from the weights' shapes.
"""
import numpy as np
import torch
import torch.nn.functional as F

from roi_cnn_ref import bound, needed_k, ulp32  # noqa: F401  (the one tolerance rule; the GPU file takes it from here)

KEYS = ("pool.score.weight", "pool.score.bias", "head.0.weight", "head.0.bias", "head.1.weight", "head.1.bias", "head.4.weight",
        "head.4.bias")
GRADS = dict(g_wscore="pool.score.weight", g_bscore="pool.score.bias", g_gamma="head.0.weight", g_beta="head.0.bias",
             dW1="head.1.weight", dW4="head.4.weight")
FWD = ("attn", "xhat", "rstd", "ln", "mid", "mid_d", "logits", "d_logits", "loss")  # what ss_tail_fwd writes
CLIP = ("d_h", "d_mid")                                                             # ss_tail_bwd, per clip
SUMS = ("g_gamma", "g_beta", "g_wscore", "dW1", "dW4")                             # sums over the clips (g_bscore: below)
LN_EPS = 1e-5
GAP = 1e-4  # the two best logits of a row are further apart than this in float64, or exactly tied: then ``correct`` is compared


# ------------------------------------------------------------------------------------------------ weights
def make_params(D, MID, C, seed):
    """The tail's tensors for free (D, MID, C) at the scales of ``golden/weights.make_state_dict``: U(-a, a) with a = 1.5 /
    sqrt(fan_in), a bias with its weight's fan-in, LayerNorm gamma 1 + U(-0.2, 0.2)."""
    g = torch.Generator().manual_seed(seed)
    shapes = {KEYS[0]: (1, D), KEYS[1]: (1,), KEYS[2]: (D,), KEYS[3]: (D,), KEYS[4]: (MID, D), KEYS[5]: (MID,), KEYS[6]: (C, MID),
              KEYS[7]: (C,)}
    fans = {KEYS[0]: D, KEYS[1]: D, KEYS[2]: D, KEYS[3]: D, KEYS[4]: D, KEYS[5]: D, KEYS[6]: MID, KEYS[7]: MID}
    p = {}
    for k in KEYS:
        t = (torch.rand(shapes[k], generator=g) * 2 - 1) * (1.5 / np.sqrt(fans[k]))
        if k == "head.0.weight":
            t = 1.0 + (torch.rand(shapes[k], generator=g) * 2 - 1) * 0.2
        p[k] = t.float().contiguous()
    return p


# ------------------------------------------------------------------------------------------------ the tail
def drop_scale(drop_p, dtype):
    """1 / (1 - float32(p)) as ``dtype`` computes it (the kernels: float32)."""
    p32 = np.float32(drop_p)
    if dtype == torch.float32:
        return float(np.float32(1.0) / (np.float32(1.0) - p32))
    return 1.0 / (1.0 - float(p32))


def tail(h, lengths, params, y, *, dtype, keep=None, drop_p=0.0, ls=0.05, denom=None):
    """h (B,T,D) zero behind every clip's length, lengths (B,), params by ``KEYS``, y (B,) labels inside the classes;
    ``keep`` (B,MID) bool with ``drop_p``: the dropout; ``denom``: what the summed loss is divided by (None: the mean, B).
    -> dict of detached tensors in ``dtype``: attn (B,T), pooled, xhat, ln (B,D), rstd (B,), mid, mid_d (B,MID), logits, d_logits
    (B,C), loss (scalar); d_h (B,T,D), d_mid (B,MID: at the first Linear's output, before the ReLU), g_gamma, g_beta, g_wscore (D,),
    g_bscore (1,), dW1 (MID,D), dW4 (C,MID) from ONE autograd backward of the loss; ``correct``: how many rows have argmax == y."""
    p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in KEYS}
    hg = h.detach().to(dtype).clone().requires_grad_(True)
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    B, T, D = hg.shape
    # ---- oracle.model_ref.attn_pool
    mask = torch.arange(T).unsqueeze(0) < lengths.unsqueeze(1)
    scores = F.linear(hg, p[KEYS[0]], p[KEYS[1]]).squeeze(-1)
    scores = scores.masked_fill(~mask, -1e9)
    attn = torch.softmax(scores, dim=1)
    pooled = (hg * attn.unsqueeze(-1)).sum(dim=1)
    # ---- oracle.model_ref.head
    ln = F.layer_norm(pooled, (D,), p[KEYS[2]], p[KEYS[3]], eps=LN_EPS)
    pre = F.linear(ln, p[KEYS[4]], p[KEYS[5]])
    mid = F.relu(pre)
    mid_d = mid
    if keep is not None:
        mid_d = mid * (keep.to(dtype) * drop_scale(drop_p, dtype))
    logits = F.linear(mid_d, p[KEYS[6]], p[KEYS[7]])
    # ---- oracle.model_ref.ce_label_smoothing
    logp = torch.log_softmax(logits, dim=1)
    nll = -logp.gather(1, y.unsqueeze(1)).squeeze(1)
    smooth = -logp.mean(dim=1)
    rows = (1.0 - ls) * nll + ls * smooth
    loss = rows.mean() if denom is None else rows.sum() / denom
    for t in (pre, logits, pooled):
        t.retain_grad()
    loss.backward()
    with torch.no_grad():  # what the kernel stashes of the LayerNorm
        mean = pooled.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(pooled.var(1, unbiased=False, keepdim=True) + LN_EPS)
        xhat = (pooled - mean) * rstd
    out = dict(attn=attn, pooled=pooled, xhat=xhat, rstd=rstd.squeeze(1), ln=ln, mid=mid, mid_d=mid_d, logits=logits, loss=loss,
               d_logits=logits.grad, d_h=hg.grad, d_mid=pre.grad, d_pooled=pooled.grad)
    for name, key in GRADS.items():
        out[name] = p[key].grad.reshape(-1) if name.startswith("g_") else p[key].grad
    out = {k: v.detach() for k, v in out.items()}
    out["correct"] = int((out["logits"].argmax(1) == y).sum())
    return out


def logit_gaps(logits64):
    """(B,) the float64 distance between the best and the second-best logit of every row (C = 1: inf)."""
    if logits64.shape[1] == 1:
        return torch.full((logits64.shape[0],), float("inf"), dtype=torch.float64)
    top = logits64.double().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def bscore_bound(case, r64):
    """g_bscore is the sum over the frames of d score_t = attn_t (g_t - dot), g_t = h_t . d_pooled, dot = sum_t attn_t g_t: exactly
    0 whatever the inputs, since the softmax does not see a shift of its scores.  What a float32 evaluation leaves is rounding, so
    k * e_ref (a multiple of the float32 reference's own leftover, which is 0 on some inputs) is no yardstick; the bound is derived.
    With u = 2^-24 and n frames: the attention weights sum to 1 + e, |e| <= (n + 2) u (n - 1 additions, a reciprocal, a product); dot
    is off by at most n u sum_t attn_t |g_t|; each d score_t carries 2 u; their sum adds (n - 1) u sum_t |d score_t|.  Errors IN the
    g_t cancel like the g_t themselves.  With S = sum_t attn_t (|g_t| + |dot|) that is below (2 n + 8) u S per clip."""
    h, dp, attn = case["h"].double(), r64["d_pooled"].double(), r64["attn"].double()
    g = (h * dp.unsqueeze(1)).sum(-1)
    dot = (attn * g).sum(1, keepdim=True)
    S = (attn * (g.abs() + dot.abs())).sum(1)
    n = torch.as_tensor(case["lengths"]).double()
    return float(((2 * n + 8) * 2.0 ** -24 * S).sum())


def exact_names(case):
    """The tensors whose float32 and float64 references may agree exactly (e_ref = 0) because the value is STRUCTURAL; they are
    held to the floor alone, k = 0.  Everywhere else e_ref > 0 (tests/test_tail_ref_cpu.py checks both directions' claim)."""
    names = set()
    B, T, D = case["h"].shape
    C = case["params"][KEYS[7]].shape[0]
    if bool((torch.as_tensor(case["lengths"]) == 1).all()):  # softmax over one frame: attn = 1, no gradient into the scores
        names |= {"attn", "g_wscore", "g_bscore"}
    if D == 1:  # a row of one value normalises to 0
        names |= {"xhat", "ln", "d_h", "g_gamma", "g_wscore", "g_bscore"}
    if C == 1:  # log_softmax of one class is 0: no loss, no gradient
        names |= {"loss", "d_logits", "d_h", "d_mid", "g_gamma", "g_beta", "g_wscore", "g_bscore", "dW1", "dW4"}
    if case.get("flat"):
        names |= {"attn", "xhat", "ln", "g_gamma", "g_wscore", "g_bscore"}
    return names


# ------------------------------------------------------------------------------------------------ inputs
def _lengths(lengths, B, T, g):
    """None / "full": every clip T frames; "one": every clip one frame; "mixed": clip 0 full, clip 1 one frame, the rest drawn."""
    if lengths is None or isinstance(lengths, str) and lengths == "full":
        return torch.full((B,), T, dtype=torch.int64)
    if isinstance(lengths, str) and lengths == "one":
        return torch.ones(B, dtype=torch.int64)
    if isinstance(lengths, str) and lengths == "mixed":
        n = torch.randint(1, T + 1, (B,), generator=g)
        n[0] = T
        if B > 1:
            n[1] = 1
        return n.to(torch.int64)
    n = torch.as_tensor(lengths, dtype=torch.int64)
    assert n.shape == (B,) and int(n.min()) >= 1 and int(n.max()) <= T
    return n


def _zero_padding(h, lengths):
    for b in range(h.shape[0]):
        h[b, int(lengths[b]):] = 0
    return h


def random_case(B, T, D, MID, C, lengths, seed):
    """-> dict(h (B,T,D) standard normal and zero behind each length, lengths int64 (B,), y (B,), params)."""
    g = torch.Generator().manual_seed(seed * 1000003 + ((B * 31 + T) * 31 + D) * 31 + MID * 7 + C)
    h = torch.randn(B, T, D, generator=g)
    n = _lengths(lengths, B, T, g)
    y = torch.randint(0, C, (B,), generator=g)
    return dict(h=_zero_padding(h, n), lengths=n, y=y, params=make_params(D, MID, C, seed + 17))


def sharp_case(B, T, D, MID, C, seed):
    """Attention scores spread over about +-60: one frame of each clip scores +60, one +35 and the others lie evenly in [-60, -45],
    in a shuffled order, so the softmax is one-hot to float32 (the runner-up is exp(-25)) and every other exponential, exp(-105) and
    below, underflows to zero."""
    case = random_case(B, T, D, MID, C, "mixed", seed)
    g = torch.Generator().manual_seed(seed + 5)
    w = case["params"][KEYS[0]][0].double()
    bsc = float(case["params"][KEYS[1]][0])
    h = 0.05 * case["h"].double()
    for b in range(B):
        n = int(case["lengths"][b])
        want = torch.cat([torch.tensor([60.0, 35.0], dtype=torch.float64), torch.linspace(-60.0, -45.0, max(n - 2, 1), dtype=torch.float64)])[:n]
        want = want[torch.randperm(n, generator=g)]
        now = h[b, :n] @ w + bsc
        h[b, :n] += ((want - now) / float(w @ w)).unsqueeze(1) * w.unsqueeze(0)
    case["h"] = _zero_padding(h.float(), case["lengths"])
    return case


def flat_row_case(B, T, D, MID, C, seed):
    """Every clip has length 1 and its only frame is the constant 0.5 over a power-of-two D: attn is 1, the pooled row is 0.5
    everywhere, its mean is exact, xhat is exactly 0, ln is exactly beta and rstd is 1 / sqrt(eps) = 316."""
    assert D & (D - 1) == 0
    case = random_case(B, T, D, MID, C, "one", seed)
    case["h"].zero_()
    case["h"][:, 0] = 0.5
    case["flat"] = True
    return case


# ------------------------------------------------------------------------------------------------ the tables of the edge tests
# One axis at a time, the others small.  What each value is the edge of, in csrc/tail.hip:
#   T    scores go to the 16 waves with stride 16, the softmax loops stride 1024 threads
#   D    the Linear(D -> MID) prefetch holds 6 x 64 columns, the rest goes in rounds of 4 x 64; per-thread loops stride 1024
#   MID  4 rows per wave, 64 rows per pass, 2 prefetched passes (the third reads its rows from column 0); backward's o = tid loop
#   C    the logits loop strides 16 waves, the loss row 64 lanes, the backward's d_logits load 1024 threads
SMALL = dict(T=9, D=64, MID=8, C=3)
T_SWEEP = (1, 15, 16, 17, 1023, 1024, 1025, 2049)
D_SWEEP = (1, 2, 63, 64, 65, 383, 384, 385, 448, 639, 640, 641, 1023, 1024, 1025, 2050)
MID_SWEEP = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 192, 1025)
C_SWEEP = (1, 2, 15, 16, 17, 63, 64, 65, 129, 1025)
CORNERS = ((17, 641, 130, 65), (1025, 385, 129, 17))
LOSS_C = (63, 64, 65, 129)
CONTRACT = ((7, 11, 5, 192), (33, 30, 10, 192), (2, 90, 100, 192), (5, 30, 100, 512), (3, 9, 7, 250))  # test_fused_tail_fwd_bwd's
DROP_PS = (0.2, 0.5)
DROP_MIDS = (5, 128, 130)
LDS_FLOATS = 60 * 1024 // 4
SWEEP_B = 3


def sweep_specs():
    """-> {tag: (B, T, D, MID, C, lengths, seed)} of every one-axis sweep and corner."""
    s, specs = SMALL, {}
    for T in T_SWEEP:
        for n in ("full", "one", "mixed"):
            if T == 1 and n != "full":
                continue
            specs[f"T{T}-{n}"] = (SWEEP_B, T, 64, 128, 5, n, 1)
    for D in D_SWEEP:
        for MID in (128, 130):
            specs[f"D{D}-MID{MID}"] = (SWEEP_B, s["T"], D, MID, s["C"], "mixed", 2)
    for MID in MID_SWEEP:
        for D in (64, 448):
            specs[f"MID{MID}-D{D}"] = (SWEEP_B, s["T"], D, MID, s["C"], "mixed", 23)
    for C in C_SWEEP:
        specs[f"C{C}"] = (SWEEP_B, s["T"], s["D"], s["MID"], C, "mixed", 4)
    for T, D, MID, C in CORNERS:
        specs[f"corner-T{T}-D{D}-MID{MID}-C{C}"] = (SWEEP_B, T, D, MID, C, "mixed", 5)
    return specs


def contract_specs():
    return {f"B{B}-T{T}-C{C}-Hd{Hd}": (B, T, 2 * Hd, 128, C, "mixed", 6) for B, T, C, Hd in CONTRACT}


def drop_specs():
    return {f"MID{MID}": (3, SMALL["T"], SMALL["D"], MID, SMALL["C"], "mixed", 7) for MID in DROP_MIDS}


def loss_specs():
    return {f"C{C}": (3, SMALL["T"], SMALL["D"], SMALL["MID"], C, "mixed", 8) for C in LOSS_C}


def special_cases():
    """-> {tag: case}: the numerical edges."""
    s = SMALL
    return {"sharp": sharp_case(3, 17, s["D"], 128, 5, 9), "flat": flat_row_case(2, 3, s["D"], s["MID"], s["C"], 10),
            "all-length-1": random_case(3, s["T"], s["D"], s["MID"], s["C"], "one", 11)}


def lds_specs():
    """The two 60 KiB conditions met from the inside at D = 64, MID = 8, B = 1: the forward's T + 2 D + MID + C and the backward's
    MID + D + 2 T + C are ``LDS_FLOATS`` exactly; one more frame is outside.  (With C = 3 the backward's sum is odd for every T: its
    exact case takes C = 4, and C = 3 is run one float below the limit.)"""
    s = SMALL
    t_fwd = LDS_FLOATS - 2 * s["D"] - s["MID"] - s["C"]
    t_bwd4 = (LDS_FLOATS - s["MID"] - s["D"] - 4) // 2
    t_bwd3 = (LDS_FLOATS - s["MID"] - s["D"] - 3) // 2
    assert t_fwd + 2 * s["D"] + s["MID"] + s["C"] == LDS_FLOATS and s["MID"] + s["D"] + 2 * t_bwd4 + 4 == LDS_FLOATS
    assert s["MID"] + s["D"] + 2 * t_bwd3 + 3 == LDS_FLOATS - 1
    return {"fwd": (1, t_fwd, s["D"], s["MID"], s["C"], "full", 12), "bwd-C4": (1, t_bwd4, s["D"], s["MID"], 4, "full", 13),
            "bwd-C3": (1, t_bwd3, s["D"], s["MID"], s["C"], "full", 14)}


_REFS = {}


def refs(tag, case, keep=None, drop_p=0.0):
    """(float32 reference, float64 reference) of a case, computed once per ``tag`` and shared; never written to."""
    if tag not in _REFS:
        kw = dict(keep=keep, drop_p=drop_p, denom=float(case["h"].shape[0]))
        _REFS[tag] = tuple(tail(case["h"], case["lengths"], case["params"], case["y"], dtype=dt, **kw)
                           for dt in (torch.float32, torch.float64))
    return _REFS[tag]
