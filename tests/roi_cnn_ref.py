"""CPU restatement of ROI normalise + TinyROICNN with what the fused kernels (csrc/roi_cnn.hip, csrc/roi_cnn_bwd.hip) stash and
return, frame by frame, in float32 or float64 -- plus the one seeded builder of the edge-case frame sets the tests run on.

Plain torch ops only: ``conv2d``, ``max_pool2d(..., return_indices=True)``, ``mean``, ``linear`` and one autograd backward per
frame.  The normalisation is ``oracle.model_ref.roi_normalise`` word for word, so the float32 form is bit-equal to
``oracle.model_ref.roi_cnn(roi_normalise(...))`` (tests/test_roi_cnn_ref_cpu.py pins that) and the float64 form is the same
function evaluated with 29 more bits: the difference of the two is the reference's own error, the yardstick every tolerance in
tests/test_gpu_roi_cnn_edges.py is a multiple of.
"""
import numpy as np
import torch
import torch.nn.functional as F

CNN_KEYS = ("roi_cnn.net.0.weight", "roi_cnn.net.0.bias", "roi_cnn.net.3.weight", "roi_cnn.net.3.bias",
            "roi_cnn.net.6.weight", "roi_cnn.net.6.bias", "roi_cnn.fc.weight", "roi_cnn.fc.bias")
GEOMS = ((64, 64), (48, 96), (32, 32))
GAP = 1e-4  # a float64 gap in (0, GAP] between the two best values of a window: the only windows an argmax comparison leaves out


# ------------------------------------------------------------------------------------------------ the network
def normalise(R, standardize, dtype=torch.float32, constant_is_zero=False):
    """uint8 (N,H,W) -> (N,1,H,W): oracle.model_ref.roi_normalise on a (1,N,H,W) batch, in ``dtype``.

    ``constant_is_zero``: a frame whose pixels are all equal normalises (standardize = 1) to exactly 0, which is the
    mathematical value; the float mean of H W equal values can be an ulp off and the 1e-6 clamp multiplies that ulp by 1e6."""
    r = (R.unsqueeze(0).to(dtype) / 255.0).unsqueeze(2)
    if standardize:
        mu = r.mean(dim=(2, 3, 4), keepdim=True)
        std = r.std(dim=(2, 3, 4), keepdim=True).clamp_min(1e-6)
        r = (r - mu) / std
    x = r[0]
    if standardize and constant_is_zero:
        flat = R.reshape(R.shape[0], -1)
        x = x.clone()
        x[flat.min(1).values == flat.max(1).values] = 0
    return x


def _layers(x, p):
    y1 = F.conv2d(x, p[CNN_KEYS[0]], p[CNN_KEYS[1]], padding=1)
    a1, i1 = F.max_pool2d(F.relu(y1), 2, return_indices=True)
    y2 = F.conv2d(a1, p[CNN_KEYS[2]], p[CNN_KEYS[3]], padding=1)
    a2, i2 = F.max_pool2d(F.relu(y2), 2, return_indices=True)
    y3 = F.conv2d(a2, p[CNN_KEYS[4]], p[CNN_KEYS[5]], padding=1)
    feat = F.relu(y3).mean((2, 3))
    out = F.linear(feat, p[CNN_KEYS[6]], p[CNN_KEYS[7]])
    return dict(y1=y1, a1=a1, i1=i1, y2=y2, a2=a2, i2=i2, y3=y3, feat=feat, out=out)


def _window_pos(idx, w_in):
    """max_pool2d's flat index into the (2h, 2w) plane -> position 0..3 inside its 2x2 window, row-major."""
    return (((idx // w_in) % 2) * 2 + (idx % w_in) % 2).to(torch.uint8)


def cast_params(params, dtype):
    return {k: params[k].detach().to(dtype) for k in CNN_KEYS}


def cnn_fwd_bwd(R_u8, params, d_out, standardize, dtype=torch.float32, constant_is_zero=False, grads=True):
    """-> dict: ``out`` (N,E); ``grads`` {key: (N, *shape)}: the gradient of sum(out[n] * d_out[n]) w.r.t. every parameter, PER
    FRAME; ``i1`` (N,8,H/2,W/2) / ``i2`` (N,16,H/4,W/4) uint8: the pool winners as window positions 0..3; ``y1`` / ``y2`` /
    ``y3``: the raw (pre-ReLU) convolution outputs the ties are judged on; ``a1`` / ``a2`` / ``feat``; ``m3`` = y3 > 0."""
    p = cast_params(params, dtype)
    x = normalise(R_u8, standardize, dtype, constant_is_zero)
    with torch.no_grad():
        r = _layers(x, p)
    r["i1"] = _window_pos(r["i1"], x.shape[3])
    r["i2"] = _window_pos(r["i2"], x.shape[3] // 2)
    r["m3"] = r["y3"] > 0
    r["x"] = x
    if grads:
        N = x.shape[0]
        d = d_out.to(dtype)
        G = {k: torch.empty((N,) + tuple(p[k].shape), dtype=dtype) for k in CNN_KEYS}
        for n in range(N):
            leaves = [p[k].clone().requires_grad_(True) for k in CNN_KEYS]
            o = _layers(x[n:n + 1], dict(zip(CNN_KEYS, leaves)))["out"]
            gs = torch.autograd.grad((o * d[n:n + 1]).sum(), leaves)
            for k, g in zip(CNN_KEYS, gs):
                G[k][n] = g
        r["grads"] = G
    return r


def cnn_sum_grads(R_u8, params, d_out, standardize, dtype=torch.float32, constant_is_zero=False):
    """-> (out (N,E), {key: gradient of sum_n sum(out[n] * d_out[n])}): one batched autograd backward, what ss_roi_cnn_bwd
    accumulates over all N frames."""
    p = cast_params(params, dtype)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = _layers(normalise(R_u8, standardize, dtype, constant_is_zero), leaves)["out"]
    gs = torch.autograd.grad((out * d_out.to(dtype)).sum(), [leaves[k] for k in CNN_KEYS])
    return out.detach(), dict(zip(CNN_KEYS, gs))


# ------------------------------------------------------------------------------------------------ pool windows and ties
def windows(y):
    """(N,C,2h,2w) -> (N,C,h,w,4): the four values of every 2x2 pool window, row-major."""
    n, c, hh, ww = y.shape
    return y.reshape(n, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, hh // 2, ww // 2, 4)


def window_classes(y):
    """Classify the pool windows of a raw conv output (judge them in float64).  -> dict of (N,C,h,w) tensors:
    ``positive``: the maximum is > 0 (only those windows pass a gradient); ``tied``: at least two of the four values equal the
    maximum exactly; ``close``: the two best differ by something in (0, GAP]; ``first``: the first maximal position in row-major
    order (torch's max_pool2d, the contract in include/ss_hotpath.h)."""
    w = windows(y)
    top2 = w.topk(2, dim=-1).values
    top, gap = top2[..., 0], top2[..., 0] - top2[..., 1]
    eq = w == top.unsqueeze(-1)
    first = (eq.int().cumsum(-1) == 0).sum(-1).to(torch.uint8)  # how many positions precede the first maximum
    return dict(positive=top > 0, tied=eq.sum(-1) > 1, close=(gap > 0) & (gap <= GAP), first=first, gap=gap)


def comparable(y64):
    """Windows on which a pool argmax is compared exactly: positive maximum, and exactly tied or separated by more than GAP."""
    c = window_classes(y64)
    return c["positive"] & ~c["close"], c


# ------------------------------------------------------------------------------------------------ tolerances
def ulp32(x):
    """One float32 ulp at magnitude x (x = 0: the smallest normal's ulp does not matter here, 0 is returned)."""
    x = float(x)
    return float(np.spacing(np.float32(x))) if x > 0 else 0.0


def bound(ref32, ref64, k):
    """The tolerance rule of the edge tests, for one tensor of one frame (or one summed tensor): k * e_ref + floor, where e_ref =
    max |float32 reference - float64 reference| on the same inputs and floor = 4 float32 ulps of the tensor's largest magnitude
    (it only matters where e_ref is 0).  -> (bound, e_ref, floor)."""
    e_ref = float((ref32.double() - ref64.double()).abs().max())
    floor = 4.0 * ulp32(ref64.abs().max())
    return k * e_ref + floor, e_ref, floor


def needed_k(err, e_ref, floor):
    """The k that (err <= k * e_ref + floor) would have needed: what docs/LAB_NOTES.md tabulates."""
    if err <= floor:
        return 0.0
    return (err - floor) / e_ref if e_ref > 0 else float("inf")


# ------------------------------------------------------------------------------------------------ inputs
def frame_kinds(R):
    """-> (constant, amplified), two bool vectors over the frames of R (N,H,W) uint8.  ``constant``: all pixels equal (the std clamp;
    normalises to exactly 0).  ``amplified``: not constant but with a std of u / 255 below 1e-3 (17s with one 18: 6e-5), where
    standardize = 1 multiplies the float32 rounding of u / 255 - mean by 1 / std, more than a thousandfold."""
    flat = R.reshape(R.shape[0], -1).double() / 255.0
    sd = flat.std(1)
    constant = flat.min(1).values == flat.max(1).values
    return constant, ~constant & (sd < 1e-3)


SPECIAL = ("zero", "all255", "const", "px_corner", "px_edge", "px_interior", "sat8", "grey8", "grey4", "sat8_shift", "grey8_shift",
           "grey4_shift", "ramp_h", "ramp_v", "checker1", "checker2", "last_row", "last_col")
CONSTANT = ("zero", "all255", "const")
BLOCK = ("sat8", "grey8", "grey4", "sat8_shift", "grey8_shift", "grey4_shift")


def _blocks(g, H, W, size, shift, saturate):
    """Random grey levels in size x size blocks; ``shift`` moves the block grid by one pixel so that block edges cut through the
    2x2 pool windows instead of lying between them; ``saturate`` thresholds to 0 / 255."""
    hb, wb = H // size + 2, W // size + 2
    lv = torch.randint(0, 256, (hb, wb), generator=g, dtype=torch.int32)
    if saturate:
        lv = (lv >= 128).to(torch.int32) * 255
    img = lv.repeat_interleave(size, 0).repeat_interleave(size, 1)
    o = size - 1 if shift else 0
    return img[o:o + H, o:o + W].to(torch.uint8)


def texture(N, H, W, g):
    """Random grey levels averaged with a horizontal ramp: the texture of tests/test_gpu_kernels.py's frames (no two pixels of
    a window equal in practice, no ties)."""
    R = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.int32)
    ramp = (torch.arange(W).view(1, 1, W) * 255 // (W - 1)).to(torch.int32)
    return ((R + ramp) // 2).to(torch.uint8)


def frame_set(H, W, seed, n_texture=4):
    """-> (R (18 + n_texture, H, W) uint8, names).  The 18 special frames, in the order of ``SPECIAL``:

    zero / all255 / const    constant frames: the std clamp; normalise to exactly 0 with standardize = 1
    px_corner / _edge / _interior   constant 17 with one pixel of 18 (a std of about 6e-5) at (0, 0), (0, W/2), (3, 5)
    sat8 / grey8 / grey4     0 / 255 and random grey levels in 8x8 blocks, random grey levels in 4x4 blocks: flat regions, where
                             the values of a pool window are bit-equal and "the first on ties" decides where the gradient goes
    *_shift                  the same with the block grid moved by one pixel
    ramp_h / ramp_v          horizontal and vertical ramps 0..255
    checker1 / checker2      checkerboards of period 1 and 2 pixels (0 / 255)
    last_row / last_col      constant 90 except random grey levels in the last row / the last column (the zero-halo sides)
    then ``n_texture`` frames of ``texture``."""
    g = torch.Generator().manual_seed(seed * 7919 + H * 131 + W)
    f = {}
    f["zero"] = torch.zeros(H, W, dtype=torch.uint8)
    f["all255"] = torch.full((H, W), 255, dtype=torch.uint8)
    f["const"] = torch.full((H, W), int(torch.randint(1, 255, (1,), generator=g)), dtype=torch.uint8)
    for name, (yy, xx) in (("px_corner", (0, 0)), ("px_edge", (0, W // 2)), ("px_interior", (3, 5))):
        f[name] = torch.full((H, W), 17, dtype=torch.uint8)
        f[name][yy, xx] = 18
    f["sat8"] = _blocks(g, H, W, 8, False, True)
    f["grey8"] = _blocks(g, H, W, 8, False, False)
    f["grey4"] = _blocks(g, H, W, 4, False, False)
    f["sat8_shift"] = _blocks(g, H, W, 8, True, True)
    f["grey8_shift"] = _blocks(g, H, W, 8, True, False)
    f["grey4_shift"] = _blocks(g, H, W, 4, True, False)
    f["ramp_h"] = (torch.arange(W) * 255 // (W - 1)).view(1, W).expand(H, W).to(torch.uint8)
    f["ramp_v"] = (torch.arange(H) * 255 // (H - 1)).view(H, 1).expand(H, W).to(torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    f["checker1"] = (((yy + xx) % 2) * 255).to(torch.uint8)
    f["checker2"] = ((((yy // 2) + (xx // 2)) % 2) * 255).to(torch.uint8)
    f["last_row"] = torch.full((H, W), 90, dtype=torch.uint8)
    f["last_row"][H - 1] = torch.randint(0, 256, (W,), generator=g, dtype=torch.int32).to(torch.uint8)
    f["last_col"] = torch.full((H, W), 90, dtype=torch.uint8)
    f["last_col"][:, W - 1] = torch.randint(0, 256, (H,), generator=g, dtype=torch.int32).to(torch.uint8)
    names = list(SPECIAL) + [f"texture{k}" for k in range(n_texture)]
    frames = [f[k].contiguous() for k in SPECIAL]
    R = torch.stack(frames)
    if n_texture:
        R = torch.cat([R, texture(n_texture, H, W, g)])
    return R.contiguous(), names


def frames_n(H, W, N, seed):
    """Exactly N frames: the special set followed by texture when N allows it, else the first N of a shuffled special set."""
    if N >= len(SPECIAL):
        return frame_set(H, W, seed, N - len(SPECIAL))[0]
    R, _ = frame_set(H, W, seed, 0)
    perm = torch.randperm(len(SPECIAL), generator=torch.Generator().manual_seed(seed))
    return R[perm[:N]].contiguous()


def tiled_set(H, W, N, seed):
    """N frames for the device-against-device comparison: the special set repeated with fresh block / texture seeds."""
    parts, n, k = [], 0, 0
    while n < N:
        R, _ = frame_set(H, W, seed + 1000 * k, 14)
        parts.append(R)
        n += R.shape[0]
        k += 1
    return torch.cat(parts)[:N].contiguous()
