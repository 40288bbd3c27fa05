"""Float64 reference of the bf16 ROI CNN of config 5 (csrc/cnn_bf16.h, cnn_bf16.hip, cnn_bf16_bwd.hip), entry point by entry
point, with a bf16 rounding exactly where the kernels round: the weights, the normalised image, every pooled map, the dense
gradient of the last layer (bf16(d feat / 144)) and every data gradient.  Everything here is NumPy / torch on the CPU.

Two ways to hold a kernel to it:

* the EXACT lane: inputs on a lattice (small integers times one power of two per tensor).  A bf16 x bf16 product is exact in
  f32, and while sum |terms| of an output stays below 2^24 units every partial sum is an integer number of units below 2^24,
  i.e. exact in f32 in ANY order -- MFMA accumulation, wave reductions and float atomics included.  The kernel's output then
  has to equal this reference rounded once, bit for bit, at every element.
* the DERIVED-BOUND lane (standardize = 1 cannot be put on a lattice): ``gamma_bound(n, sum_abs)`` = (n - 1) 2^-24 sum |terms|
  bounds the distance of an f32 sum of n exact products, in any order, from the exact sum.

THE WINNER RULE (read from conv1_fwd_kernel / conv_fwd_kernel / conv12_fwd_kernel and conv1_rows / conv1_winners of cnn_bf16.h):
the four raw convolution sums of a 2 x 2 window are scanned in the order 0 = (0,0), 1 = (0,1), 2 = (1,0), 3 = (1,1) with a
STRICT ``>``, so the FIRST of several equal maxima wins; the pooled value is max(best + bias, 0); the byte is the winner's
position where that value is > 0 and 4 (IDX_DEAD) where it is not -- a dead window names no tap, whatever was tied in it.
``pool`` below is the one statement of that rule; every reference routine goes through it."""
import numpy as np
import torch

C5 = [1, 16, 32, 64, 96]
IDX_DEAD = 4
NPIX_LAST = 144
LIMIT = float(2 ** 24)


# ------------------------------------------------------------------------------------------------ number formats
def bf16_rne(x64):
    """float64 tensor -> int16 tensor of bf16 bit patterns, ONE rounding to nearest, ties to even (no detour through f32)."""
    x = np.asarray(x64.detach().cpu().numpy() if isinstance(x64, torch.Tensor) else x64, dtype=np.float64)
    _, e = np.frexp(x)                                   # x = m 2^e, 0.5 <= |m| < 1: the bf16 ulp at x is 2^(e - 8)
    ulp = np.ldexp(1.0, np.maximum(e - 8, -133))         # (below 2^-126: the subnormal spacing 2^-133)
    r = np.rint(x / ulp) * ulp                           # x / ulp is exact (a power of two); rint rounds half to even
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r), "value outside the bf16 range"
    bits = (r32.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    return torch.from_numpy(bits.reshape(x.shape).copy())


def bf16_bits_to_f64(bits):
    """int16 bf16 bit patterns -> float64 values."""
    return bits.cpu().view(torch.bfloat16).double()


def bf16_val(x64):
    """float64 -> the float64 value of its bf16 rounding."""
    return bf16_bits_to_f64(bf16_rne(x64)).reshape(x64.shape)


def f32_val(x64):
    return x64.float().double()


def gamma_bound(n, sum_abs):
    """Order-independent bound of |f32 sum of n exact products - exact sum|: n - 1 roundings, each at most half an ulp of a partial
    sum that is at most sum |terms| in magnitude."""
    return (n - 1) * 2.0 ** -24 * sum_abs


# ------------------------------------------------------------------------------------------------ NHWC packers (test_gpu_bf16.py)
def nhwc_bits(x_nchw):
    """(N,C,H,W) float64 / float32 holding bf16-exact values -> int16 (N,H,W,C) bit patterns (CPU)."""
    bits = bf16_rne(x_nchw.double())
    assert torch.equal(bf16_bits_to_f64(bits), x_nchw.double()), "not bf16-exact"
    return bits.permute(0, 2, 3, 1).contiguous()


def from_nhwc_bits(t):
    """(N,H,W,C) int16 bit patterns -> (N,C,H,W) int16 on the CPU."""
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def nhwc_bytes(idx_nchw):
    return idx_nchw.permute(0, 2, 3, 1).contiguous()


def from_nhwc_bytes(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ normalisation
def normalise_like_kernel(R, standardize=True):
    """The forward kernel's per-frame normalisation, operation by operation (exact integer sums, f64 mean / variance,
    f32 table of the 256 grey levels, train_model_official.py:286-291): -> (xn f32 (N,96,96), mu (N,), sd (N,))."""
    Rn = R.numpy().astype(np.int64)
    N = Rn.shape[0]
    xn = np.empty(Rn.shape, np.float32)
    mus, sds = np.zeros(N, np.float32), np.ones(N, np.float32)
    lev = np.arange(256, dtype=np.float32) / np.float32(255.0)
    for n in range(N):
        tab = lev
        if standardize:
            tsu, tsq, nn = float(Rn[n].sum()), float((Rn[n] ** 2).sum()), float(Rn[n].size)
            mu = np.float32(np.float32(tsu / nn) / np.float32(255.0))
            var = (tsq - tsu * tsu / nn) / (nn - 1.0)
            sd = max(np.float32(np.sqrt(max(var, 0.0)) / 255.0), np.float32(1e-6))
            tab = ((lev - mu) / sd).astype(np.float32)
            mus[n], sds[n] = mu, sd
        xn[n] = tab[Rn[n]]
    return torch.from_numpy(xn), torch.from_numpy(mus), torch.from_numpy(sds)


def image_bf16(R, standardize):
    """-> (normalised image rounded to bf16, float64 (N,1,96,96); mu; sd)."""
    xn, mu, sd = normalise_like_kernel(R, bool(standardize))
    return bf16_val(xn.double()).unsqueeze(1), mu, sd


# ------------------------------------------------------------------------------------------------ the restated operations
def _pad(a):
    n, c, h, w = a.shape
    p = a.new_zeros(n, c, h + 2, w + 2)
    p[:, :, 1:-1, 1:-1] = a
    return p


def conv_raw(a, w):
    """3 x 3 convolution, zero padding 1, no bias: (N,CIN,H,W), (COUT,CIN,3,3) -> (N,COUT,H,W); all float64."""
    n, c, h, wd = a.shape
    p = _pad(a)
    out = a.new_zeros(n, w.shape[0], h, wd)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("nchw,oc->nohw", p[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
    return out


def windows(c):
    """(N,C,H,W) -> (N,C,H/2,W/2,4), position e = 2 dy + dx last."""
    return torch.stack([c[:, :, 0::2, 0::2], c[:, :, 0::2, 1::2], c[:, :, 1::2, 0::2], c[:, :, 1::2, 1::2]], -1)


def pool(c, bias):
    """THE WINNER RULE (module docstring).  raw sums (N,C,H,W), bias (C,) -> (max(best + bias, 0) unrounded, byte)."""
    win = windows(c)
    best, bi = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for e in (1, 2, 3):
        gt = win[..., e] > best
        best = torch.where(gt, win[..., e], best)
        bi = torch.where(gt, torch.full_like(bi, e), bi)
    val = torch.clamp_min(best + bias.view(1, -1, 1, 1), 0.0)
    return val, torch.where(val > 0, bi, torch.full_like(bi, IDX_DEAD))


def conv_pool_fwd(a_in, w, b):
    """A pooled layer: bf16 input map (float64 values), f32 weights (rounded to bf16 here), f32 bias -> (bf16 map as float64, bytes)."""
    val, idx = pool(conv_raw(a_in, bf16_val(w.double())), b.double())
    return bf16_val(val), idx


def conv1_fwd(R, standardize, w1, b1):
    xn, mu, sd = image_bf16(R, standardize)
    a1, i1 = conv_pool_fwd(xn, w1, b1)
    return a1, i1, mu, sd


def last_fwd(a3, w, b, wfc=None, bfc=None):
    """Layer 4: -> dict(x, mask (N,96,12,12) bool, S = sum of ReLU, feat_div = f32(S / 144) (ss_c5_conv_last_fwd), feat_mul =
    f32(S * f32(1/144)) (ss_c5_conv_last_fwd_feat), z = bfc + feat_div . wfc^T in float64)."""
    x = conv_raw(a3, bf16_val(w.double())) + b.double().view(1, -1, 1, 1)
    S = torch.clamp_min(x, 0.0).sum(dim=(2, 3))
    out = dict(x=x, mask=x > 0, S=S, feat_div=f32_val(S / NPIX_LAST), feat_mul=f32_val(S * float(np.float32(1.0) / np.float32(NPIX_LAST))))
    if wfc is not None:
        out["z"] = out["feat_div"] @ wfc.double().t() + bfc.double()
    return out


def expand_dy(da, idx):
    """pooled-grid gradient (N,C,h,w) + bytes -> dense (N,C,2h,2w): the value at the position the byte names, nothing for byte 4."""
    n, c, h, w = da.shape
    out = da.new_zeros(n, c, h, 2, w, 2)
    for e in range(4):
        out[:, :, :, e >> 1, :, e & 1] = torch.where(idx == e, da, torch.zeros_like(da))
    return out.reshape(n, c, 2 * h, 2 * w)


def conv_wgrad(a_in, dy):
    """-> (g_w (COUT,CIN,3,3), g_b (COUT,)) summed over the frames, float64."""
    n, c, h, w = a_in.shape
    p = _pad(a_in)
    g = a_in.new_zeros(dy.shape[1], c, 3, 3)
    for ky in range(3):
        for kx in range(3):
            g[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", dy, p[:, :, ky:ky + h, kx:kx + w])
    return g, dy.sum(dim=(0, 2, 3))


def conv_dgrad(dy, w):
    """conv_transpose of the dense gradient with the bf16 weights, UNMASKED, rounded to bf16 (float64 values)."""
    return bf16_val(conv_dgrad_raw(dy, bf16_val(w.double())))


def conv_dgrad_raw(dy, wb):
    n, o, h, w = dy.shape
    p = _pad(dy)
    out = dy.new_zeros(n, wb.shape[1], h, w)
    for ky in range(3):
        for kx in range(3):  # da[y][x] += dy[y - ky + 1][x - kx + 1] w[ky][kx]
            out += torch.einsum("nohw,oc->nchw", p[:, :, 2 - ky:2 - ky + h, 2 - kx:2 - kx + w], wb[:, :, ky, kx])
    return out


def last_dy_df(dfeat144, mask):
    """dense gradient of the last layer from d feat * 144 = d z . W_fc (N,96): bf16(dfeat144 / 144) where the mask is set."""
    d = bf16_val(dfeat144.double() / NPIX_LAST)
    return d.view(*d.shape, 1, 1) * mask.double()


def last_dy_dz(dz, wfc, mask):
    return last_dy_df(dz.double() @ wfc.double(), mask)


def last_fc_grads(dz, feat):
    return dz.double().t() @ feat.double(), dz.double().sum(0)


def mask_to_kernel(mask):
    """(N,96,12,12) bool -> (N,144,96) uint8 as the kernels store it."""
    n = mask.shape[0]
    return mask.reshape(n, 96, NPIX_LAST).permute(0, 2, 1).contiguous().to(torch.uint8)


# ------------------------------------------------------------------------------------------------ lattice inputs
N_MAX = 11  # the largest frame count the suite uses: the weight-gradient sums over all frames are checked for it


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _blocks(g, n, hw, block, p_on):
    """(n,1,hw,hw) 0/1 float64, constant over block x block squares."""
    m = (torch.rand(n, 1, hw // block, hw // block, generator=g) < p_on).double()
    return m.repeat_interleave(block, 2).repeat_interleave(block, 3)


def check_lattice(name, sum_abs, unit, out):
    """sum |terms| of every element of an output, in its unit, must stay below 2^24."""
    m = float(sum_abs.max()) / unit if torch.is_tensor(sum_abs) else float(sum_abs) / unit
    assert m < LIMIT, f"{name}: sum |terms| = {m:.4g} units, not below 2^24"
    out[name] = m
    return m


def lattice_weights(seed, cout, cin, k):
    """(cout,cin,3,3) in {-2..2} 2^-k and a bias (multiples of 2^-k in [-6, 6]); channel 0 is killed (bias -16384 units, below
    every sum the suite can form: its every window is dead) and channel 1 has no weights and a positive bias (all tied, alive)."""
    g = _gen(seed)
    w = _ints(g, -2, 2, (cout, cin, 3, 3)) * 2.0 ** -k
    b = _ints(g, -6, 6, (cout,)) * 2.0 ** -k
    b[0] = -16384.0 * 2.0 ** -k
    w[1] = 0.0
    b[1] = 3.0 * 2.0 ** -k
    return w.float(), b.float()


def lattice_frames(seed, N=N_MAX):
    """uint8 frames with pixels from {0, 255}.  Frame 0: blocks of 0 / 255 beside a noisy region; 1: all 0; 2: all 255 (with a
    positive bias every inner window is tied and alive); the rest like frame 0."""
    g = _gen(seed)
    noisy = (torch.rand(N, 1, 96, 96, generator=g) < 0.5).double()
    blk = _blocks(g, N, 96, 8, 0.5)
    region = _blocks(g, N, 96, 16, 0.75)         # 1: block-constant, 0: noisy
    f = torch.where(region > 0, blk, noisy)
    if N > 1:
        f[1] = 0.0
    if N > 2:
        f[2] = 1.0
    return (f[:, 0] * 255).to(torch.uint8)


def lattice_act(seed, N, c, hw):
    """Activations in {0..3}: zero / constant blocks (tied windows) beside a random region.  Frame 1 is constant per channel."""
    g = _gen(seed)
    a = _ints(g, 0, 3, (N, c, hw, hw))
    keep = _blocks(g, N, hw, 4, 0.5)
    a = a * keep
    if N > 1:
        a[1] = _ints(g, 0, 3, (1, c, 1, 1)).expand(1, c, hw, hw)[0]
    return a


def lattice_grad(seed, shape, k):
    return _ints(_gen(seed), -2, 2, shape) * 2.0 ** -k


def lattice_bytes(seed, shape):
    return torch.randint(0, 5, shape, generator=_gen(seed)).to(torch.uint8)


def lattice_start(seed, shape, unit):
    """A nonzero accumulator start on the output's lattice."""
    g = _gen(seed)
    return ((_ints(g, 1, 5, shape)) * (2 * _ints(g, 0, 1, shape) - 1) * unit)


def tie_shares(c, b):
    """raw sums, bias -> (share of windows whose maximum is attained more than once, share of dead windows)."""
    win = windows(c)
    top = win.max(dim=-1, keepdim=True).values
    tied = ((win == top).sum(-1) > 1).double().mean().item()
    dead = ((top[..., 0] + b.double().view(1, -1, 1, 1)) <= 0).double().mean().item()
    return tied, dead


def assert_shares(name, c, b):
    tied, dead = tie_shares(c, b)
    assert tied >= 0.20, f"{name}: only {tied:.3f} of the pool windows are tied at the top"
    assert dead >= 0.05, f"{name}: only {dead:.3f} of the pool windows are dead"
    return tied, dead


K1, K2, K3, K4 = 3, 4, 5, 5     # the weights' powers of two, per layer
KD = 2                           # upstream gradients: {-2..2} 2^-KD


def make_pooled_layer(layer, N, seed=0):
    """Lattice inputs of one pooled layer (2 or 3) on its own: a_in in {0..3}, weights, bias; -> dict with the float64 reference."""
    cin, cout, hw = C5[layer - 1], C5[layer], 96 >> (layer - 1)
    k = (K2, K3)[layer - 2]
    a = lattice_act(100 * layer + seed, N, cin, hw)
    w, b = lattice_weights(200 * layer + seed, cout, cin, k)
    sums = {}
    unit = 2.0 ** -k
    check_lattice("conv", conv_raw(a.abs(), w.double().abs()) + b.double().abs().view(1, -1, 1, 1), unit, sums)
    c = conv_raw(a, w.double())
    shares = assert_shares(f"layer {layer}", c, b)
    a_out, idx = conv_pool_fwd(a, w, b)
    return dict(a_in=a, w=w, b=b, a_out=a_out, idx=idx, sums=sums, shares=shares, unit=unit)


def make_front(N, seed=0):
    """Lattice inputs of conv1 and conv2 as the fused kernels see them (standardize = 0): frames from {0, 255}, both layers'
    weights; a1 is then an integer number of 2^-K1 below 256 (bf16-exact), conv2's sums integers of 2^-(K1 + K2)."""
    R = lattice_frames(300 + seed, N)
    w1, b1 = lattice_weights(301 + seed, 16, 1, K1)
    w2, b2 = lattice_weights(302 + seed, 32, 16, K2)
    # (b2: multiples of 2^-K2 = 8 units of conv2's lattice 2^-(K1 + K2), up to 48 units: the size of the sums)
    b2[0] = -2.0 ** 20 * 2.0 ** -(K1 + K2)
    xn, mu, sd = image_bf16(R, 0)
    assert set(torch.unique(xn).tolist()) <= {0.0, 1.0}
    sums = {}
    u1, u2 = 2.0 ** -K1, 2.0 ** -(K1 + K2)
    check_lattice("conv1", conv_raw(xn, w1.double().abs()) + b1.double().abs().view(1, -1, 1, 1), u1, sums)
    c1 = conv_raw(xn, w1.double())
    sh1 = assert_shares("conv1", c1, b1)
    v1, i1 = pool(c1, b1.double())
    a1 = bf16_val(v1)
    assert torch.equal(a1, v1), "a1 is not bf16-exact on the lattice"
    check_lattice("conv2", conv_raw(a1, w2.double().abs()) + b2.double().abs().view(1, -1, 1, 1), u2, sums)
    c2 = conv_raw(a1, w2.double())
    sh2 = assert_shares("conv2", c2, b2)
    a2, i2 = conv_pool_fwd(a1, w2, b2)
    st = torch.stack([mu, sd], 1).contiguous()
    return dict(R=R, w1=w1, b1=b1, w2=w2, b2=b2, xn=xn, st=st, a1=a1, i1=i1, a2=a2, i2=i2, sums=sums, shares=(sh1, sh2), u1=u1, u2=u2)


def make_last(N, E, seed=0, dyadic=False):
    """Lattice inputs of the last layer.  ``dyadic``: every channel is either linear (weights and bias >= 0: no ReLU acts) or dead
    (weights <= 0, bias < 0), a3 lives on the inner 10 x 10 pixels only (every tap then sees every pixel) and each channel of each
    frame sums to 144: S is a multiple of 144 units, feat = S / 144 sits on the lattice and z is exact too.  Otherwise signs are
    free: x, the mask and S are exact, feat is S / 144 rounded once, z is not on a lattice (not compared)."""
    g = _gen(400 + seed + 7 * E)
    u = 2.0 ** -K4
    if dyadic:
        a3 = torch.zeros(N, 64, 12, 12, dtype=torch.float64)
        inner = torch.ones(N, 64, 100, dtype=torch.float64)          # 100 ones + 44 more spread over random pixels: sum 144
        extra = torch.randint(0, 100, (N, 64, 44), generator=g)
        inner.scatter_add_(2, extra, torch.ones(N, 64, 44, dtype=torch.float64))
        inner = inner.clamp_max(3.0)
        deficit = 144 - inner.sum(-1)                                # what the clamp took away goes onto pixels still at 1
        for n in range(N):
            for c in range(64):
                d = int(deficit[n, c])
                if d:
                    ones = (inner[n, c] == 1).nonzero()[:d, 0]
                    inner[n, c, ones] += 1
        assert bool((inner.sum(-1) == 144).all()) and float(inner.max()) <= 3
        a3[:, :, 1:11, 1:11] = inner.view(N, 64, 10, 10)
        w = _ints(g, 0, 2, (96, 64, 3, 3)) * u
        b = _ints(g, 0, 6, (96,)) * u
        deadc = torch.arange(96) % 5 == 0
        w[deadc] = -w[deadc]
        b[deadc] = -(b[deadc] + u)
    else:
        a3 = lattice_act(401 + seed, N, 64, 12)
        w = _ints(g, -2, 2, (96, 64, 3, 3)) * u
        b = _ints(g, -6, 6, (96,)) * u
        b[0] = -16384.0 * u
        w[1] = 0.0
        b[1] = 3 * u
        w[2] = 0.0
        b[2] = 0.0                                                   # x is exactly 0 everywhere: mask 0 (x > 0 is strict)
    wfc = (_ints(g, -2, 2, (E, 96)) * 0.25).float()
    bfc = (_ints(g, -6, 6, (E,)) * 0.25).float()
    w, b = w.float(), b.float()
    sums = {}
    xa = conv_raw(a3, w.double().abs()) + b.double().abs().view(1, -1, 1, 1)
    check_lattice("x", xa, u, sums)
    check_lattice("S", xa.sum(dim=(2, 3)), u, sums)
    ref = last_fwd(a3, w, b, wfc, bfc)
    if dyadic:
        assert torch.equal(ref["S"] / NPIX_LAST, ref["feat_div"]) and torch.equal(ref["feat_div"], ref["feat_mul"])
        assert bool(((ref["feat_div"] / u) == torch.round(ref["feat_div"] / u)).all()), "feat is not on the lattice"
        check_lattice("z", ref["feat_div"].abs() @ wfc.double().abs().t() + bfc.double().abs(), u * 0.25, sums)
        assert torch.equal(f32_val(ref["z"]), ref["z"])
    return dict(a3=a3, w=w, b=b, wfc=wfc, bfc=bfc, ref=ref, sums=sums, unit=u)


def make_last_bwd(N, E, seed=0):
    """Lattice inputs of the last layer's backward: a3 in {0..3}, a random mask with dead and full channels, dz = 144 x
    {-2..2} / 4 (f32, so that d z . W_fc / 144 is on the lattice and its bf16 rounding is no rounding), wfc in {-2..2} / 4,
    feat on the lattice (an input of the fc gradients)."""
    g = _gen(500 + seed + 7 * E)
    a3 = lattice_act(501 + seed, N, 64, 12)
    mask = torch.rand(N, 96, 12, 12, generator=g) < 0.5
    mask[:, 0] = False
    mask[:, 1] = True
    dz = _ints(g, -2, 2, (N, E)) * 0.25 * NPIX_LAST
    wfc = _ints(g, -2, 2, (E, 96)) * 0.25
    feat = _ints(g, 0, 40, (N, 96)) * 0.125
    w = _ints(g, -2, 2, (96, 64, 3, 3)) * 2.0 ** -K4
    df = dz @ wfc                                                  # d feat * 144: multiples of 144 / 16, |.| <= 64 * 144 / 4
    dy = last_dy_df(df, mask)
    assert torch.equal(dy, (df / NPIX_LAST).view(N, 96, 1, 1) * mask.double()), "bf16(d feat / 144) rounds on the lattice"
    sums = {}
    ud = 1.0 / 16
    check_lattice("dfeat", dz.abs() @ wfc.abs(), ud, sums)
    big = N_MAX / N                                                # the sums over N_MAX frames of the same kind
    ga, gb = conv_wgrad(a3, dy.abs())
    check_lattice("g_w", ga * big + 5 * ud, ud, sums)
    check_lattice("g_b", gb * big + 5 * ud, ud, sums)
    check_lattice("g_wfc", (dz.abs().t() @ feat) * big + 5 * ud, 0.25 * 0.125, sums)
    check_lattice("da3", conv_dgrad_raw(dy.abs(), w.abs()), ud * 2.0 ** -K4, sums)
    g_w, g_b = conv_wgrad(a3, dy)
    g_wfc, g_bfc = last_fc_grads(dz, feat)
    return dict(a3=a3, mask=mask, dz=dz.float(), wfc=wfc.float(), feat=feat.float(), w=w.float(), df=df.float(), dy=dy, g_w=g_w, g_b=g_b,
                g_wfc=g_wfc, g_bfc=g_bfc, da3=conv_dgrad(dy, w), sums=sums, unit=ud)


def make_pooled_bwd(layer, N, seed=0, a_in=None, u_in=1.0):
    """Lattice inputs of a pooled layer's backward (2 or 3): a_in in {0..3} (or given, in units of ``u_in``: the front's a1), da in
    {-2..2} 2^-KD, random bytes 0..4, weights for the data gradient."""
    cin, cout, hw = C5[layer - 1], C5[layer], 96 >> (layer - 1)
    k = (K2, K3)[layer - 2]
    if a_in is None:
        a_in = lattice_act(600 * layer + seed, N, cin, hw)
    da = lattice_grad(601 * layer + seed, (N, cout, hw // 2, hw // 2), KD)
    idx = lattice_bytes(602 * layer + seed, (N, cout, hw // 2, hw // 2))
    w, _ = lattice_weights(603 * layer + seed, cout, cin, k)
    dy = expand_dy(da, idx)
    sums = {}
    ua = u_in
    assert bool(((a_in / ua) == torch.round(a_in / ua)).all())
    ud = 2.0 ** -KD
    big = N_MAX / N
    ga, gb = conv_wgrad(a_in, dy.abs())
    check_lattice("g_w", ga * big + 5 * ua * ud, ua * ud, sums)
    check_lattice("g_b", gb * big + 5 * ud, ud, sums)
    check_lattice("da_in", conv_dgrad_raw(dy.abs(), w.double().abs()), ud * 2.0 ** -k, sums)
    g_w, g_b = conv_wgrad(a_in, dy)
    return dict(a_in=a_in, da=da, idx=idx, w=w, dy=dy, g_w=g_w, g_b=g_b, da_in=conv_dgrad(dy, w), sums=sums, u_w=ua * ud, u_b=ud)


def make_conv1_bwd(front, da1, i1, unit):
    """conv1's weight gradient on the front's frames: da1 (N,16,48,48) float64, bf16-exact multiples of ``unit``, routed by ``i1``."""
    xn = front["xn"]
    N = xn.shape[0]
    dy = expand_dy(da1, i1)
    assert bool(((da1 / unit) == torch.round(da1 / unit)).all())
    sums = {}
    big = N_MAX / N
    ga, gb = conv_wgrad(xn, dy.abs())
    check_lattice("g_w1", ga * big + 5 * unit, unit, sums)
    check_lattice("g_b1", gb * big + 5 * unit, unit, sums)
    g_w, g_b = conv_wgrad(xn, dy)
    return dict(g_w=g_w, g_b=g_b, unit=unit, sums=sums)
