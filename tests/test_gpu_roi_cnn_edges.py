"""GPU: the f32 ROI CNN at the edges of its ABI -- every embedding width, both normalisations, exact pool ties, single frames,
the grid boundary, wide rows -- frame by frame against the float64 reference of tests/roi_cnn_ref.py; the fused kernels against
the layer-by-layer path on thousands of frames; and the seven building blocks of that path one by one.

Tolerances are multiples of the reference's own error: a tensor of a frame must lie within ``k * e_ref + floor`` of the float64
value, e_ref = max |float32 reference - float64 reference| on the same inputs, floor = 4 float32 ulps of the tensor's largest
magnitude (roi_cnn_ref.bound).  The three values of k and the ratios observed on the MI355X are in docs/LAB_NOTES.md section 9:
K = 64 in general; K_CONST = 4 for the gradients of a constant frame under standardize = 1 (its ``out``: the floor alone, k = 0);
K_AMP = 4 where the float32 reference itself leaves the older contract, which is allowed only for the named cases (frames with a
std below 1e-3 under standardize = 1, the network with all weights times 30).  Everywhere else the contract numbers of
tests/test_gpu_kernels.py are asserted to be upper bounds: the tolerance applied is the smaller of the two at every element.
Integer outputs (pool winners, masks, im2col, pool gradients) are compared exactly.  Every figure is printed before it is
asserted (``-s`` shows them: lines starting with ``RATIO``).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import roi_cnn_ref as RR
from gpu_support import L  # noqa: F401
from roi_cnn_ref import CNN_KEYS

pytestmark = pytest.mark.gpu

K = 64        # docs/LAB_NOTES.md section 9: twice the largest observed (kernel error / e_ref) = 2 x 22.2, rounded up to a power of two
K_CONST = 4   # gradients of a constant frame, standardize = 1: 2 x 1.99 observed (sums of 1 024 ... 4 608 addends that cancel)
K_AMP = 4     # where the float32 reference itself is outside the older contract (named cases only): observed 1.0
X_DIM = 84    # d_out / out live in the engine's Z matrix: X_DIM landmark columns, then the E embedding columns
SENT = -3.0
SLACK = 2048  # floats behind every gradient buffer that must stay zero
GEOMS = RR.GEOMS
ALL_E = (1, 7, 16, 17, 32, 48, 63, 64)


_KEEP = []


def dev(t):
    """Host -> device copy that stays alive until the next sync() (see tests/test_gpu_kernels.py)."""
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


def sync():
    torch.cuda.synchronize()
    _KEEP.clear()


def report(name, got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    idx = int(err.argmax())
    return f"{name}: max abs err {float(err.max()):.3e} at flat {idx} (got {float(got.reshape(-1)[idx]):.6g}, ref {float(ref.reshape(-1)[idx]):.6g}), ref scale {float(ref.abs().max()):.3e}"


def assert_close(name, got, ref, atol, rtol=0.0):
    g = got.detach().double().cpu()
    r = ref.detach().double().cpu()
    assert g.shape == r.shape, (name, g.shape, r.shape)
    assert torch.isfinite(g).all(), name + " has non-finite values"
    bad = (g - r).abs() > atol + rtol * r.abs()
    if bad.any():
        pytest.fail(report(name, got, ref) + f"; {int(bad.sum())}/{bad.numel()} outside atol={atol} rtol={rtol}", pytrace=False)


def cap_out(ref):  # the contract of test_roi_cnn_fwd for an embedding
    return 2e-5 + 1e-4 * ref.abs()


def cap_grad(ref):  # the contract of test_roi_cnn_stash_and_bwd for a gradient tensor
    return 3e-4 * max(float(ref.abs().max()), 1e-3) + 1e-3 * ref.abs()


def check_bound(tag, name, got, ref64, e_ref, cap, fails, k=K, ref32=None, amplified=False):
    """|got - ref64| <= k * e_ref + floor at every element, floor = 4 float32 ulps of the largest |ref64|, and never looser than
    ``cap(ref64)``, the older contract for the quantity: where the float32 reference meets that contract the tolerance is the
    smaller of the two at every element.  Where the float32 REFERENCE itself is outside it, no float32 implementation can be held
    to it against float64: that is accepted only for a case the caller names (``amplified``: a frame with a std below 1e-3 under
    standardize = 1, where 1 / std multiplies the float32 rounding of u / 255 - mean; the network with all weights times 30), and
    the kernel is then held to K_AMP * e_ref + floor (observed: 1.0 e_ref), not to the general K.  Prints the k this tensor would
    have needed; appends to ``fails`` instead of raising so that a test reports every tensor."""
    g, r64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r64.shape, (name, g.shape, r64.shape)
    floor = 4.0 * RR.ulp32(r64.abs().max())
    if cap is not None:
        c = cap(r64)
        if ref32 is None or bool(((ref32.double() - r64).abs() <= c).all()):
            tol = torch.minimum(torch.full_like(r64, k * e_ref + floor), c)
            assert bool((tol <= c).all()), "the bound in use is looser than the older contract"
        else:
            assert amplified, f"{tag} {name}: the float32 reference is outside the older contract on a case that is not one of the named ones"
            k = min(k, K_AMP)
            tol = torch.full_like(r64, k * e_ref + floor)
            print(f"RATIO {tag} {name}: the float32 reference itself is outside the older contract; held to {k} * e_ref + floor")
    else:
        tol = torch.full_like(r64, k * e_ref + floor)
    b = k * e_ref + floor
    err = float((g - r64).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
    need = RR.needed_k(err, e_ref, floor)
    print(f"RATIO {tag} {name}: err {err:.3e} e_ref {e_ref:.3e} floor {floor:.3e} ulps {err / (floor / 4) if floor else 0.0:.1f} k_needed {need:.2f}")
    if not bool(((g - r64).abs() <= tol).all()):  # (NaN compares false)
        fails.append(f"{tag} {report(name, g, r64)}; bound {b:.3e} = {k} * {e_ref:.3e} + {floor:.3e}, k needed {need:.1f}")
    return need


def check_rule(tag, name, got, ref32, ref64, cap, fails, k=K, amplified=False):
    """One tensor of one frame (or one summed tensor): e_ref = max |float32 reference - float64 reference|."""
    return check_bound(tag, name, got, ref64, float((ref32.double() - ref64.double()).abs().max()), cap, fails, k=k, ref32=ref32,
                       amplified=amplified)


def frame_k(R, standardize, x30=False):
    """Per frame: (k for ``out``, k for a gradient, amplified).  Constant frames under standardize = 1 normalise to exactly 0: the
    float64 network of a zero image is their only reference, ``out`` must meet it within the floor alone (k = 0), their gradients
    within K_CONST * e_ref, e_ref from the two precisions of that zero-image network."""
    const, amp = RR.frame_kinds(R)
    rows = []
    for n in range(R.shape[0]):
        if standardize and bool(const[n]):
            rows.append((0, K_CONST, x30))
        else:
            rows.append((K, K, x30 or bool(standardize and amp[n])))
    return rows


def flush(fails):
    if fails:
        pytest.fail(f"{len(fails)} tensors outside K * e_ref + floor:\n" + "\n".join(fails[:40]), pytrace=False)


# ------------------------------------------------------------------------------------------------ fused kernels: plumbing
def params(E, seed=21, kind=None):
    import weights as W

    sd = W.make_state_dict(seed, X_DIM, 5, True, roi_emb=E)
    sd = {k: v.clone() for k, v in sd.items() if k.startswith("roi_cnn.")}
    if kind == "dead":  # every ReLU dead
        for k in (CNN_KEYS[1], CNN_KEYS[3], CNN_KEYS[5]):
            sd[k].fill_(-10.0)
    elif kind == "x30":
        for k in CNN_KEYS:
            sd[k] *= 30.0
    elif kind == "wfc0":
        sd[CNN_KEYS[6]].zero_()
    return sd


def d_out_for(N, E, seed=9):
    return torch.randn(N, E, generator=torch.Generator().manual_seed(seed + 100 * E))


class Fused:
    """One forward-with-stash launch of the fused kernels over R (N,H,W) and the backward launches that reuse its stash."""

    def __init__(self, L, R, sd, E, standardize):
        self.L, self.E, self.std = L, E, int(standardize)
        self.N, self.H, self.W = R.shape
        N, H, W = R.shape
        self.P = [sd[k].contiguous().cuda() for k in CNN_KEYS]
        self.R = R.contiguous().cuda()
        self.ld = X_DIM + E
        self.Z = torch.full((N, self.ld), SENT, device="cuda")
        self.sizes = L.cnn_stash_sizes(H, W)
        n_a1, n_a2, n_i1, n_i2, n_m3, n_feat = self.sizes
        u8 = dict(device="cuda", dtype=torch.uint8)
        self.st = [torch.zeros(N, n_a1, device="cuda"), torch.zeros(N, n_i1, **u8), torch.zeros(N, n_a2, device="cuda"),
                   torch.zeros(N, n_i2, **u8), torch.zeros(N, n_m3, **u8), torch.zeros(N, n_feat, device="cuda")]
        L.call("ss_roi_cnn_fwd_stash", self.R.data_ptr(), N, H, W, self.std, *[p.data_ptr() for p in self.P], E,
               self.Z.data_ptr() + 4 * X_DIM, self.ld, *[s.data_ptr() for s in self.st], self.sizes.ptr, L.stream())
        sync()
        self.out = self.Z[:, X_DIM:]
        H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
        self.i1 = self.st[1].view(N, 8, -1)[:, :, : H2 * W2].reshape(N, 8, H2, W2).cpu()  # planes are padded
        self.i2 = self.st[3].view(N, H4, W4, 16).permute(0, 3, 1, 2).contiguous().cpu()  # pixel-major in the stash
        self.m3 = self.st[4].view(N, H4 * W4, 32).cpu()

    def untouched(self):
        return bool(torch.all(self.Z[:, :X_DIM] == SENT))

    def bwd(self, d_out, frames=None):
        """Gradients into zeroed buffers.  d_out sits in columns [X_DIM, X_DIM + E) of a matrix whose other columns are NaN (and
        one spare NaN row behind the last frame): a kernel that reads outside a row's E poisons a gradient."""
        L, N, E = self.L, self.N, self.E
        dz = torch.full((N + 1, self.ld), float("nan"), device="cuda")
        dz[:N, X_DIM:] = d_out.cuda()
        # every gradient buffer is followed by SLACK zeroed floats that must still be zero afterwards: E-dependent indexing that
        # runs past E * 24 (or past any other tensor's end) shows up there instead of in somebody else's memory
        B = [torch.zeros(p.numel() + SLACK, device="cuda") for p in self.P]
        G = [b[: p.numel()].view(p.shape) for b, p in zip(B, self.P)]
        args = [self.R.data_ptr(), N, self.H, self.W, self.std, *[p.data_ptr() for p in self.P], E,
                *[s.data_ptr() for s in self.st], self.sizes.ptr, dz.data_ptr() + 4 * X_DIM, self.ld, *[g.data_ptr() for g in G]]
        if frames is None:
            L.call("ss_roi_cnn_bwd", *args, L.stream())
        else:
            fl = dev(torch.tensor([len(frames)] + list(frames) + [0] * (N - len(frames)), dtype=torch.int32))
            L.call("ss_roi_cnn_bwd_frames", *args, fl.data_ptr(), L.stream())
        sync()
        for k, b, p in zip(CNN_KEYS, B, self.P):
            assert float(b[p.numel():].abs().max()) == 0.0, f"the backward wrote behind the end of the gradient of {k}"
        return dict(zip(CNN_KEYS, [g.cpu() for g in G]))


_REF = {}


def reference(H, W, E, standardize, kind=None):
    """The frame set of section B with its float32 and float64 references (cached: forward and backward tests share them)."""
    key = (H, W, E, standardize, kind)
    if key not in _REF:
        sd = params(E, kind=kind)
        R, names = RR.frame_set(H, W, 5, 4)
        d_out = d_out_for(R.shape[0], E)
        r32 = RR.cnn_fwd_bwd(R, sd, d_out, standardize, torch.float32, constant_is_zero=True)
        r64 = RR.cnn_fwd_bwd(R, sd, d_out, standardize, torch.float64, constant_is_zero=True)
        for r, drop in ((r32, ("x", "y1", "y2", "y3", "a1", "a2", "i1", "i2", "m3")), (r64, ("x", "a2", "i1", "i2", "m3"))):
            for k in drop:  # the forward and the backward test of a case share this entry: keep what they read
                del r[k]
        _REF[key] = (sd, R, names, d_out, r32, r64)
    return _REF[key]


def check_argmax(tag, name, got, y64, names, fails):
    """Pool winners, exactly, on every window with a positive maximum that is exactly tied in float64 (the first maximal position
    in row-major order must win) or separated by more than 1e-4; windows with a gap in (0, 1e-4] are left out, at most 2 %."""
    keep, c = RR.comparable(y64)
    n_pos, n_left = int(c["positive"].sum()), int((c["positive"] & c["close"]).sum())
    n_tied = int((c["positive"] & c["tied"]).sum())
    assert n_left <= 0.02 * n_pos, f"{tag} {name}: {n_left} of {n_pos} windows left out"
    bad = keep & (got != c["first"])
    print(f"RATIO {tag} {name}: {n_pos} positive windows, {n_tied} exactly tied, {n_left} left out, {int(bad.sum())} mismatches "
          f"({int((bad & c['tied']).sum())} on tied windows)")
    if bad.any():
        w = RR.windows(y64)
        lines = []
        for n, ch, py, px in bad.nonzero()[:6].tolist():
            lines.append(f"  frame {names[n]} ch {ch} window ({py},{px}): values {w[n, ch, py, px].tolist()} tied={bool(c['tied'][n, ch, py, px])} "
                         f"got {int(got[n, ch, py, px])} want {int(c['first'][n, ch, py, px])}")
        per = {names[n]: int(bad[n].sum()) for n in range(bad.shape[0]) if bad[n].any()}
        fails.append(f"{tag} {name}: {int(bad.sum())} argmax mismatches of {int(keep.sum())} compared ({int((bad & c['tied']).sum())} on "
                     f"exactly tied windows), per frame {per}\n" + "\n".join(lines))


CASES_C = [(H, W, E, s) for (H, W) in GEOMS for E in ALL_E for s in (1, 0)]


# ------------------------------------------------------------------------------------------------ C: forward, frame by frame
@pytest.mark.parametrize("H,W,E,standardize", CASES_C)
def test_fwd_every_frame_every_width(L, H, W, E, standardize):
    sd, R, names, d_out, r32, r64 = reference(H, W, E, standardize)
    tag = f"{H}x{W} E={E} std={standardize}"
    N = R.shape[0]
    f = Fused(L, R, sd, E, standardize)
    assert f.untouched(), "ss_roi_cnn_fwd_stash wrote outside its E columns"
    # the plain forward: same rows, a wider matrix, columns on both sides of the embedding
    ld = X_DIM + E + 5
    Z = torch.full((N, ld), SENT, device="cuda")
    L.call("ss_roi_cnn_fwd", f.R.data_ptr(), N, H, W, standardize, *[p.data_ptr() for p in f.P], E, Z.data_ptr() + 4 * X_DIM, ld,
           L.stream())
    sync()
    assert bool(torch.all(Z[:, :X_DIM] == SENT)) and bool(torch.all(Z[:, X_DIM + E:] == SENT)), "ss_roi_cnn_fwd wrote outside its E columns"
    assert torch.equal(Z[:, X_DIM:X_DIM + E], f.out), "the stash must not change the embedding"
    fails = []
    out = f.out.cpu()
    fk = frame_k(R, standardize)
    for n in range(N):
        check_rule(tag, f"out[{names[n]}]", out[n], r32["out"][n], r64["out"][n], cap_out, fails, k=fk[n][0], amplified=fk[n][2])
    check_argmax(tag, "i1", f.i1, r64["y1"], names, fails)
    check_argmax(tag, "i2", f.i2, r64["y2"], names, fails)
    y3 = r64["y3"].reshape(N, 24, -1)
    sure3 = y3.abs() > 1e-4
    m3 = f.m3[:, :, :24].permute(0, 2, 1).bool()
    n_left3 = int((~sure3).sum())
    print(f"RATIO {tag} m3: {sure3.numel()} conv3 outputs, {n_left3} within 1e-4 of zero left out, {int((m3 != (y3 > 0))[sure3].sum())} mismatches")
    assert n_left3 <= 0.02 * sure3.numel(), f"{tag} conv3 sign mask: {n_left3} of {sure3.numel()} outputs left out"
    if not torch.equal(m3[sure3], (y3 > 0)[sure3]):
        fails.append(f"{tag} conv3 sign mask: {int((m3 != (y3 > 0))[sure3].sum())} mismatches")
    assert int(f.m3[:, :, 24:].sum()) == 0
    flush(fails)


# ------------------------------------------------------------------------------------------------ C: backward, one frame at a time
@pytest.mark.parametrize("H,W,E,standardize", CASES_C)
def test_bwd_one_frame_at_a_time(L, H, W, E, standardize):
    """ss_roi_cnn_bwd_frames with a one-entry list for each special frame of section B, against that frame's float64 gradients:
    the summed comparison of test_roi_cnn_stash_and_bwd cannot see a wrong frame among 270."""
    sd, R, names, d_out, r32, r64 = reference(H, W, E, standardize)
    tag = f"{H}x{W} E={E} std={standardize}"
    f = Fused(L, R, sd, E, standardize)
    fails = []
    fk = frame_k(R, standardize)
    for n in range(len(RR.SPECIAL)):
        G = f.bwd(d_out, frames=[n])
        for k in CNN_KEYS:
            check_rule(tag, f"{k}[{names[n]}]", G[k], r32["grads"][k][n], r64["grads"][k][n], cap_grad, fails, k=fk[n][1], amplified=fk[n][2])
    # and N = 1 through ss_roi_cnn_bwd: a grid of one workgroup, no list
    for n in (names.index("grey8"), names.index("px_corner")):
        f1 = Fused(L, R[n:n + 1], sd, E, standardize)
        assert torch.equal(f1.out, f.out[n:n + 1]), "a frame's embedding must not depend on N"
        G = f1.bwd(d_out[n:n + 1])
        for k in CNN_KEYS:
            check_rule(tag, f"N=1 {k}[{names[n]}]", G[k], r32["grads"][k][n], r64["grads"][k][n], cap_grad, fails, k=fk[n][1], amplified=fk[n][2])
    flush(fails)


@pytest.mark.parametrize("H,W", GEOMS)
def test_bwd_without_standardize_takes_no_statistics_from_the_stash(L, H, W):
    """standardize = 0 is the mu = 0, sd = 1 branch of the backward's grey-level table: xn = u / 255 whatever the mean / std slots
    of st_feat hold (the forward leaves 0 and 1 there, so only a stash with other numbers in them tells the branches apart)."""
    E = 17
    sd, R, names, d_out, r32, r64 = reference(H, W, E, 0)
    f = Fused(L, R, sd, E, 0)
    assert torch.equal(f.st[5][:, 48:50].cpu(), torch.tensor([0.0, 1.0]).expand(R.shape[0], 2))
    G0 = f.bwd(d_out)
    f.st[5][:, 48] = 0.25
    f.st[5][:, 49] = 3.0
    G1 = f.bwd(d_out)
    fails = []
    for k in CNN_KEYS:
        check_rule(f"{H}x{W} std=0 other statistics in the stash", k, G1[k], r32["grads"][k].sum(0), r64["grads"][k].sum(0), cap_grad, fails)
        spread = float((G1[k] - G0[k]).abs().max()) / max(float(G0[k].abs().max()), 1e-30)
        assert spread < 2e-5, f"{k}: moved by {spread:.1e} of its largest entry with the statistics slots"  # float atomics reorder
    flush(fails)


# ------------------------------------------------------------------------------------------------ C: backward, summed, at the grid boundary
_SUM_REF = {}
SUMMED = [(64, 64, n) for n in (1, 255, 256, 257, 513)] + [(48, 96, n) for n in (1, 257)] + [(32, 32, n) for n in (1, 256, 513)]


@pytest.mark.parametrize("H,W,N", SUMMED)
@pytest.mark.parametrize("cap", [0, 3], ids=["grid_default", "grid_3"])  # (innermost: the two caps of a case share its references)
def test_bwd_summed_at_the_grid_boundary(L, H, W, N, cap):
    E = 64 if N % 2 else 17
    standardize = 0 if N in (255, 513) else 1
    sd = params(E, seed=22)
    R = RR.frames_n(H, W, N, 11)
    d_out = d_out_for(N, E, seed=4)
    tag = f"{H}x{W} N={N} E={E} std={standardize} cap={cap}"
    if (H, W, N) not in _SUM_REF:  # the references do not depend on the grid cap
        _SUM_REF.clear()
        _SUM_REF[(H, W, N)] = (RR.cnn_sum_grads(R, sd, d_out, standardize, torch.float32, constant_is_zero=True),
                               RR.cnn_sum_grads(R, sd, d_out, standardize, torch.float64, constant_is_zero=True))
    (o32, g32), (o64, g64) = _SUM_REF[(H, W, N)]
    L.call("ss_roi_cnn_set_max_workgroups", cap)
    try:
        f = Fused(L, R, sd, E, standardize)
        G = f.bwd(d_out)
    finally:
        L.call("ss_roi_cnn_set_max_workgroups", 0)
    fails = []
    assert f.untouched()
    out = f.out.cpu()
    fk = frame_k(R, standardize)
    for n in range(N):
        check_rule(tag, f"out[{n}]", out[n], o32[n], o64[n], cap_out, fails, k=fk[n][0], amplified=fk[n][2])
    some_amp = any(a for _, _, a in fk)
    for k in CNN_KEYS:
        check_rule(tag, k, G[k], g32[k], g64[k], cap_grad, fails, amplified=some_amp)
    flush(fails)


# ------------------------------------------------------------------------------------------------ C: dead and saturated networks
@pytest.mark.parametrize("H,W", GEOMS)
@pytest.mark.parametrize("kind", ["dead", "x30", "wfc0"])
def test_dead_and_saturated_networks(L, H, W, kind):
    E = 17
    sd, R, names, d_out, r32, r64 = reference(H, W, E, 1, kind)
    tag = f"{H}x{W} {kind}"
    N = R.shape[0]
    f = Fused(L, R, sd, E, 1)
    out = f.out.cpu()
    G = f.bwd(d_out)
    s32 = {k: r32["grads"][k].sum(0) for k in CNN_KEYS}
    s64 = {k: r64["grads"][k].sum(0) for k in CNN_KEYS}
    fails = []
    if kind == "dead":  # every conv bias at -10: no ReLU passes anything
        # (the one-pixel frames normalise that pixel to about sqrt(H W): a few conv1 outputs around it do get past -10, nothing
        # gets past conv3's)
        assert bool((r64["y3"] <= 0).all()) and float(r64["feat"].abs().max()) == 0, "the inputs are meant to leave the network dead"
        assert torch.equal(out, sd[CNN_KEYS[7]].expand(N, E)), "out must be b_fc exactly"
        assert int(f.m3.sum()) == 0
        for k in CNN_KEYS[:7]:
            assert float(G[k].abs().max()) == 0.0, f"{k} must be exactly zero"
        check_rule(tag, CNN_KEYS[7], G[CNN_KEYS[7]], s32[CNN_KEYS[7]], s64[CNN_KEYS[7]], cap_grad, fails, amplified=True)
    else:
        fk = frame_k(R, 1, x30=kind == "x30")
        for n in range(N):
            check_rule(tag, f"out[{names[n]}]", out[n], r32["out"][n], r64["out"][n], cap_out, fails, k=fk[n][0], amplified=fk[n][2])
        for k in CNN_KEYS:
            if kind == "wfc0" and k in CNN_KEYS[:6]:  # d feat = d_out . W_fc = 0
                assert float(G[k].abs().max()) == 0.0, f"{k} must be exactly zero"
            else:
                check_rule(tag, k, G[k], s32[k], s64[k], cap_grad, fails, amplified=True)  # (the set holds the px_* frames)
    flush(fails)


# ------------------------------------------------------------------------------------------------ C: rejections
def test_rejected_on_the_host(L):
    """E outside 1..64 and leading dimensions below E are refused before anything is launched: outputs keep their sentinel."""
    H, W, N = 32, 32, 3
    R = RR.frames_n(H, W, N, 1)
    sd = params(64)
    f = Fused(L, R, sd, 64, 1)
    wide = [torch.cat([sd[CNN_KEYS[6]], sd[CNN_KEYS[6]][:1]]).cuda(), torch.cat([sd[CNN_KEYS[7]], sd[CNN_KEYS[7]][:1]]).cuda()]
    P65 = f.P[:6] + wide  # a well-formed E = 65 layer: the refusal is about the shape, not about short buffers
    Z = torch.full((N, 200), SENT, device="cuda")
    G = [torch.full((p.numel() + 64,), SENT, device="cuda") for p in P65]
    dz = torch.zeros(N, 200, device="cuda")

    def fwd(name, P, E, ld, *more):
        L.call(name, f.R.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], E, Z.data_ptr(), ld, *more, L.stream())

    def bwd(P, E, ld):
        L.call("ss_roi_cnn_bwd", f.R.data_ptr(), N, H, W, 1, *[p.data_ptr() for p in P], E, *[s.data_ptr() for s in f.st],
               f.sizes.ptr, dz.data_ptr(), ld, *[g.data_ptr() for g in G], L.stream())

    stash = [*[s.data_ptr() for s in f.st], f.sizes.ptr]
    with pytest.raises(RuntimeError, match="unsupported"):
        fwd("ss_roi_cnn_fwd", P65, 65, 200)
    with pytest.raises(RuntimeError, match="unsupported"):
        fwd("ss_roi_cnn_fwd_stash", P65, 65, 200, *stash)
    with pytest.raises(RuntimeError, match="unsupported"):
        bwd(P65, 65, 200)
    for E, ld in ((0, 200), (-1, 200), (64, 63), (17, 16)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            fwd("ss_roi_cnn_fwd", f.P, E, ld)
        with pytest.raises(RuntimeError, match="invalid argument"):
            fwd("ss_roi_cnn_fwd_stash", f.P, E, ld, *stash)
        with pytest.raises(RuntimeError, match="invalid argument"):
            bwd(f.P, E, ld)
    sync()
    assert bool(torch.all(Z == SENT)) and all(bool(torch.all(g == SENT)) for g in G)


# ------------------------------------------------------------------------------------------------ D: fused against layer by layer
@pytest.mark.parametrize("H,W,E,standardize,N,chunk_rows", [
    (64, 64, 32, 1, 2048, None), (64, 64, 17, 0, 1500, 4096 * 700), (48, 96, 64, 1, 1100, None),
    (32, 32, 17, 1, 3000, None), (32, 32, 64, 0, 2500, 1024 * 900), (48, 96, 17, 0, 1030, None)])
def test_fused_equals_layer_by_layer(L, H, W, E, standardize, N, chunk_rows, monkeypatch):
    """Two independent device implementations of one function -- LDS-resident fused kernels and im2col + GEMM -- on thousands of
    frames.  ``out``: e_ref is the largest per-frame e_ref of a 64-frame CPU subsample of the same set; both paths are within the
    rule of the float64 value there, and they are compared with each other under the same bound on every frame.  Gradients: summed
    over three disjoint subsets (selected by zeroing the other rows of d_out); each subset has its own float32 and float64 CPU
    reference (a few hundred frames: seconds), so e_ref is measured on the very frames that are summed, nothing is extrapolated,
    and each path is held to the rule on its own -- which also says which path carries an error."""
    from silent_speech_amd import cnn_generic

    if chunk_rows:
        monkeypatch.setattr(cnn_generic, "MAX_GEMM_ROWS", chunk_rows)
    tag = f"{H}x{W} E={E} std={standardize} N={N}"
    sd = params(E, seed=23)
    R = RR.tiled_set(H, W, N, 31)
    d_out = d_out_for(N, E, seed=6)
    pick = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:64].sort().values
    r32 = RR.cnn_fwd_bwd(R[pick], sd, None, standardize, torch.float32, constant_is_zero=True, grads=False)
    r64 = RR.cnn_fwd_bwd(R[pick], sd, None, standardize, torch.float64, constant_is_zero=True, grads=False)

    f = Fused(L, R, sd, E, standardize)
    gen = cnn_generic.GenericCnn(N, H, W, torch.device("cuda"), train=True)
    if chunk_rows:
        assert N % gen.chunk != 0 and gen.chunk < N, "the case is meant to end on a ragged chunk"
    Pd = dict(zip(CNN_KEYS, f.P))
    Zg = torch.full((N, X_DIM + E), SENT, device="cuda")
    gen.forward(Pd, f.R, bool(standardize), E, Zg.data_ptr() + 4 * X_DIM, X_DIM + E, True)
    sync()
    assert bool(torch.all(Zg[:, :X_DIM] == SENT))
    fails = []
    fo, go = f.out.cpu(), Zg[:, X_DIM:].cpu()
    # both implementations against the float64 reference on the sample, then against each other everywhere
    e_out = float((r32["out"].double() - r64["out"]).abs().max())
    floor = 4 * RR.ulp32(r64["out"].abs().max())
    for name, o in (("fused", fo), ("layerwise", go)):
        err = float((o[pick].double() - r64["out"]).abs().max())
        print(f"RATIO {tag} out {name} vs float64 on the sample: err {err:.3e} e_ref {e_out:.3e} k_needed {RR.needed_k(err, e_out, floor):.2f}")
    assert torch.isfinite(fo).all() and torch.isfinite(go).all()
    err = (fo.double() - go.double()).abs()
    tol = torch.minimum(torch.full_like(err, K * e_out + floor), cap_out(go.double()))
    print(f"RATIO {tag} out fused vs layerwise: err {float(err.max()):.3e} e_ref {e_out:.3e} k_needed {RR.needed_k(float(err.max()), e_out, floor):.2f}")
    if not bool((err <= tol).all()):
        fails.append(f"{tag} " + report("out fused vs layerwise", fo, go) + f"; frame {int(err.max(1).values.argmax())}")
    # gradients summed over three disjoint subsets, selected by zeroing the other rows of d_out
    for s in range(3):
        sel = (torch.arange(N) % 3 == s) if s < 2 else (torch.arange(N) % 3 == 2) & (torch.arange(N) >= N // 2)
        d_s = d_out * sel.unsqueeze(1)
        Gf = f.bwd(d_s)
        dz = torch.zeros(N, X_DIM + E, device="cuda")
        dz[:, X_DIM:] = d_s.cuda()
        Gg = {k: torch.zeros_like(p) for k, p in Pd.items()}
        gen.backward(Pd, Gg, E, dz.data_ptr() + 4 * X_DIM, X_DIM + E)
        sync()
        n_s = int(sel.sum())
        _, g32 = RR.cnn_sum_grads(R[sel], sd, d_out[sel], standardize, torch.float32, constant_is_zero=True)
        _, g64 = RR.cnn_sum_grads(R[sel], sd, d_out[sel], standardize, torch.float64, constant_is_zero=True)
        for k in CNN_KEYS:  # (the tiled set holds the px_* frames: amplified under standardize = 1)
            for path, g in (("fused", Gf[k]), ("layerwise", Gg[k])):
                check_rule(f"{tag} subset {s} ({n_s} frames)", f"{k} {path}", g, g32[k], g64[k], cap_grad, fails, amplified=bool(standardize))
            d = float((Gf[k].double() - Gg[k].cpu().double()).abs().max())
            print(f"RATIO {tag} subset {s} {k} fused vs layerwise: diff {d:.3e} of scale {float(g64[k].abs().max()):.3e}")
    flush(fails)


# ------------------------------------------------------------------------------------------------ E: the seven building blocks
def second_trip():
    """Elements above which a grid-stride kernel of csrc/roi_cnn_generic.hip takes a second trip: 64 blocks per CU, 256 threads."""
    return 64 * torch.cuda.get_device_properties(0).multi_processor_count * 256


@pytest.mark.parametrize("HW", [2, 3, 255, 256, 257, 4096, 9216])
def test_block_roi_norm(L, HW):
    """xn and stats against float64.  The bound is the float32 arithmetic of the kernel written out: r = u/255 and mu carry one
    and two roundings (2^-24 each, both below 1), the difference is divided by sd, whose three roundings and the quotient's own
    add 4 * 2^-24 |xn|: |err| <= 2^-24 (4 / sd + 8 |xn|), with a margin of one rounding on either term."""
    g = torch.Generator().manual_seed(HW)
    R = torch.randint(0, 256, (6, HW), generator=g, dtype=torch.int32).to(torch.uint8)
    R[1] = 0
    R[2] = 200
    R[3] = (torch.arange(HW) % 2 * 255).to(torch.uint8)
    R[4] = 17
    R[4, HW // 2] = 18
    N = R.shape[0]
    Rd = dev(R)
    xn = torch.full((N, HW), SENT, device="cuda")
    stats = torch.full((N, 2), SENT, device="cuda")
    L.call("ss_roi_norm", Rd.data_ptr(), N, HW, 1, xn.data_ptr(), stats.data_ptr(), L.stream())
    xn2 = torch.full((N, HW), SENT, device="cuda")
    L.call("ss_roi_norm", Rd.data_ptr(), N, HW, 1, xn2.data_ptr(), None, L.stream())
    x0 = torch.full((N, HW), SENT, device="cuda")
    st0 = torch.full((N, 2), SENT, device="cuda")
    L.call("ss_roi_norm", Rd.data_ptr(), N, HW, 0, x0.data_ptr(), st0.data_ptr(), L.stream())
    sync()
    r = R.double() / 255.0
    mu = r.mean(1, keepdim=True)
    sd = r.std(1, keepdim=True).clamp_min(1e-6)
    ref = (r - mu) / sd
    const = (R.min(1).values == R.max(1).values)
    assert bool(const[1]) and bool(const[2])
    xn, stats = xn.cpu(), stats.cpu()
    assert torch.equal(xn2.cpu(), xn), "stats = NULL must not change xn"
    assert float(xn[const].abs().max()) == 0.0, "a constant frame normalises to exactly 0"
    assert torch.equal(stats[const][:, 1], torch.full((int(const.sum()),), 1e-6)), "the std clamp"
    u = 2.0 ** -24
    live = ~const
    assert torch.isfinite(xn).all() and torch.isfinite(stats).all()
    assert bool(((xn[live].double() - ref[live]).abs() <= u * (4 / sd[live] + 8 * ref[live].abs())).all()), report("xn", xn[live], ref[live])
    assert bool(((stats[:, 0:1].double() - mu).abs() <= 4 * u * mu.abs()).all()), report("mu", stats[:, 0:1], mu)
    assert bool(((stats[live][:, 1:2].double() - sd[live]).abs() <= 4 * u * sd[live]).all()), report("sd", stats[live][:, 1:2], sd[live])
    assert torch.equal(x0.cpu(), R.float() / torch.full((N, HW), 255.0)), "standardize = 0 is float(u) / 255.0f"
    assert torch.equal(st0.cpu(), torch.tensor([0.0, 1.0]).expand(N, 2))


def _im2col_ref(src):
    N, C, H, W = src.shape
    return F.unfold(src, 3, padding=1).permute(0, 2, 1).reshape(N * H * W, 9 * C)  # unfold's rows are already c*9 + ky*3 + kx


@pytest.mark.parametrize("N,C,H,W,pad", [(2, 1, 5, 7, 3), (3, 5, 1, 6, 3), (2, 8, 2, 1, 0), (1, 16, 6, 2, 4), (2, 8, 1, 1, 1),
                                         (3, 5, 2, 2, 0), (2, 1, 64, 64, 3), (5, 16, 256, 256, 0)])
def test_block_im2col(L, N, C, H, W, pad):
    if N * C * H * W > 1 << 20:
        assert N * H * W * C > second_trip(), "this shape is here to run the grid-stride loop a second time"
    src = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C * 100 + H))
    ld = 9 * C + pad
    rows = N * H * W
    col = torch.full((rows * ld + 64,), SENT, device="cuda")
    L.call("ss_im2col3x3", dev(src).data_ptr(), N, C, H, W, col.data_ptr(), ld, L.stream())
    sync()
    got = col[: rows * ld].view(rows, ld).cpu()
    assert torch.equal(got[:, : 9 * C], _im2col_ref(src))
    if pad:
        assert float(got[:, 9 * C:].abs().max()) == 0.0, "the padding columns are zero"
    assert bool(torch.all(col[rows * ld:] == SENT)), "memory behind the last row"


def _tie_rich(shape, seed):
    """Values on a grid of 0.25 (exact ties in bulk), signed zeros included."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-3, 4, shape, generator=g).float() * 0.25
    neg0 = torch.rand(shape, generator=g) < 0.05
    y[neg0] = -0.0
    return y


@pytest.mark.parametrize("N,C,H,W", [(2, 1, 2, 2), (3, 5, 6, 2), (2, 8, 2, 10), (1, 16, 14, 6), (2, 24, 4, 4), (5, 16, 512, 512)])
def test_block_relu_pool2(L, N, C, H, W):
    if H == 512:
        assert N * C * (H // 2) * (W // 2) > second_trip()
    y = _tie_rich((N, H, W, C), H * 10 + C)  # pixel-major, as the GEMM leaves it
    y[0, :2, :2, 0] = torch.tensor([[-1.0, -0.5], [-0.5, -2.0]])  # all negative: a = 0, idx = first maximum of the raw values
    if C > 1 or N > 1:
        y[-1, :2, :2, -1] = torch.tensor([[-0.0, 0.0], [0.0, -0.0]])
    a = torch.full((N, C, H // 2, W // 2), SENT, device="cuda")
    idx = torch.full((N, C, H // 2, W // 2), 9, device="cuda", dtype=torch.uint8)
    L.call("ss_relu_pool2", dev(y).data_ptr(), N, C, H, W, a.data_ptr(), idx.data_ptr(), L.stream())
    sync()
    planar = y.permute(0, 3, 1, 2).contiguous()
    c = RR.window_classes(planar)
    want_a = F.max_pool2d(F.relu(planar), 2)
    assert torch.equal(a.cpu(), want_a)  # every value bit for bit; the sign of a zero is not part of the contract (-0.0 == 0.0 here)
    assert torch.equal(idx.cpu(), c["first"]), f"{int((idx.cpu() != c['first']).sum())} winners differ ({int(c['tied'].sum())} windows are tied)"
    if c["tied"].numel() >= 100:
        assert int(c["tied"].sum()) > 0.15 * c["tied"].numel(), "the input is meant to tie"
    assert int(idx[0, 0, 0, 0]) == 1 and float(a[0, 0, 0, 0]) == 0.0


@pytest.mark.parametrize("P", [1, 3, 144, 255, 256, 257, 1000])
@pytest.mark.parametrize("C", [24, 5])
def test_block_relu_mean(L, P, C):
    N = 3
    g = torch.Generator().manual_seed(P + C)
    y = torch.randn(N * P, C, generator=g)
    y[0, 0], y[N * P - 1, C - 1] = 0.0, -0.0
    feat = torch.full((N, C), SENT, device="cuda")
    mask = torch.full((N * P, C), 9, device="cuda", dtype=torch.uint8)
    yd = dev(y)
    L.call("ss_relu_mean", yd.data_ptr(), N, P, C, feat.data_ptr(), mask.data_ptr(), L.stream())
    feat2 = torch.full((N, C), SENT, device="cuda")
    L.call("ss_relu_mean", yd.data_ptr(), N, P, C, feat2.data_ptr(), None, L.stream())
    sync()
    assert torch.equal(mask.cpu(), (y > 0).to(torch.uint8))
    assert torch.equal(feat2, feat), "mask = NULL must not change feat"
    r32 = F.relu(y).view(N, P, C).mean(1)
    r64 = F.relu(y.double()).view(N, P, C).mean(1)
    fails = []
    check_rule(f"relu_mean P={P} C={C}", "feat", feat, r32, r64, None, fails)
    flush(fails)


@pytest.mark.parametrize("N,P,C", [(1, 1, 1), (3, 15, 24), (2, 257, 5), (200, 1000, 24)])
def test_block_mask_scale(L, N, P, C):
    if N == 200:
        assert N * P * C > second_trip()
    g = torch.Generator().manual_seed(P)
    mask = (torch.rand(N * P, C, generator=g) < 0.5).to(torch.uint8)
    mask[0, 0] = 7  # any non-zero byte is "set"
    dfeat = torch.randn(N, C, generator=g)
    dy = torch.full((N * P, C), SENT, device="cuda")
    L.call("ss_mask_scale", dev(mask).data_ptr(), dev(dfeat).data_ptr(), N, P, C, dy.data_ptr(), L.stream())
    sync()
    want = torch.where(mask.view(N, P, C) != 0, (dfeat / torch.full_like(dfeat, float(P))).unsqueeze(1).expand(N, P, C), torch.zeros(())).reshape(N * P, C)
    assert torch.equal(dy.cpu(), want)


@pytest.mark.parametrize("N,C,H2,W2", [(1, 1, 1, 1), (3, 5, 3, 1), (2, 8, 1, 5), (2, 16, 7, 3), (5, 16, 256, 256)])
def test_block_pool2_bwd(L, N, C, H2, W2):
    if H2 == 256:
        assert N * C * H2 * W2 > second_trip()
    g = torch.Generator().manual_seed(H2 + C)
    da = torch.randn(N, C, H2, W2, generator=g)
    a = torch.relu(torch.randn(N, C, H2, W2, generator=g))  # about half the pooled values are exactly 0: nothing passes
    a[0, 0, 0, 0] = 0.0
    idx = torch.randint(0, 4, (N, C, H2, W2), generator=g).to(torch.uint8)
    H, W = 2 * H2, 2 * W2
    dy = torch.full((N * H * W, C), SENT, device="cuda")
    L.call("ss_pool2_bwd", dev(da).data_ptr(), dev(a).data_ptr(), dev(idx).data_ptr(), N, C, H2, W2, dy.data_ptr(), L.stream())
    sync()
    gsel = torch.where(a > 0, da, torch.zeros(()))
    want = torch.zeros(N, C, H2, 2, W2, 2)
    for pos in range(4):
        want[:, :, :, pos // 2, :, pos % 2] = torch.where(idx == pos, gsel, torch.zeros(()))
    want = want.reshape(N, C, H, W).permute(0, 2, 3, 1).reshape(N * H * W, C)
    got = dy.cpu()
    assert not bool((got == SENT).any()), "all four positions of every window are written"
    assert torch.equal(got, want)


@pytest.mark.parametrize("N,C,H,W,pad", [(2, 1, 5, 7, 3), (3, 5, 1, 6, 0), (2, 8, 2, 1, 2), (1, 16, 6, 2, 0), (2, 8, 1, 1, 0),
                                         (2, 16, 16, 24, 0), (3, 8, 512, 512, 0)])
def test_block_col2im_and_adjoint(L, N, C, H, W, pad):
    if H == 512:
        assert N * C * H * W > second_trip()
    g = torch.Generator().manual_seed(H * 7 + C)
    ld = 9 * C + pad
    rows = N * H * W
    dcol = torch.randn(rows, ld, generator=g)
    x = torch.randn(N, C, H, W, generator=g)
    d = torch.full((N, C, H, W), SENT, device="cuda")
    dcol_d = dev(dcol)
    L.call("ss_col2im3x3", dcol_d.data_ptr(), ld, N, C, H, W, d.data_ptr(), L.stream())
    col = torch.empty(rows, ld, device="cuda")
    L.call("ss_im2col3x3", dev(x).data_ptr(), N, C, H, W, col.data_ptr(), ld, L.stream())
    sync()
    d, col = d.cpu(), col.cpu()

    def fold(t):
        return F.fold(t[:, : 9 * C].reshape(N, H * W, 9 * C).permute(0, 2, 1), (H, W), 3, padding=1)

    fails = []
    check_rule(f"col2im {N}x{C}x{H}x{W}", "d", d, fold(dcol), fold(dcol.double()), None, fails)
    flush(fails)
    # the adjoint identity <col2im(dcol), x> = <dcol, im2col(x)>, both sides accumulated in float64 from the device results; the
    # left side carries col2im's float32 roundings: at most 8 additions per output, each 2^-24 of a partial sum of |terms|
    lhs = float((d.double() * x.double()).sum())
    rhs = float((dcol[:, : 9 * C].double() * col[:, : 9 * C].double()).sum())
    budget = 8 * 2.0 ** -24 * float((dcol[:, : 9 * C].double().abs() * col[:, : 9 * C].double().abs()).sum())
    print(f"RATIO col2im adjoint {N}x{C}x{H}x{W}: lhs {lhs:.9g} rhs {rhs:.9g} diff {abs(lhs - rhs):.3e} budget {budget:.3e}")
    assert abs(lhs - rhs) <= budget
    assert math.isfinite(lhs)
