"""GPU: the bf16 ROI CNN of config 5 (csrc/cnn_bf16.h, cnn_bf16.hip, cnn_bf16_bwd.hip), every ss_c5_* entry point against the
float64 reference of tests/cnn_bf16_ref.py.

EXACT LANE.  Inputs on a lattice (cnn_bf16_ref: pixels from {0, 255} under standardize = 0, activations in {0..3}, weights and
upstream gradients in {-2..2} 2^-k), on which every f32 partial sum is exact in any order: each output is compared bit for bit
with the reference rounded once -- every element, every pool byte, every mask byte, nothing left out and nothing tolerated.
The inputs are full of exactly tied and dead pool windows (asserted by the makers), so the recomputing backward kernels have to
route every tied window's gradient to the tap the forward stash names.  Frame counts are the ones at which the persistent walk
``for (n = blockIdx.x; n < N; n += gridDim.x)`` and its prefetch of frame n + gridDim.x change shape: 1, grid - 1, grid,
grid + 1, 2 grid, 2 grid + 1 under a cap of 5 workgroups, and 1 and 3 under the default grid (ss_c5_conv_dgrad, two workgroups
per CU, also under a cap of 2: grid 4, N = 3, 4, 5, 8, 9).  Weight gradients accumulate
onto a nonzero start; the ``_ws`` forms run with exactly enough scratch, one float short and none.  Every output buffer sits
between sentinels that must survive.

DERIVED-BOUND LANE (standardize = 1).  The statistics bit for bit; a bf16 output must equal the rounding of the float64 value
wherever that value is farther than cnn_bf16_ref.gamma_bound from a rounding boundary and one of the two neighbours elsewhere;
a pool byte must be the reference's wherever the window's order is decided by more than the bounds.  The share of elements
exempted from exact equality is computed on the CPU before a kernel runs and capped (1 % conv1, 5 % conv2 through the fused
kernel).  f32 gradients: gamma_bound of their own sum plus 4 f32 ulps of the largest magnitude, and never looser than the
contract of tests/test_gpu_bf16.py.  ``RATIO`` lines print error / bound.

ARGUMENT CHECKS.  Only error codes; nothing is launched."""
import functools
import math

import pytest
import torch

import cnn_bf16_ref as CR
from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

CAP = 5
GRIDS = [(CAP, 1), (CAP, 4), (CAP, 5), (CAP, 6), (CAP, 10), (CAP, 11), (0, 1), (0, 3)]
GRID_IDS = [f"cap{c}-N{n}" for c, n in GRIDS]
ALL_E = (1, 7, 63, 64)
X_OFF, LD_Z = 84, 152            # the embedding columns inside a wider row
FRONT, BACK = 64, 1024           # sentinel elements in front of / behind every output buffer
SENT = {torch.float32: 12345.0, torch.int16: 0x7fc0, torch.uint8: 0xA5}
SS_ERR_ARG, SS_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(params=GRIDS, ids=GRID_IDS)
def grid(L, request):
    """(workgroup cap, frames).  The cap is restored to 0 (all CUs) whatever the test does."""
    cap, n = request.param
    L.call("ss_roi_cnn_set_max_workgroups", cap)

    def restore():
        L.call("ss_roi_cnn_set_max_workgroups", 0)

    request.addfinalizer(restore)
    return cap, n


def wgs(cap, N, per_cu=1):
    cus = cap if cap > 0 else torch.cuda.get_device_properties(0).multi_processor_count
    return min(N, per_cu * cus)


class Bufs:
    """Device buffers of one test: inputs kept alive until the sync, outputs between sentinels."""

    def __init__(self):
        self.keep, self.outs = [], []

    def dev(self, t):
        d = t.contiguous().cuda()
        self.keep.append(d)
        return d.data_ptr()

    def out(self, name, shape, dtype, init=None, fill=None, back=BACK):
        n = math.prod(shape)
        full = torch.full((FRONT + n + back,), SENT[dtype], dtype=dtype, device="cuda")
        view = full[FRONT:FRONT + n].view(shape)
        if init is not None:
            view.copy_(init.to(dtype))
        elif fill is not None:
            view.fill_(fill)
        self.outs.append((name, full, n, back))
        return view

    def finish(self):
        torch.cuda.synchronize()
        for name, full, n, back in self.outs:
            s = torch.full((1,), SENT[full.dtype], dtype=full.dtype, device="cuda")
            assert bool((full[:FRONT] == s).all()), f"{name}: the sentinel in front of the buffer changed"
            assert bool((full[FRONT + n:] == s).all()), f"{name}: the sentinel behind the buffer changed"
        self.keep.clear()


def f32_bits(x64):
    """float64 values that must be f32-exact -> their int32 bit patterns."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "the expected value is not an f32 number"
    return x32.contiguous().view(torch.int32)


def same_f32(name, got, want64):
    g = got.detach().cpu().contiguous()
    w = f32_bits(want64.reshape(g.shape))
    if not torch.equal(g.view(torch.int32), w):
        bad = g.view(torch.int32) != w
        i = int(bad.reshape(-1).nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat {i}: got {float(g.reshape(-1)[i])!r}, "
                    f"want {float(want64.reshape(-1)[i])!r}", pytrace=False)


def same_map(name, got_nhwc, want64_nchw):
    """bf16 map from the device (N,H,W,C) int16 against float64 values rounded ONCE to bf16."""
    g = CR.from_nhwc_bits(got_nhwc)
    w = CR.bf16_rne(want64_nchw)
    if not torch.equal(g, w):
        bad = g != w
        i = int(bad.reshape(-1).nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} bf16 elements differ; first at flat (NCHW) {i}: got "
                    f"{float(CR.bf16_bits_to_f64(g.reshape(-1)[i:i + 1]))!r}, want {float(want64_nchw.reshape(-1)[i])!r}", pytrace=False)


def same_bytes(name, got_nhwc, want_nchw):
    g = CR.from_nhwc_bytes(got_nhwc)
    if not torch.equal(g, want_nchw):
        bad = g != want_nchw
        i = int(bad.reshape(-1).nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} bytes differ; first at flat (NCHW) {i}: got {int(g.reshape(-1)[i])}, "
                    f"want {int(want_nchw.reshape(-1)[i])}", pytrace=False)


# one reference per (maker, arguments) for the whole module; the tests only read them
front_of = functools.lru_cache(None)(CR.make_front)
pooled_of = functools.lru_cache(None)(CR.make_pooled_layer)
pooled_bwd_of = functools.lru_cache(None)(CR.make_pooled_bwd)
last_of = functools.lru_cache(None)(CR.make_last)
last_bwd_of = functools.lru_cache(None)(CR.make_last_bwd)


@functools.lru_cache(None)
def front_bwd_of(N):
    """The backward of the front on its own frames: conv2's weight gradient from the front's a1, conv2's data gradient, and conv1's
    weight gradient from (a) a lattice d a1, (b) conv2's data gradient -- both routed by the front's own pool bytes."""
    f = front_of(N)
    b2 = CR.make_pooled_bwd(2, N, seed=9, a_in=f["a1"], u_in=f["u1"])
    da1 = CR.lattice_grad(77, (N, 16, 48, 48), CR.KD)
    return dict(b2=b2, da1=da1, c1_lat=CR.make_conv1_bwd(f, da1, f["i1"], 2.0 ** -CR.KD),
                c1_chain=CR.make_conv1_bwd(f, b2["da_in"], f["i1"], 2.0 ** -(CR.KD + CR.K2)))


# ================================================================================================ exact lane: forward
def test_exact_front_forward(L, grid):
    """ss_c5_conv1_fwd, ss_c5_conv12_fwd, ss_c5_conv12_fwd_i1 and ss_c5_conv_fwd(2) on conv1's map, standardize = 0."""
    cap, N = grid
    f = front_of(N)
    B = Bufs()
    R, w1, b1, w2, b2 = (B.dev(f[k]) for k in ("R", "w1", "b1", "w2", "b2"))
    a1 = B.out("a1", (N, 48, 48, 16), torch.int16)
    i1 = B.out("i1", (N, 48, 48, 16), torch.uint8)
    st = B.out("st", (N, 2), torch.float32)
    L.call("ss_c5_conv1_fwd", R, N, 0, w1, b1, a1.data_ptr(), i1.data_ptr(), st.data_ptr(), L.stream())
    a2u = B.out("a2 unfused", (N, 24, 24, 32), torch.int16)
    i2u = B.out("i2 unfused", (N, 24, 24, 32), torch.uint8)
    L.call("ss_c5_conv_fwd", 2, a1.data_ptr(), N, w2, b2, a2u.data_ptr(), i2u.data_ptr(), L.stream())
    a2f = B.out("a2 fused", (N, 24, 24, 32), torch.int16)
    i2f = B.out("i2 fused", (N, 24, 24, 32), torch.uint8)
    stf = B.out("st fused", (N, 2), torch.float32)
    L.call("ss_c5_conv12_fwd", R, N, 0, w1, b1, w2, b2, a2f.data_ptr(), i2f.data_ptr(), stf.data_ptr(), L.stream())
    a2s = B.out("a2 stash", (N, 24, 24, 32), torch.int16)
    i2s = B.out("i2 stash", (N, 24, 24, 32), torch.uint8)
    sts = B.out("st stash", (N, 2), torch.float32)
    i1s = B.out("i1 stash", (N, 48, 48, 16), torch.uint8)
    L.call("ss_c5_conv12_fwd_i1", R, N, 0, w1, b1, w2, b2, a2s.data_ptr(), i2s.data_ptr(), sts.data_ptr(), i1s.data_ptr(), L.stream())
    B.finish()
    same_map("a1", a1, f["a1"])
    same_bytes("i1", i1, f["i1"])
    for name, a2, i2, s in (("unfused", a2u, i2u, st), ("fused", a2f, i2f, stf), ("stash", a2s, i2s, sts)):
        same_map(f"a2 {name}", a2, f["a2"])
        same_bytes(f"i2 {name}", i2, f["i2"])
        same_f32(f"st {name}", s, f["st"].double())
    same_bytes("i1 of the fused stash", i1s, f["i1"])
    assert torch.equal(i1s, i1) and torch.equal(a2f, a2u) and torch.equal(i2f, i2u) and torch.equal(a2s, a2u) and torch.equal(i2s, i2u)


@pytest.mark.parametrize("layer", [2, 3])
def test_exact_pooled_forward(L, grid, layer):
    cap, N = grid
    m = pooled_of(layer, N)
    cout, hw = CR.C5[layer], 96 >> layer
    B = Bufs()
    out = B.out("a_out", (N, hw, hw, cout), torch.int16)
    idx = B.out("idx", (N, hw, hw, cout), torch.uint8)
    L.call("ss_c5_conv_fwd", layer, B.dev(CR.nhwc_bits(m["a_in"])), N, B.dev(m["w"]), B.dev(m["b"]), out.data_ptr(), idx.data_ptr(), L.stream())
    B.finish()
    same_map(f"a{layer}", out, m["a_out"])
    same_bytes(f"i{layer}", idx, m["idx"])


@pytest.mark.parametrize("E", ALL_E)
def test_exact_last_forward(L, grid, E):
    """ss_c5_conv_last_fwd into columns [X_OFF, X_OFF + E) of a wider row, and ss_c5_conv_last_fwd_feat with and without the mask.
    Free signs: x, mask and the ReLU sum are exact, feat is that sum / 144 rounded once (a division in one kernel, a product
    with f32(1/144) in the other).  Dyadic inputs (cnn_bf16_ref.make_last): feat is on the lattice and z is exact as well."""
    cap, N = grid
    for dyadic in (False, True):
        m = last_of(N, E, 0, dyadic)
        ref = m["ref"]
        B = Bufs()
        a3, w, b, wfc, bfc = B.dev(CR.nhwc_bits(m["a3"])), B.dev(m["w"]), B.dev(m["b"]), B.dev(m["wfc"]), B.dev(m["bfc"])
        z = B.out("z", (N, LD_Z), torch.float32, fill=5.0)
        mask = B.out("mask", (N, 144, 96), torch.uint8)
        feat = B.out("feat", (N, 96), torch.float32)
        L.call("ss_c5_conv_last_fwd", a3, N, w, b, wfc, bfc, E, z.data_ptr() + 4 * X_OFF, LD_Z, mask.data_ptr(), feat.data_ptr(), L.stream())
        z2 = B.out("z inference", (N, E), torch.float32)
        L.call("ss_c5_conv_last_fwd", a3, N, w, b, wfc, bfc, E, z2.data_ptr(), E, None, None, L.stream())
        mask_f = B.out("mask feat", (N, 144, 96), torch.uint8)
        feat_f = B.out("feat feat", (N, 96), torch.float32)
        L.call("ss_c5_conv_last_fwd_feat", a3, N, w, b, mask_f.data_ptr(), feat_f.data_ptr(), L.stream())
        feat_n = B.out("feat no mask", (N, 96), torch.float32)
        L.call("ss_c5_conv_last_fwd_feat", a3, N, w, b, None, feat_n.data_ptr(), L.stream())
        B.finish()
        want_mask = CR.mask_to_kernel(ref["mask"])
        assert torch.equal(mask.cpu(), want_mask), f"mask (dyadic={dyadic})"
        assert torch.equal(mask_f.cpu(), want_mask), f"mask of the feature form (dyadic={dyadic})"
        same_f32("feat", feat, ref["feat_div"])
        same_f32("feat of the feature form", feat_f, ref["feat_mul"])
        same_f32("feat of the feature form, no mask", feat_n, ref["feat_mul"])
        zc = z.cpu()
        outside = torch.ones(LD_Z, dtype=torch.bool)
        outside[X_OFF:X_OFF + E] = False
        assert bool((zc[:, outside] == 5.0).all()), "columns outside [off, off + E) were written"
        assert torch.equal(zc[:, X_OFF:X_OFF + E], z2.cpu()), "z differs between the training and the inference form"
        if dyadic:
            same_f32("z", zc[:, X_OFF:X_OFF + E], ref["z"])


# ================================================================================================ exact lane: weight gradients
def run_ws_forms(L, B, cap, N, total, launch, shape_w, shape_b, start_w, start_b):
    """``launch(g_w, g_b, part_ptr, part_floats)`` three ways: scratch NULL, one float short of grid * total (both: float atomics,
    the scratch untouched) and exactly grid * total (the scratch fully written).  -> [(name, g_w, g_b, part)]."""
    need = wgs(cap, N) * total
    res = []
    for name, floats in (("part=NULL", None), ("part one short", need - 1), ("part exact", need)):
        gw = B.out(f"g_w {name}", shape_w, torch.float32, init=start_w)
        gb = B.out(f"g_b {name}", shape_b, torch.float32, init=start_b)
        part = None if floats is None else B.out(f"part {name}", (floats,), torch.float32, fill=float("nan"), back=64)
        launch(gw.data_ptr(), gb.data_ptr(), None if part is None else part.data_ptr(), 0 if part is None else floats)
        res.append((name, gw, gb, part))
    return res


def check_ws_forms(res, want_w, want_b):
    for name, gw, gb, part in res:
        same_f32(f"g_w {name}", gw, want_w)
        same_f32(f"g_b {name}", gb, want_b)
        if name == "part one short":
            assert bool(torch.isnan(part).all()), "scratch that is one float short was written"
        if name == "part exact":  # every workgroup leaves all its sums there: the scratch path was taken, with the grid the test expects
            assert not bool(torch.isnan(part).any()), "scratch of exactly grid * total floats was not (fully) written: the atomics path ran"


@pytest.mark.parametrize("layer", [2, 3])
def test_exact_pooled_wgrad(L, grid, layer):
    """ss_c5_conv_wgrad and ss_c5_conv_wgrad_ws: start + sum over the frames, exactly."""
    cap, N = grid
    m = pooled_bwd_of(layer, N)
    cin, cout = CR.C5[layer - 1], CR.C5[layer]
    sw, sb = CR.lattice_start(layer, (cout, cin, 3, 3), m["u_w"]), CR.lattice_start(layer + 10, (cout,), m["u_b"])
    B = Bufs()
    a, da, idx = B.dev(CR.nhwc_bits(m["a_in"])), B.dev(CR.nhwc_bits(m["da"])), B.dev(CR.nhwc_bytes(m["idx"]))
    gw = B.out("g_w", (cout, cin, 3, 3), torch.float32, init=sw)
    gb = B.out("g_b", (cout,), torch.float32, init=sb)
    L.call("ss_c5_conv_wgrad", layer, a, da, idx, N, gw.data_ptr(), gb.data_ptr(), L.stream())
    res = run_ws_forms(L, B, cap, N, cout * cin * 9,
                       lambda w_, b_, p_, n_: L.call("ss_c5_conv_wgrad_ws", layer, a, da, idx, N, w_, b_, p_, n_, L.stream()),
                       (cout, cin, 3, 3), (cout,), sw, sb)
    B.finish()
    same_f32("g_w", gw, sw + m["g_w"])
    same_f32("g_b", gb, sb + m["g_b"])
    check_ws_forms(res, sw + m["g_w"], sb + m["g_b"])


def test_exact_conv2_wgrad_recomputed(L, grid):
    """ss_c5_conv2_wgrad_rc and _rc_ws, standardize = 0: conv1's map is rebuilt from the frame, tied windows and all."""
    cap, N = grid
    f, fb = front_of(N), front_bwd_of(N)
    m = fb["b2"]
    sw, sb = CR.lattice_start(21, (32, 16, 3, 3), m["u_w"]), CR.lattice_start(22, (32,), m["u_b"])
    B = Bufs()
    R, st, w1, b1 = B.dev(f["R"]), B.dev(f["st"]), B.dev(f["w1"]), B.dev(f["b1"])
    da, idx = B.dev(CR.nhwc_bits(m["da"])), B.dev(CR.nhwc_bytes(m["idx"]))
    gw = B.out("g_w", (32, 16, 3, 3), torch.float32, init=sw)
    gb = B.out("g_b", (32,), torch.float32, init=sb)
    L.call("ss_c5_conv2_wgrad_rc", R, st, 0, w1, b1, da, idx, N, gw.data_ptr(), gb.data_ptr(), L.stream())
    res = run_ws_forms(L, B, cap, N, 32 * 16 * 9,
                       lambda w_, b_, p_, n_: L.call("ss_c5_conv2_wgrad_rc_ws", R, st, 0, w1, b1, da, idx, N, w_, b_, p_, n_, L.stream()),
                       (32, 16, 3, 3), (32,), sw, sb)
    B.finish()
    same_f32("g_w2", gw, sw + m["g_w"])
    same_f32("g_b2", gb, sb + m["g_b"])
    check_ws_forms(res, sw + m["g_w"], sb + m["g_b"])


def test_exact_conv1_wgrad_all_forms(L, grid):
    """conv1's weight gradient, standardize = 0, on frames whose pool windows are mostly tied or dead: the stored-winner form, the
    recomputing form (i1 = NULL), and the kernel fused with conv2's data gradient -- recomputing, with and without the d a1 map,
    and with the stashed bytes.  A recomputing kernel that breaks a tie differently from the forward kernels moves g_w1 between
    taps and fails here."""
    cap, N = grid
    f, fb = front_of(N), front_bwd_of(N)
    u_lat, u_ch = fb["c1_lat"]["unit"], fb["c1_chain"]["unit"]
    B = Bufs()
    R, st, w1, b1, w2 = B.dev(f["R"]), B.dev(f["st"]), B.dev(f["w1"]), B.dev(f["b1"]), B.dev(fb["b2"]["w"])
    i1 = B.dev(CR.nhwc_bytes(f["i1"]))
    da1 = B.dev(CR.nhwc_bits(fb["da1"]))
    da2, i2 = B.dev(CR.nhwc_bits(fb["b2"]["da"])), B.dev(CR.nhwc_bytes(fb["b2"]["idx"]))
    outs = {}

    def acc(name, unit, seed):
        sw, sb = CR.lattice_start(seed, (16, 1, 3, 3), unit), CR.lattice_start(seed + 1, (16,), unit)
        outs[name] = (B.out(f"g_w1 {name}", (16, 1, 3, 3), torch.float32, init=sw), B.out(f"g_b1 {name}", (16,), torch.float32, init=sb), sw, sb)
        return outs[name][0].data_ptr(), outs[name][1].data_ptr()

    L.call("ss_c5_conv1_wgrad", R, N, 0, st, da1, i1, None, None, *acc("stored", u_lat, 31), L.stream())
    L.call("ss_c5_conv1_wgrad", R, N, 0, st, da1, None, w1, b1, *acc("recomputed", u_lat, 33), L.stream())
    da1_map = B.out("d a1", (N, 48, 48, 16), torch.int16)
    L.call("ss_c5_conv2_dgrad_conv1_wgrad", da2, i2, N, w2, R, st, 0, w1, b1, da1_map.data_ptr(), *acc("fused+map", u_ch, 35), L.stream())
    L.call("ss_c5_conv2_dgrad_conv1_wgrad", da2, i2, N, w2, R, st, 0, w1, b1, None, *acc("fused", u_ch, 37), L.stream())
    L.call("ss_c5_conv2_dgrad_conv1_wgrad_i1", da2, i2, N, w2, R, st, 0, w1, b1, None, *acc("fused+i1", u_ch, 39), i1, L.stream())
    B.finish()
    same_map("d a1 of the fused kernel", da1_map, fb["b2"]["da_in"])
    for name, (gw, gb, sw, sb) in outs.items():
        ref = fb["c1_lat"] if name in ("stored", "recomputed") else fb["c1_chain"]
        same_f32(f"g_w1 {name}", gw, sw + ref["g_w"])
        same_f32(f"g_b1 {name}", gb, sb + ref["g_b"])


@pytest.mark.parametrize("E", ALL_E)
def test_exact_last_backward(L, grid, E):
    """ss_c5_conv_last_wgrad / _dgrad (d z at a column offset of a wider row) and the _df forms (d z . W_fc ready-made)."""
    cap, N = grid
    m = last_bwd_of(N, E)
    u = m["unit"]
    sw, sb = CR.lattice_start(41, (96, 64, 3, 3), u), CR.lattice_start(42, (96,), u)
    swfc, sbfc = CR.lattice_start(43, (E, 96), 2.0 ** -5), CR.lattice_start(44, (E,), 0.25)
    dz_row = torch.full((N, LD_Z), 1e30)        # whatever surrounds the E columns must not be read into the sums
    dz_row[:, X_OFF:X_OFF + E] = m["dz"]
    B = Bufs()
    a3, wfc, feat, w, df = B.dev(CR.nhwc_bits(m["a3"])), B.dev(m["wfc"]), B.dev(m["feat"]), B.dev(m["w"]), B.dev(m["df"])
    mk = B.dev(CR.mask_to_kernel(m["mask"]))
    dz = B.dev(dz_row) + 4 * X_OFF
    gw = B.out("g_w4", (96, 64, 3, 3), torch.float32, init=sw)
    gb = B.out("g_b4", (96,), torch.float32, init=sb)
    gwfc = B.out("g_wfc", (E, 96), torch.float32, init=swfc)
    gbfc = B.out("g_bfc", (E,), torch.float32, init=sbfc)
    L.call("ss_c5_conv_last_wgrad", a3, dz, LD_Z, E, wfc, mk, feat, N, gw.data_ptr(), gb.data_ptr(), gwfc.data_ptr(), gbfc.data_ptr(), L.stream())
    din = B.out("d a3", (N, 12, 12, 64), torch.int16)
    L.call("ss_c5_conv_last_dgrad", dz, LD_Z, E, wfc, mk, N, w, din.data_ptr(), L.stream())
    din_df = B.out("d a3 df", (N, 12, 12, 64), torch.int16)
    L.call("ss_c5_conv_last_dgrad_df", df, mk, N, w, din_df.data_ptr(), L.stream())
    res = run_ws_forms(L, B, cap, N, 96 * 64 * 9,
                       lambda w_, b_, p_, n_: L.call("ss_c5_conv_last_wgrad_df", a3, df, mk, N, w_, b_, p_, n_, L.stream()),
                       (96, 64, 3, 3), (96,), sw, sb)
    B.finish()
    same_f32("g_w4", gw, sw + m["g_w"])
    same_f32("g_b4", gb, sb + m["g_b"])
    same_f32("g_wfc", gwfc, swfc + m["g_wfc"])
    same_f32("g_bfc", gbfc, sbfc + m["g_bfc"])
    same_map("d a3", din, m["da3"])
    same_map("d a3 (df form)", din_df, m["da3"])
    check_ws_forms(res, sw + m["g_w"], sb + m["g_b"])


# ================================================================================================ exact lane: data gradients
DGRAD_CAP = 2
DGRAD_GRIDS = [(DGRAD_CAP, n) for n in (3, 4, 5, 8, 9)]


@pytest.fixture(params=DGRAD_GRIDS, ids=[f"cap{c}-N{n}" for c, n in DGRAD_GRIDS])
def grid_dgrad(L, request):
    """ss_c5_conv_dgrad holds two workgroups per CU, so under the cap of 5 its grid is min(N, 10) and no workgroup walks a third
    frame.  Cap 2 makes its grid 4: N = grid - 1, grid, grid + 1, 2 grid, 2 grid + 1 (a workgroup then walks three frames)."""
    cap, n = request.param
    L.call("ss_roi_cnn_set_max_workgroups", cap)
    request.addfinalizer(lambda: L.call("ss_roi_cnn_set_max_workgroups", 0))
    return cap, n


@pytest.mark.parametrize("layer", [2, 3])
def test_exact_pooled_dgrad_own_grid(L, grid_dgrad, layer):
    _pooled_dgrad(L, grid_dgrad, layer)


@pytest.mark.parametrize("layer", [2, 3])
def test_exact_pooled_dgrad(L, grid, layer):
    """ss_c5_conv_dgrad: the unmasked bf16 map (two workgroups per CU: under the cap of 5 the grid is min(N, 10))."""
    _pooled_dgrad(L, grid, layer)


def _pooled_dgrad(L, grid, layer):
    cap, N = grid
    m = pooled_bwd_of(layer, N)
    cin, hw = CR.C5[layer - 1], 96 >> (layer - 1)
    B = Bufs()
    din = B.out("da_in", (N, hw, hw, cin), torch.int16)
    L.call("ss_c5_conv_dgrad", layer, B.dev(CR.nhwc_bits(m["da"])), B.dev(CR.nhwc_bytes(m["idx"])), N, B.dev(m["w"]), din.data_ptr(), L.stream())
    B.finish()
    same_map(f"d a{layer - 1}", din, m["da_in"])


# ================================================================================================ arguments the ABI refuses
def test_refused_arguments_launch_nothing(L):
    """Error codes of the argument checks.  Every output stays as it was: nothing ran."""
    lib = L.load()
    N = 1
    B = Bufs()
    z16 = lambda *s: B.dev(torch.zeros(*s, dtype=torch.int16))
    z8 = lambda *s: B.dev(torch.zeros(*s, dtype=torch.uint8))
    zf = lambda *s: B.dev(torch.zeros(*s))
    gw = B.out("g_w", (96 * 64 * 9 + 4,), torch.float32, fill=1.0)
    gb = B.out("g_b", (96,), torch.float32, fill=1.0)
    part = B.out("part", (96 * 64 * 9 + 4,), torch.float32, fill=2.0)
    din = B.out("din", (N, 12, 12, 64), torch.int16, fill=3)
    s = L.stream()
    for layer, cin, cout, hw in ((2, 16, 32, 48), (3, 32, 64, 24)):
        a, da, ix = z16(N, hw, hw, cin), z16(N, hw // 2, hw // 2, cout), z8(N, hw // 2, hw // 2, cout)
        n_part = cout * cin * 9
        assert lib.ss_c5_conv_wgrad_ws(layer, a, da, ix, N, gw.data_ptr(), gb.data_ptr(), part.data_ptr() + 4, n_part, s) == SS_ERR_ARG
        assert lib.ss_c5_conv_wgrad_ws(layer, a, da, ix, N, gw.data_ptr() + 4, gb.data_ptr(), part.data_ptr(), n_part, s) == SS_ERR_ARG
        assert lib.ss_c5_conv_wgrad(layer, a, da, ix, N, gw.data_ptr() + 8, gb.data_ptr(), s) == SS_ERR_ARG
    R, st, w1, b1 = z8(N, 96, 96), zf(N, 2), zf(16, 9), zf(16)
    da2, i2 = z16(N, 24, 24, 32), z8(N, 24, 24, 32)
    assert lib.ss_c5_conv2_wgrad_rc_ws(R, st, 0, w1, b1, da2, i2, N, gw.data_ptr(), gb.data_ptr(), part.data_ptr() + 4, 32 * 16 * 9, s) == SS_ERR_ARG
    assert lib.ss_c5_conv2_wgrad_rc_ws(R, st, 0, w1, b1, da2, i2, N, gw.data_ptr() + 4, gb.data_ptr(), part.data_ptr(), 32 * 16 * 9, s) == SS_ERR_ARG
    a3, df, mk = z16(N, 12, 12, 64), zf(N, 96), z8(N, 144, 96)
    assert lib.ss_c5_conv_last_wgrad_df(a3, df, mk, N, gw.data_ptr(), gb.data_ptr(), part.data_ptr() + 4, 96 * 64 * 9, s) == SS_ERR_ARG
    assert lib.ss_c5_conv_last_wgrad_df(a3, df, mk, N, gw.data_ptr() + 4, gb.data_ptr(), part.data_ptr(), 96 * 64 * 9, s) == SS_ERR_ARG
    dz, wfc, feat, w4 = zf(N, 80), zf(80, 96), zf(N, 96), zf(96, 64, 9)
    gwfc, gbfc = B.out("g_wfc", (80, 96), torch.float32, fill=1.0), B.out("g_bfc", (80,), torch.float32, fill=1.0)
    for E in (0, 65):
        assert lib.ss_c5_conv_last_wgrad(a3, dz, 80, E, wfc, mk, feat, N, gw.data_ptr(), gb.data_ptr(), gwfc.data_ptr(), gbfc.data_ptr(),
                                         s) == SS_ERR_UNSUPPORTED
        assert lib.ss_c5_conv_last_dgrad(dz, 80, E, wfc, mk, N, w4, din.data_ptr(), s) == SS_ERR_UNSUPPORTED
    da1 = z16(N, 48, 48, 16)
    assert lib.ss_c5_conv1_wgrad(R, N, 0, st, da1, None, None, None, gw.data_ptr(), gb.data_ptr(), s) == SS_ERR_ARG
    assert lib.ss_c5_conv1_wgrad(R, N, 0, st, da1, None, w1, None, gw.data_ptr(), gb.data_ptr(), s) == SS_ERR_ARG
    assert lib.ss_c5_conv1_wgrad(R, N, 0, st, da1, None, None, b1, gw.data_ptr(), gb.data_ptr(), s) == SS_ERR_ARG
    B.finish()
    assert bool((gw == 1.0).all()) and bool((gb == 1.0).all()) and bool((part == 2.0).all()) and bool((din == 3).all())
    assert bool((gwfc == 1.0).all()) and bool((gbfc == 1.0).all())


# ================================================================================================ derived-bound lane
CAP_CONV1, CAP_CONV2 = 0.01, 0.05     # largest share of elements exempted from exact equality


def std_frames(N, seed):
    g = torch.Generator().manual_seed(seed)
    R = torch.randint(0, 256, (N, 96, 96), generator=g, dtype=torch.uint8)
    R[1] = 7                      # constant frame: the std clamp, every normalised pixel exactly 0
    R[2] = 200
    R[2, 5, 9] = 201              # near-constant frame
    return R


def pooled_interval(c, c_abs, b, n_terms, extra=None):
    """Exact raw sums c (float64), sum |terms| c_abs, bias -> what an f32 kernel may deliver.  B_e = gamma_bound(n_terms + 1,
    c_abs_e + |b|) (+ ``extra``) bounds every raw sum and the bias addition; the pooled value of the kernel lies within the largest
    B_e of its window of the exact one (max and ReLU are 1-Lipschitz).  -> (val, byte, lo bits, hi bits, exempt, byte_sure)."""
    babs = b.double().abs().view(1, -1, 1, 1)
    Be = CR.gamma_bound(n_terms + 1, c_abs + babs)
    if extra is not None:
        Be = Be + extra
    val, byte = CR.pool(c, b.double())
    Bw = CR.windows(Be).max(-1).values
    top0 = CR.windows(c).max(-1).values + b.double().view(1, -1, 1, 1)
    hi_v = torch.where(top0 < -Bw, torch.zeros_like(val), val + Bw)        # below zero by more than the bound: 0 for certain
    lo, hi = CR.bf16_rne(torch.clamp_min(val - Bw, 0.0)), CR.bf16_rne(hi_v)
    exempt = lo != hi
    win, bwin = CR.windows(c), CR.windows(Be)
    top = win.max(-1, keepdim=True).values
    first = (win == top).double().argmax(-1, keepdim=True)
    btop = torch.gather(bwin, -1, first)
    others = torch.ones_like(win, dtype=torch.bool).scatter_(-1, first, False)
    decided = ((top - win > btop + bwin) | ~others).all(-1)               # every other position loses by more than the two bounds
    pre = top[..., 0] + b.double().view(1, -1, 1, 1)
    byte_sure = (pre < -Bw) | ((pre > Bw) & decided)                       # dead for certain, or alive with a certain winner
    return val, byte, lo, hi, exempt, byte_sure, Bw


def bf16_steps(lo, hi):
    """bf16 numbers from lo to hi (bit patterns, lo <= hi as values): 0 equal, 1 neighbours."""
    key = lambda b: torch.where(b >= 0, b.int(), -(b.int() & 0x7fff))
    return key(hi) - key(lo)


CAP_WIDE = 0.001  # share of elements whose interval holds more than two bf16 numbers (conv2 behind an exempt a1 element)


def check_interval(name, got_nhwc, lo, hi, exempt, cap_wide=CAP_WIDE):
    """Equal to the rounded reference outside the bound's reach, one of the two neighbours inside it.  Where the interval holds more
    than two bf16 numbers (the bound carries the spread of an input map) the kernel must still lie inside; that share is computed
    from the reference alone, printed and capped at CAP_WIDE, a fiftieth of conv2's cap on exempt elements (``cap_wide`` = None: printed
    only -- a signed gradient map whose sums cancel to near zero, where a bf16 step is smaller than any bound)."""
    wide = float((bf16_steps(lo, hi) > 1).double().mean())
    assert cap_wide is None or wide <= cap_wide, f"{name}: {wide:.5f} of the intervals hold more than two bf16 numbers: change the inputs"
    g = CR.bf16_bits_to_f64(CR.from_nhwc_bits(got_nhwc))
    lo64, hi64 = CR.bf16_bits_to_f64(lo), CR.bf16_bits_to_f64(hi)
    exact_ok = g[~exempt] == lo64[~exempt]
    assert bool(exact_ok.all()), f"{name}: {int((~exact_ok).sum())} elements outside the bound's reach differ from the rounded reference"
    assert bool(((g >= lo64) & (g <= hi64)).all()), f"{name}: an exempted element is not one of the two neighbours"
    moved = float((g != lo64).double().mean())
    print(f"RATIO {name}: exempt {float(exempt.double().mean()):.5f} of the elements, {moved:.5f} sit on the upper neighbour, wide {wide:.6f}")


def test_bound_front_forward_standardized(L, grid):
    """ss_c5_conv1_fwd, ss_c5_conv12_fwd and ss_c5_conv12_fwd_i1 with standardize = 1 on random, constant and near-constant frames."""
    cap, N = grid
    g = torch.Generator().manual_seed(5)
    R = std_frames(max(N, 3), 50)[:N]
    w1 = (torch.randn(16, 1, 3, 3, generator=g) * 0.4).to(torch.bfloat16).float()
    b1 = torch.randn(16, generator=g) * 0.2
    # conv2's weights lean positive: with zero-mean weights the sums cancel (sum |terms| ~ 16 |sum|), gamma_bound(145) then reaches a
    # rounding boundary at 7 % of the elements (computed on the CPU) -- over the cap, so the inputs changed, not the cap: ~1 % now
    w2 = ((torch.randn(32, 16, 3, 3, generator=g) + 0.5) / 12.0).to(torch.bfloat16).float()
    b2 = torch.randn(32, generator=g) * 0.1
    xn, mu, sd = CR.image_bf16(R, 1)
    c1, c1a = CR.conv_raw(xn, w1.double()), CR.conv_raw(xn.abs(), w1.double().abs())
    v1, i1, lo1, hi1, ex1, sure1, _ = pooled_interval(c1, c1a, b1, 9)
    share1 = float(ex1.double().mean())
    assert share1 <= CAP_CONV1, f"conv1: {share1:.4f} of the elements are exempt: change the inputs, not the cap"
    a1 = CR.bf16_val(v1)
    lo1v, hi1v = CR.bf16_bits_to_f64(lo1), CR.bf16_bits_to_f64(hi1)
    spread = torch.maximum(hi1v - a1, a1 - lo1v)                            # how far the kernel's a1 may sit from the reference's
    c2, c2a = CR.conv_raw(a1, w2.double()), CR.conv_raw(hi1v, w2.double().abs())
    v2, i2, lo2, hi2, ex2, sure2, _ = pooled_interval(c2, c2a, b2, 144, extra=CR.conv_raw(spread, w2.double().abs()))
    share2 = float(ex2.double().mean())
    assert share2 <= CAP_CONV2, f"conv2: {share2:.4f} of the elements are exempt: change the inputs, not the cap"
    B = Bufs()
    Rd, w1d, b1d, w2d, b2d = B.dev(R), B.dev(w1), B.dev(b1), B.dev(w2), B.dev(b2)
    a1k = B.out("a1", (N, 48, 48, 16), torch.int16)
    i1k = B.out("i1", (N, 48, 48, 16), torch.uint8)
    st = B.out("st", (N, 2), torch.float32)
    L.call("ss_c5_conv1_fwd", Rd, N, 1, w1d, b1d, a1k.data_ptr(), i1k.data_ptr(), st.data_ptr(), L.stream())
    a2k = B.out("a2", (N, 24, 24, 32), torch.int16)
    i2k = B.out("i2", (N, 24, 24, 32), torch.uint8)
    st2 = B.out("st fused", (N, 2), torch.float32)
    L.call("ss_c5_conv12_fwd", Rd, N, 1, w1d, b1d, w2d, b2d, a2k.data_ptr(), i2k.data_ptr(), st2.data_ptr(), L.stream())
    a2s = B.out("a2 stash", (N, 24, 24, 32), torch.int16)
    i2s = B.out("i2 stash", (N, 24, 24, 32), torch.uint8)
    i1s = B.out("i1 stash", (N, 48, 48, 16), torch.uint8)
    st3 = B.out("st stash", (N, 2), torch.float32)
    L.call("ss_c5_conv12_fwd_i1", Rd, N, 1, w1d, b1d, w2d, b2d, a2s.data_ptr(), i2s.data_ptr(), st3.data_ptr(), i1s.data_ptr(), L.stream())
    B.finish()
    want_st = torch.stack([mu, sd], 1).double()
    for s_ in (st, st2, st3):
        same_f32("st", s_, want_st)
    check_interval(f"N={N} cap={cap} a1", a1k, lo1, hi1, ex1)
    check_interval(f"N={N} cap={cap} a2", a2k, lo2, hi2, ex2)
    for name, got, want, sure in (("i1", i1k, i1, sure1), ("i1 stash", i1s, i1, sure1), ("i2", i2k, i2, sure2)):
        gb_ = CR.from_nhwc_bytes(got)
        assert torch.equal(gb_[sure], want[sure]), f"{name}: a pool byte differs where the bounds decide the window"
        print(f"RATIO N={N} cap={cap} {name}: decided {float(sure.double().mean()):.5f} of the windows")
    assert torch.equal(a2s, a2k) and torch.equal(i2s, i2k), "the stashing form computes another a2 / i2"
    if N > 1:  # the constant frame: conv output exactly 0 -> ReLU(bias), bit for bit
        assert torch.equal(CR.from_nhwc_bits(a1k)[1], CR.bf16_rne(torch.relu(b1).double()).view(16, 1, 1).expand(16, 48, 48))


def grad_bound(n_terms, sum_abs, ref):
    return CR.gamma_bound(n_terms, sum_abs) + 4 * 2.0 ** -23 * 2.0 ** math.floor(math.log2(max(float(ref.abs().max()), 1e-30)))


def check_grad(name, got, ref, bound, older, extra=None):
    """|got - ref| <= bound elementwise, the bound never looser than ``older`` (the contract of tests/test_gpu_bf16.py); ``extra``:
    what the older test does not face at all (the spread of a recomputed input map, the mass of undecided windows) comes on top."""
    tol = torch.minimum(bound, torch.full_like(bound, older))
    if extra is not None:
        tol = tol + extra
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / tol).max())
    print(f"RATIO {name}: max err {float(err.max()):.3e}, err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: error {float(err.max()):.3e} exceeds the derived bound (ratio {ratio:.2f})"


def value_interval(ref, bound):
    """A bf16 map whose f32 sums lie within ``bound`` of ``ref``: -> (lo bits, hi bits, exempt, spread = the farthest the kernel's
    value may sit from the rounded reference)."""
    lo, hi = CR.bf16_rne(ref - bound), CR.bf16_rne(ref + bound)
    r = CR.bf16_val(ref)
    return lo, hi, lo != hi, torch.maximum(CR.bf16_bits_to_f64(hi) - r, r - CR.bf16_bits_to_f64(lo))


def tap_windows(xn):
    """[ky][kx] -> (N,1,48,48,4): the pixel that tap (ky, kx) meets from each of the four positions of a pool window."""
    p = CR._pad(xn)
    return [[CR.windows(p[:, :, ky:ky + 96, kx:kx + 96]) for kx in range(3)] for ky in range(3)]


def test_bound_conv1_and_conv2_weight_gradients_standardized(L, grid):
    """f32 gradients under standardize = 1, every form.

    Stored winners / random bytes (ss_c5_conv1_wgrad with i1, ss_c5_conv2_wgrad_rc and _rc_ws): the only freedom is the summation
    order (and, for conv2, the spread of the recomputed a1): gamma_bound + 4 ulps (+ that spread), never looser than the contract of
    tests/test_gpu_bf16.py.

    Recomputed winners (ss_c5_conv1_wgrad with i1 = NULL, ss_c5_conv2_dgrad_conv1_wgrad with and without the d a1 map): the
    reference routes d a1 by its own bytes.  Where pooled_interval decides a window (byte_sure) the kernel has to route alike, and
    that part of the sum is held as above.  A window the bounds do not decide may go to another of its four positions or die:
    another position moves g_w1[c][tap] by at most |d a1| D(window, tap), D = the largest difference between two pixels the tap meets
    from the window's CONTENDERS, the positions whose sum is within the bounds of the largest (nothing on a constant patch, whoever
    wins); life or death undecided moves it by at most |d a1| M(window, tap),
    M = the largest |pixel| met, and g_b1[c] by |d a1|.  Those masses, summed from the reference alone, are added to the bound
    (tests/test_gpu_bf16.py leaves such windows out altogether).  In the fused kernels d a1 is itself a bf16 map of f32 sums: it is
    checked as an interval, and its spread times |pixel| is added too.  ss_c5_conv2_dgrad_conv1_wgrad_i1 gets the reference's
    bytes: no undecided mass."""
    cap, N = grid
    g = torch.Generator().manual_seed(6)
    R = std_frames(max(N, 3), 60)[:N]
    w1 = (torch.randn(16, 1, 3, 3, generator=g) * 0.4).to(torch.bfloat16).float()
    b1 = torch.randn(16, generator=g) * 0.2
    xn, mu, sd = CR.image_bf16(R, 1)
    st = torch.stack([mu, sd], 1).contiguous()
    da1 = torch.randn(N, 16, 48, 48, generator=g).to(torch.bfloat16).double()
    i1 = CR.lattice_bytes(61, (N, 16, 48, 48))
    dy1 = CR.expand_dy(da1, i1)
    gw_ref, gb_ref = CR.conv_wgrad(xn, dy1)
    gw_abs, gb_abs = CR.conv_wgrad(xn.abs(), dy1.abs())
    n1 = N * 48 * 48
    # conv2's weight gradient from the recomputed a1
    c1, c1a = CR.conv_raw(xn, w1.double()), CR.conv_raw(xn.abs(), w1.double().abs())
    v1, i1_ref, lo1, hi1, ex1, sure1, Bw1 = pooled_interval(c1, c1a, b1, 9)
    a1 = CR.bf16_val(v1)
    lo1v, hi1v = CR.bf16_bits_to_f64(lo1), CR.bf16_bits_to_f64(hi1)
    spread = torch.maximum(hi1v - a1, a1 - lo1v)
    da2 = torch.randn(N, 32, 24, 24, generator=g).to(torch.bfloat16).double()
    i2 = CR.lattice_bytes(62, (N, 32, 24, 24))
    dy2 = CR.expand_dy(da2, i2)
    g2_ref, gb2_ref = CR.conv_wgrad(a1, dy2)
    g2_abs, gb2_abs = CR.conv_wgrad(hi1v, dy2.abs())
    g2_spread, _ = CR.conv_wgrad(spread, dy2.abs())
    n2 = N * 24 * 24
    # recomputed winners: the undecided windows' masses
    taps = tap_windows(xn)
    cwin, bwin = CR.windows(c1), CR.windows(CR.gamma_bound(10, c1a + b1.double().abs().view(1, -1, 1, 1)))
    contender = cwin + bwin >= (cwin - bwin).max(-1, keepdim=True).values    # (N,16,48,48,4)
    pre1 = CR.windows(c1).max(-1).values + b1.double().view(1, -1, 1, 1)
    life_open = pre1.abs() <= Bw1

    def open_mass(da):
        mw = torch.zeros(16, 1, 3, 3, dtype=torch.float64)
        inf = torch.tensor(float("inf"), dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                w = taps[ky][kx]
                D = torch.where(contender, w, -inf).max(-1).values - torch.where(contender, w, inf).min(-1).values
                mw[:, 0, ky, kx] = (da.abs() * ((~sure1).double() * D + life_open.double() * w.abs().max(-1).values)).sum(dim=(0, 2, 3))
        return mw, (da.abs() * life_open.double()).sum(dim=(0, 2, 3))

    rc_ref_w, rc_ref_b = CR.conv_wgrad(xn, CR.expand_dy(da1, i1_ref))
    rc_abs_w, rc_abs_b = CR.conv_wgrad(xn.abs(), CR.expand_dy(da1.abs(), i1_ref))
    rc_open_w, rc_open_b = open_mass(da1)
    # the fused kernels: d a1 = bf16(conv_transpose(dy2, w2)), unmasked, then routed by conv1's winners
    w2 = (torch.randn(32, 16, 3, 3, generator=g) / 12.0).to(torch.bfloat16).float()
    d_raw = CR.conv_dgrad_raw(dy2, w2.double())
    d_lo, d_hi, d_ex, d_spread = value_interval(d_raw, CR.gamma_bound(288, CR.conv_dgrad_raw(dy2.abs(), w2.double().abs())))
    d1 = CR.bf16_val(d_raw)
    fu_ref_w, fu_ref_b = CR.conv_wgrad(xn, CR.expand_dy(d1, i1_ref))
    fu_abs_w, fu_abs_b = CR.conv_wgrad(xn.abs(), CR.expand_dy(d1.abs() + d_spread, i1_ref))
    fu_spr_w, fu_spr_b = CR.conv_wgrad(xn.abs(), CR.expand_dy(d_spread, i1_ref))
    fu_open_w, fu_open_b = open_mass(d1.abs() + d_spread)
    B = Bufs()
    Rd, std_, w1d, b1d, w2d = B.dev(R), B.dev(st), B.dev(w1), B.dev(b1), B.dev(w2)
    da1d, da2d, i2d, i1refd = B.dev(CR.nhwc_bits(da1)), B.dev(CR.nhwc_bits(da2)), B.dev(CR.nhwc_bytes(i2)), B.dev(CR.nhwc_bytes(i1_ref))
    outs = {}

    def acc(name, shape_w, shape_b):
        outs[name] = (B.out(f"g_w {name}", shape_w, torch.float32, fill=0.0), B.out(f"g_b {name}", shape_b, torch.float32, fill=0.0))
        return outs[name][0].data_ptr(), outs[name][1].data_ptr()

    s1, s2 = ((16, 1, 3, 3), (16,)), ((32, 16, 3, 3), (32,))
    L.call("ss_c5_conv1_wgrad", Rd, N, 1, std_, da1d, B.dev(CR.nhwc_bytes(i1)), None, None, *acc("stored", *s1), L.stream())
    L.call("ss_c5_conv2_wgrad_rc", Rd, std_, 1, w1d, b1d, da2d, i2d, N, *acc("rc", *s2), L.stream())
    need = wgs(cap, N) * 32 * 16 * 9
    part = B.out("part", (need,), torch.float32, fill=float("nan"), back=64)
    L.call("ss_c5_conv2_wgrad_rc_ws", Rd, std_, 1, w1d, b1d, da2d, i2d, N, *acc("rc_ws", *s2), part.data_ptr(), need, L.stream())
    L.call("ss_c5_conv1_wgrad", Rd, N, 1, std_, da1d, None, w1d, b1d, *acc("recomputed", *s1), L.stream())
    d_map = B.out("d a1", (N, 48, 48, 16), torch.int16)
    L.call("ss_c5_conv2_dgrad_conv1_wgrad", da2d, i2d, N, w2d, Rd, std_, 1, w1d, b1d, d_map.data_ptr(), *acc("fused+map", *s1), L.stream())
    L.call("ss_c5_conv2_dgrad_conv1_wgrad", da2d, i2d, N, w2d, Rd, std_, 1, w1d, b1d, None, *acc("fused", *s1), L.stream())
    L.call("ss_c5_conv2_dgrad_conv1_wgrad_i1", da2d, i2d, N, w2d, Rd, std_, 1, w1d, b1d, None, *acc("fused+i1", *s1), i1refd, L.stream())
    B.finish()
    tag = f"N={N} cap={cap}"
    print(f"RATIO {tag}: undecided conv1 windows {float((~sure1).double().mean()):.5f}, life undecided {float(life_open.double().mean()):.5f}")
    check_grad(f"{tag} g_w1", outs["stored"][0], gw_ref, grad_bound(n1, gw_abs, gw_ref), 2e-4 * float(gw_ref.abs().max()))
    check_grad(f"{tag} g_b1", outs["stored"][1], gb_ref, grad_bound(n1, gb_abs, gb_ref), 2e-4 * float(gb_ref.abs().max()))
    for k in ("rc", "rc_ws"):
        check_grad(f"{tag} g_w2 {k}", outs[k][0], g2_ref, grad_bound(n2, g2_abs, g2_ref), 1e-3 * float(g2_ref.abs().max()), extra=g2_spread)
        check_grad(f"{tag} g_b2 {k}", outs[k][1], gb2_ref, grad_bound(n2, gb2_abs, gb2_ref), 2e-4 * float(gb2_ref.abs().max()))
    assert not bool(torch.isnan(part).any()), "the scratch of ss_c5_conv2_wgrad_rc_ws was not taken"
    check_grad(f"{tag} g_w1 recomputed", outs["recomputed"][0], rc_ref_w, grad_bound(n1, rc_abs_w, rc_ref_w), 3e-4 * float(rc_ref_w.abs().max()),
               extra=rc_open_w)
    check_grad(f"{tag} g_b1 recomputed", outs["recomputed"][1], rc_ref_b, grad_bound(n1, rc_abs_b, rc_ref_b), 3e-4 * float(rc_ref_b.abs().max()),
               extra=rc_open_b)
    check_interval(f"{tag} d a1 of the fused kernel", d_map, d_lo, d_hi, d_ex, cap_wide=None)
    for k, ow, ob in (("fused+map", fu_open_w, fu_open_b), ("fused", fu_open_w, fu_open_b), ("fused+i1", 0.0, 0.0)):
        check_grad(f"{tag} g_w1 {k}", outs[k][0], fu_ref_w, grad_bound(n1, fu_abs_w, fu_ref_w), 3e-4 * float(fu_ref_w.abs().max()),
                   extra=fu_spr_w + ow)
        check_grad(f"{tag} g_b1 {k}", outs[k][1], fu_ref_b, grad_bound(n1, fu_abs_b, fu_ref_b), 3e-4 * float(fu_ref_b.abs().max()),
                   extra=fu_spr_b + ob)
