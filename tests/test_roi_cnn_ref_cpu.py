"""CPU: tests/roi_cnn_ref.py, the per-frame float32 / float64 restatement of ROI normalise + TinyROICNN that
tests/test_gpu_roi_cnn_edges.py measures the kernels with, and the frame sets it builds.

The reference hangs on ``oracle.model_ref`` (bit-equal in float32), its per-frame gradients add up to the batched autograd
gradient, and the edge-case frames really contain what the GPU tests rely on: exact ties in bulk, resolved the same way in both
precisions, and almost no window that an argmax comparison has to leave out.
"""
import pytest
import torch

import roi_cnn_ref as RR
import weights as W
from oracle import model_ref as MR


def _sd(E, seed=21):
    sd = W.make_state_dict(seed, 84, 5, True, roi_emb=E)
    return {k: v for k, v in sd.items() if k.startswith("roi_cnn.")}


@pytest.mark.parametrize("H,W_", RR.GEOMS)
@pytest.mark.parametrize("standardize", [1, 0])
def test_float32_form_is_the_oracle_bit_for_bit(H, W_, standardize):
    sd = _sd(17)
    R, _ = RR.frame_set(H, W_, 1, 3)
    want = MR.roi_cnn(MR.roi_normalise(R.unsqueeze(0), bool(standardize)), sd)[0]
    got = RR.cnn_fwd_bwd(R, sd, None, standardize, torch.float32, grads=False)
    assert torch.equal(got["x"], MR.roi_normalise(R.unsqueeze(0), bool(standardize))[0])
    assert torch.equal(got["out"], want)
    assert sd[RR.CNN_KEYS[6]].shape[0] == 17 and want.shape == (R.shape[0], 17)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_per_frame_gradients_sum_to_the_batched_gradient(dtype):
    H, W_ = 32, 32
    sd = _sd(7)
    R, _ = RR.frame_set(H, W_, 2, 2)
    d_out = torch.randn(R.shape[0], 7, generator=torch.Generator().manual_seed(3))
    per = RR.cnn_fwd_bwd(R, sd, d_out, 1, dtype, constant_is_zero=True)
    out, tot = RR.cnn_sum_grads(R, sd, d_out, 1, dtype, constant_is_zero=True)
    assert torch.equal(per["out"], out)
    eps = 1e-5 if dtype == torch.float32 else 1e-13  # 20 addends re-associated: a few ulps of the sum's largest entry
    for k in RR.CNN_KEYS:
        s = per["grads"][k].sum(0)
        assert s.shape == tot[k].shape
        assert float((s - tot[k]).abs().max()) <= eps * max(float(tot[k].abs().max()), 1e-3), k


def test_window_classes_on_known_windows():
    y = torch.tensor([[1.0, 1.0, 0.5, 1.0],      # three-way tie: the first wins
                      [-1.0, -1.0, -1.0, -1.0],  # all negative: not positive, tied
                      [0.2, 0.7, 0.7, 0.1],      # tie of positions 1 and 2
                      [0.3, 0.30005, 0.0, 0.0],  # separated by less than GAP: left out
                      [0.0, 0.1, 0.9, 0.4]], dtype=torch.float64)
    img = y.reshape(1, 5, 2, 2)  # five channels of one 2x2 image = five windows
    c = RR.window_classes(img)
    assert c["first"].flatten().tolist() == [0, 0, 1, 1, 2]
    assert c["tied"].flatten().tolist() == [True, True, True, False, False]
    assert c["positive"].flatten().tolist() == [True, False, True, True, True]
    assert c["close"].flatten().tolist() == [False, False, False, True, False]
    keep, _ = RR.comparable(img)
    assert keep.flatten().tolist() == [True, False, True, False, True]
    # and torch's max_pool2d picks exactly ``first``
    _, idx = torch.nn.functional.max_pool2d(img, 2, return_indices=True)
    assert RR._window_pos(idx, 2).flatten().tolist() == c["first"].flatten().tolist()


@pytest.mark.parametrize("H,W_", RR.GEOMS)
@pytest.mark.parametrize("E", [17, 64])
def test_frame_sets_tie_in_bulk_and_both_precisions_agree(H, W_, E):
    """On the frame set of the GPU tests, standardize = 1: every window that is exactly tied in float64 has the same winner in
    float32 and float64 (the first maximal position); at least 30 % of the positive windows of the block frames are exactly tied,
    so a later change of the builder cannot silently empty the tie test; at most 2 % of the windows of the whole set have a
    float64 gap in (0, 1e-4] and are left out of the comparison."""
    sd = _sd(E)
    R, names = RR.frame_set(H, W_, 5, 4)
    r32 = RR.cnn_fwd_bwd(R, sd, None, 1, torch.float32, constant_is_zero=True, grads=False)
    r64 = RR.cnn_fwd_bwd(R, sd, None, 1, torch.float64, constant_is_zero=True, grads=False)
    block = torch.tensor([n in RR.BLOCK for n in names])
    pos = tied = close = total = 0
    for y, i in (("y1", "i1"), ("y2", "i2")):
        c = RR.window_classes(r64[y])
        t = c["tied"] & c["positive"]
        assert torch.equal(r64[i][t], c["first"][t]), "float64 max_pool2d does not take the first maximum"
        assert torch.equal(r32[i][t], r64[i][t]), f"{i}: float32 and float64 disagree on an exactly tied window"
        pos += int(c["positive"][block].sum())
        tied += int(t[block].sum())
        close += int((c["close"] & c["positive"]).sum())
        total += int(c["positive"].sum())
    print(f"{H}x{W_} E={E}: block frames {pos} positive windows, {tied} tied ({tied / pos:.1%}); whole set {total} positive, "
          f"{close} left out ({close / total:.2%})")
    assert tied >= 0.30 * pos, (tied, pos)
    assert close <= 0.02 * total, (close, total)


def test_frame_set_is_what_it_says():
    for H, W_ in RR.GEOMS:
        R, names = RR.frame_set(H, W_, 5, 4)
        assert R.dtype == torch.uint8 and R.shape == (22, H, W_) and names[:18] == list(RR.SPECIAL)
        f = dict(zip(names, R))
        for k in RR.CONSTANT:
            assert int(f[k].min()) == int(f[k].max())
        assert int(f["zero"].max()) == 0 and int(f["all255"].min()) == 255 and 0 < int(f["const"][0, 0]) < 255
        for k, (yy, xx) in (("px_corner", (0, 0)), ("px_edge", (0, W_ // 2)), ("px_interior", (3, 5))):
            assert int(f[k][yy, xx]) == 18 and int((f[k] != 17).sum()) == 1
        assert set(f["sat8"].flatten().tolist()) <= {0, 255} and set(f["sat8_shift"].flatten().tolist()) <= {0, 255}
        assert torch.equal(f["grey8"][:8, :8], f["grey8"][0, 0].expand(8, 8))
        assert torch.equal(f["grey8_shift"][1:9, 1:9], f["grey8_shift"][1, 1].expand(8, 8))  # the grid starts one pixel in
        assert torch.equal(f["grey4"][4:8, 4:8], f["grey4"][4, 4].expand(4, 4))
        assert torch.equal(f["ramp_v"], f["ramp_v"][:, :1].expand(H, W_)) and int(f["ramp_v"][-1, 0]) == 255
        assert torch.equal(f["ramp_h"], f["ramp_h"][:1].expand(H, W_)) and int(f["ramp_h"][0, -1]) == 255
        assert int(f["checker1"][0, 1]) == 255 and int(f["checker1"][1, 1]) == 0 and int(f["checker2"][0, 2]) == 255
        assert int((f["last_row"][:-1] != 90).sum()) == 0 and int((f["last_col"][:, :-1] != 90).sum()) == 0
        assert torch.equal(RR.frame_set(H, W_, 5, 4)[0], R), "the builder is seeded"
        assert RR.frames_n(H, W_, 1, 3).shape == (1, H, W_) and RR.frames_n(H, W_, 257, 3).shape == (257, H, W_)
        assert RR.tiled_set(H, W_, 100, 3).shape == (100, H, W_)


def test_bound_rule():
    a64 = torch.tensor([1.0, -3.0], dtype=torch.float64)
    a32 = torch.tensor([1.0, -3.0 + 2 ** -20])
    b, e, fl = RR.bound(a32, a64, 8)
    assert fl == 4 * 2.0 ** -22 and abs(e - 2 ** -20) < 1e-12 and b == 8 * e + fl  # ulp of 3.0 is 2^-22
    assert RR.needed_k(fl, e, fl) == 0.0 and abs(RR.needed_k(fl + 3 * e, e, fl) - 3.0) < 1e-9
    assert RR.bound(a64.float(), a64, 8)[0] == fl
