"""CPU: pins tests/cnn_bf16_ref.py, the float64 reference of the bf16 ROI CNN, without a GPU -- the restated layers against
torch's own convolutions and autograd, the winner rule on hand-written windows, the bf16 rounding against torch's, and the
conditions the lattice makers promise (exact f32 sums in any order, enough tied and dead windows)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_bf16_ref as CR


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def rand_bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).double()


def test_bf16_rne_is_torchs_rounding_and_ties_go_to_even():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20000, generator=g) * torch.exp2(torch.randint(-20, 20, (20000,), generator=g).float())
    assert torch.equal(CR.bf16_rne(x.double()), x.to(torch.bfloat16).view(torch.int16))
    # halfway cases, which a detour through f32 could not even represent differently: 1 + 2^-8 -> 1 (even), 1 + 3 2^-8 -> 1 + 2^-6
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -40, 0.0, 255.0, 257.0, 258.0], dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7, 0.0, 255.0, 256.0, 258.0], dtype=torch.float64)
    assert torch.equal(CR.bf16_val(t), want)
    # one rounding, not two: 1 + 2^-8 + 2^-30 is above the tie; rounded to f32 first it would BE the tie and fall to 1
    assert float(CR.bf16_val(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64))) == 1 + 2.0 ** -7


def test_winner_rule_on_hand_written_windows():
    #                 window (e = 0..3)         bias   value  byte
    cases = [([1.0, 2.0, 3.0, 4.0],             0.0,   4.0,   3),
             ([5.0, 5.0, 5.0, 5.0],             0.0,   5.0,   0),      # all tied: the first
             ([1.0, 7.0, 7.0, 2.0],             0.0,   7.0,   1),      # tie between 1 and 2: the first
             ([1.0, 2.0, 7.0, 7.0],             0.0,   7.0,   2),
             ([0.0, 0.0, 0.0, 0.0],             0.0,   0.0,   4),      # maximum exactly 0: dead
             ([0.0, 0.0, 0.0, 0.0],             0.5,   0.5,   0),      # a positive bias revives the tied window
             ([-3.0, -1.0, -2.0, -1.0],         1.0,   0.0,   4),      # max + bias == 0: dead (> is strict)
             ([-3.0, -1.0, -2.0, -1.0],         1.5,   0.5,   1),
             ([2.0, 1.0, 2.0, 0.0],            -5.0,   0.0,   4)]      # the bias kills it
    for win, bias, val, byte in cases:
        c = torch.tensor(win, dtype=torch.float64).view(1, 1, 2, 2)
        v, i = CR.pool(c, torch.tensor([bias], dtype=torch.float64))
        assert float(v) == val and int(i) == byte, (win, bias, float(v), int(i))
    dense = CR.expand_dy(torch.tensor([[[[9.0]]]], dtype=torch.float64), torch.tensor([[[[2]]]], dtype=torch.uint8))
    assert torch.equal(dense, torch.tensor([[[[0.0, 0.0], [9.0, 0.0]]]], dtype=torch.float64))
    assert float(CR.expand_dy(torch.tensor([[[[9.0]]]], dtype=torch.float64), torch.tensor([[[[4]]]], dtype=torch.uint8)).abs().sum()) == 0


@pytest.mark.parametrize("cin,cout,hw", [(1, 16, 12), (16, 32, 8), (64, 96, 12)])
def test_restated_layers_equal_torchs(cin, cout, hw):
    g = torch.Generator().manual_seed(cin)
    a, w = rand_bf16(g, 3, cin, hw, hw), rand_bf16(g, cout, cin, 3, 3, scale=0.3)
    dy = rand_bf16(g, 3, cout, hw, hw)
    assert rel(CR.conv_raw(a, w), F.conv2d(a, w, padding=1)) < 1e-12
    assert rel(CR.conv_dgrad_raw(dy, w), F.conv_transpose2d(dy, w, padding=1)) < 1e-12
    gw, gb = CR.conv_wgrad(a, dy)
    assert rel(gw, torch.nn.grad.conv2d_weight(a, w.shape, dy, padding=1)) < 1e-12
    assert rel(gb, dy.sum(dim=(0, 2, 3))) < 1e-12


def test_restated_network_equals_autograd_and_both_last_layer_forms_agree():
    """The whole chain conv1 .. conv4 + average + Linear backwards, layer by layer with the reference's routines, against float64
    autograd through a network that applies the same bf16 roundings as constants (masks and winners from the forward pass)."""
    g = torch.Generator().manual_seed(3)
    N, E = 2, 7
    R = torch.randint(0, 256, (N, 96, 96), generator=g, dtype=torch.uint8)
    ws = [rand_bf16(g, CR.C5[i + 1], CR.C5[i], 3, 3, scale=0.5 / CR.C5[i] ** 0.5) for i in range(4)]
    bs = [rand_bf16(g, CR.C5[i + 1], scale=0.1) for i in range(4)]
    wfc, dz = rand_bf16(g, E, 96), rand_bf16(g, N, E)
    xn, _, _ = CR.image_bf16(R, 1)
    # forward with the reference's routines
    acts, idxs = [xn], []
    for i in range(3):
        a, ix = CR.conv_pool_fwd(acts[-1], ws[i], bs[i])
        acts.append(a)
        idxs.append(ix)
    last = CR.last_fwd(acts[3], ws[3], bs[3], wfc, torch.zeros(E, dtype=torch.float64))
    # the same network for autograd: the roundings of the maps are straight-through constants
    wl = [w.clone().requires_grad_(True) for w in ws]
    bl = [b.clone().requires_grad_(True) for b in bs]
    h = xn
    for i in range(3):
        c = F.conv2d(h, wl[i], padding=1)
        win = CR.windows(c)
        pick = torch.gather(win, -1, idxs[i].clamp_max(3).long().unsqueeze(-1))[..., 0]     # the reference's winner
        v = torch.relu(pick + bl[i].view(1, -1, 1, 1))
        assert rel(CR.bf16_val(v.detach()), acts[i + 1]) == 0
        h = v + (acts[i + 1] - v).detach()
    x = F.conv2d(h, wl[3], padding=1) + bl[3].view(1, -1, 1, 1)
    feat = torch.relu(x).mean(dim=(2, 3))
    assert rel(feat.detach(), last["feat_div"]) < 1e-6
    ((feat @ wfc.t()) * dz).sum().backward()
    # backward with the reference's routines, WITHOUT its bf16 roundings of the gradients (autograd has none)
    df = dz @ wfc
    dy = (df / 144).view(N, 96, 1, 1) * last["mask"].double()
    for i in (3, 2, 1, 0):
        gw, gb = CR.conv_wgrad(acts[i], dy)
        assert rel(gw, wl[i].grad) < 1e-10 and rel(gb, bl[i].grad) < 1e-10, i
        if i:
            dy = CR.expand_dy(CR.conv_dgrad_raw(dy, ws[i]), idxs[i - 1])
    # the dz / wfc form and the dfeat form of the last layer are one thing
    assert torch.equal(CR.last_dy_dz(dz, wfc, last["mask"]), CR.last_dy_df(dz @ wfc, last["mask"]))
    d = CR.last_dy_df(df, last["mask"])
    assert torch.equal(d, CR.bf16_val(d)) and rel(d, (df / 144).view(N, 96, 1, 1) * last["mask"].double()) < 2.0 ** -8


def _two_orders_f32(terms):
    """f32 sums of the last axis, forwards and backwards, one addition at a time."""
    t = terms.float()
    fw, bw = torch.zeros(t.shape[:-1]), torch.zeros(t.shape[:-1])
    for k in range(t.shape[-1]):
        fw = fw + t[..., k]
        bw = bw + t[..., t.shape[-1] - 1 - k]
    return fw, bw


def _conv_terms(a, w, n, o, ys, xs):
    """The 9 CIN products of output elements (n, o, ys, xs) of conv_raw, as float64 (len(ys), 9 CIN)."""
    p = CR._pad(a)[n]
    rows = [torch.stack([p[:, y + ky, x + kx] * w[o, :, ky, kx] for ky in range(3) for kx in range(3)]).reshape(-1) for y, x in zip(ys, xs)]
    return torch.stack(rows)


def test_lattice_makers_sum_exactly_in_any_order_and_meet_their_shares():
    front = CR.make_front(4)
    assert all(v < CR.LIMIT for v in front["sums"].values())
    for tied, dead in front["shares"]:
        assert tied >= 0.20 and dead >= 0.05
    g = torch.Generator().manual_seed(1)
    ys, xs = torch.randint(0, 48, (64,), generator=g).tolist(), torch.randint(0, 48, (64,), generator=g).tolist()
    c2 = CR.conv_raw(front["a1"], front["w2"].double())
    for n, o in ((0, 5), (2, 31), (3, 2)):
        terms = _conv_terms(front["a1"], front["w2"].double(), n, o, ys, xs)
        fw, bw = _two_orders_f32(terms)
        assert torch.equal(fw, bw) and torch.equal(fw.double(), c2[n, o, ys, xs])
    for layer in (2, 3):
        m = CR.make_pooled_layer(layer, 2)
        assert m["shares"][0] >= 0.20 and m["shares"][1] >= 0.05 and m["sums"]["conv"] < CR.LIMIT
        b = CR.make_pooled_bwd(layer, 2)
        # a weight-gradient element: the products over all pixels of both frames, two orders
        hw = b["a_in"].shape[-1]
        p = CR._pad(b["a_in"])
        terms = (b["dy"][:, 3] * p[:, 1, 0:hw, 2:2 + hw]).reshape(1, -1)        # g_w[3][1][ky = 0][kx = 2]
        fw, bw = _two_orders_f32(terms)
        assert torch.equal(fw, bw) and float(fw) == float(b["g_w"][3, 1, 0, 2])
    # a random order as the float atomics would produce it
    perm = torch.randperm(terms.shape[1], generator=g)
    assert float(_two_orders_f32(terms[:, perm])[0]) == float(b["g_w"][3, 1, 0, 2])
    for dyadic in (True, False):
        m = CR.make_last(3, 7, dyadic=dyadic)
        assert all(v < CR.LIMIT for v in m["sums"].values())
        assert 0.02 < float(m["ref"]["mask"].double().mean()) < 0.98
    m = CR.make_last_bwd(3, 7)
    assert all(v < CR.LIMIT for v in m["sums"].values())
    # the front's special frames: all 0, all 255; a killed channel (every byte 4) and a weightless one with a positive bias (every byte 0)
    assert int(front["R"][1].max()) == 0 and int(front["R"][2].min()) == 255
    assert bool((front["i1"][:, 0] == 4).all()) and bool((front["i1"][:, 1] == 0).all())
    assert bool((front["i2"][:, 0] == 4).all()) and bool((front["i2"][:, 1] == 0).all())
    assert bool((front["i1"][2, 2:, 1:-1, 1:-1] % 4 == 0).all()), "inner windows of a constant frame are all tied: byte 0 or dead"


def test_gamma_bound_holds_on_random_sums():
    g = torch.Generator().manual_seed(2)
    for n in (9, 144, 576):
        t = rand_bf16(g, 4000, n) * rand_bf16(g, 4000, n)
        fw, bw = _two_orders_f32(t)
        bound = CR.gamma_bound(n, t.abs().sum(-1))
        exact = t.sum(-1)
        assert bool(((fw.double() - exact).abs() <= bound).all()) and bool(((bw.double() - exact).abs() <= bound).all())
    assert CR.gamma_bound(1, 5.0) == 0.0 and CR.gamma_bound(9, 2.0) == 8 * 2.0 ** -24 * 2.0
