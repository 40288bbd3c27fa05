"""CPU: tests/tail_ref.py pinned -- its float32 form against oracle/model_ref.py bit for bit, its dropout against a separately
built float64 graph, its exact case, and for every shape of tests/test_gpu_tail_edges.py the conditions its tolerances rest on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as TR
import weights as W
from oracle import model_ref as MR

K_BOUND = TR.FWD + TR.CLIP + TR.SUMS


@pytest.mark.parametrize("B,T,C,Hd", [(7, 11, 5, 192), (3, 9, 7, 250)])
def test_float32_form_is_the_oracle_bit_for_bit(B, T, C, Hd):
    """MID = 128, p = 0, the golden weights and inputs of test_fused_tail_fwd_bwd: logits, loss and every gradient."""
    g = torch.Generator().manual_seed(B * 7 + T)
    sd = {k: v for k, v in W.make_state_dict(31 + B, 84, C, False, hidden=Hd).items() if k.startswith(("pool.", "head."))}
    h = torch.randn(B, T, 2 * Hd, generator=g)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    lengths[0] = T
    for b in range(B):
        h[b, lengths[b]:] = 0
    y = torch.randint(0, C, (B,), generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    hg = h.clone().requires_grad_(True)
    pooled = MR.attn_pool(hg, lengths, leaves)
    logits = MR.head(pooled, leaves)
    loss = MR.ce_label_smoothing(logits, y)
    loss.backward()
    r = TR.tail(h, lengths, sd, y, dtype=torch.float32)
    assert torch.equal(r["pooled"], pooled.detach()) and torch.equal(r["logits"], logits.detach())
    assert torch.equal(r["loss"], loss.detach()) and torch.equal(r["d_h"], hg.grad)
    for name, key in TR.GRADS.items():
        assert torch.equal(r[name].reshape(-1), leaves[key].grad.reshape(-1)), name
    # the same with a mask through the oracle's own ``dropout_mask``
    keep = torch.rand(B, 128, generator=g) >= 0.2
    r = TR.tail(h, lengths, sd, y, dtype=torch.float32, keep=keep, drop_p=0.2)
    want = MR.head(MR.attn_pool(h, lengths, sd), sd, dropout_mask=keep.float() * TR.drop_scale(0.2, torch.float32))
    assert torch.equal(r["logits"], want)
    assert r["mid"].shape == (B, 128) and bool((r["mid_d"][~keep] == 0).all())


@pytest.mark.parametrize("MID,p", [(5, 0.2), (130, 0.5)])
def test_float64_form_with_a_keep_mask_against_its_own_graph(MID, p):
    """The graph built a second time, by hand (no F.layer_norm, no F.dropout, the mask as a multiply), in float64."""
    case = TR.random_case(3, 9, 64, MID, 3, "mixed", 21)
    keep = torch.rand(3, MID, generator=torch.Generator().manual_seed(2)) >= p
    r = TR.tail(case["h"], case["lengths"], case["params"], case["y"], dtype=torch.float64, keep=keep, drop_p=p, denom=3.0)
    P = {k: v.double().clone().requires_grad_(True) for k, v in case["params"].items()}
    h = case["h"].double().clone().requires_grad_(True)
    B, T, D = h.shape
    mask = torch.arange(T).unsqueeze(0) < case["lengths"].unsqueeze(1)
    s = (h * P[TR.KEYS[0]][0]).sum(-1) + P[TR.KEYS[1]]
    e = torch.where(mask, torch.exp(s - s.masked_fill(~mask, -1e30).max(1, keepdim=True).values), torch.zeros_like(s))
    a = e / e.sum(1, keepdim=True)
    pooled = (a.unsqueeze(-1) * h).sum(1)
    mu = pooled.mean(1, keepdim=True)
    var = ((pooled - mu) ** 2).mean(1, keepdim=True)
    xhat = (pooled - mu) / torch.sqrt(var + 1e-5)
    ln = xhat * P[TR.KEYS[2]] + P[TR.KEYS[3]]
    pre = ln @ P[TR.KEYS[4]].t() + P[TR.KEYS[5]]
    mid = pre.clamp_min(0)
    mid_d = mid * keep.double() * (1.0 / (1.0 - float(np.float32(p))))
    logits = mid_d @ P[TR.KEYS[6]].t() + P[TR.KEYS[7]]
    lse = torch.logsumexp(logits, 1)
    C = logits.shape[1]
    rows = 0.95 * (lse - logits[torch.arange(B), case["y"]]) + 0.05 * (lse - logits.sum(1) / C)
    loss = rows.sum() / 3.0
    pre.retain_grad()
    logits.retain_grad()
    loss.backward()
    got = dict(attn=a, pooled=pooled, xhat=xhat, rstd=1.0 / torch.sqrt(var + 1e-5).squeeze(1), ln=ln, mid=mid, mid_d=mid_d,
               logits=logits, loss=loss, d_logits=logits.grad, d_h=h.grad, d_mid=pre.grad)
    got.update({name: P[key].grad.reshape(r[name].shape) for name, key in TR.GRADS.items()})
    for k, v in got.items():
        scale = max(float(r[k].abs().max()), 1e-30)
        assert float((v.detach() - r[k]).abs().max()) <= 1e-12 * max(scale, 1.0), k
    assert bool((r["mid_d"][~keep] == 0).all()) and bool((r["d_mid"][~keep] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_flat_row_case_is_exact(dtype):
    case = TR.special_cases()["flat"]
    r = TR.tail(case["h"], case["lengths"], case["params"], case["y"], dtype=dtype)
    assert not bool(r["xhat"].any())
    assert torch.equal(r["ln"], case["params"][TR.KEYS[3]].to(dtype).expand_as(r["ln"]))
    assert bool((r["attn"][:, 0] == 1).all()) and not bool(r["attn"][:, 1:].any())
    assert bool((r["pooled"] == 0.5).all())
    assert float((r["rstd"].double() - 1e-5 ** -0.5).abs().max()) <= 2 * TR.ulp32(1e-5 ** -0.5)


def _all_cases():
    out = {}
    for group, specs in (("sweep", TR.sweep_specs()), ("contract", TR.contract_specs()), ("drop", TR.drop_specs()),
                         ("loss", TR.loss_specs()), ("lds", TR.lds_specs())):
        out.update({f"{group}/{tag}": TR.random_case(*spec) for tag, spec in specs.items()})
    out.update({f"special/{tag}": case for tag, case in TR.special_cases().items()})
    return out


def test_every_gpu_shape_meets_the_conditions_of_its_tolerances():
    """The float32 reference is finite; e_ref > 0 for every tensor that gets a k-bound (the structural exceptions are named by
    ``exact_names`` and agree exactly or nearly: they are held to the floor alone); every logit row has a float64 gap above GAP
    between its two best, or an exact tie, so ``correct`` is compared on every row."""
    bad = []
    for tag, case in _all_cases().items():
        r32, r64 = TR.refs(tag, case)
        exact = TR.exact_names(case)
        for k in K_BOUND:
            if not bool(torch.isfinite(r32[k]).all()):
                bad.append(f"{tag} {k}: float32 reference not finite")
            e_ref = float((r32[k].double() - r64[k]).abs().max())
            if e_ref == 0.0 and k not in exact:
                bad.append(f"{tag} {k}: e_ref = 0")
        # g_bscore, exactly 0 in exact arithmetic, has a derived bound: the float32 reference's own leftover is inside it.  (Not at
        # D = 1, where d pooled is exactly 0 as well and torch's LayerNorm backward, which does not subtract the mean first,
        # leaves 1e-13 of it in float32: the kernel is held to the bound there all the same.)
        gb = TR.bscore_bound(case, r64)
        if case["h"].shape[2] > 1 and (float(r32["g_bscore"].abs().max()) > gb or (gb == 0.0 and "g_bscore" not in exact)):
            bad.append(f"{tag} g_bscore: float32 reference {float(r32['g_bscore']):.3e} against a derived bound of {gb:.3e}")
        gaps = TR.logit_gaps(r64["logits"])
        if not bool(((gaps > TR.GAP) | (gaps == 0)).all()):
            bad.append(f"{tag}: a logit gap of {float(gaps.min()):.3e}")
        if r32["correct"] != r64["correct"]:
            bad.append(f"{tag}: the two references count {r32['correct']} and {r64['correct']} hits")
    assert not bad, "\n".join(bad)


def test_tables_and_the_sharp_case():
    specs = TR.sweep_specs()
    assert len(specs) == 22 + 32 + 26 + 10 + 2
    assert all(spec[0] <= 3 for spec in specs.values())
    lds = TR.lds_specs()
    assert lds["fwd"][1] == 15221 and lds["bwd-C4"][1] == 7642 and lds["bwd-C3"][1] == 7642
    case = TR.special_cases()["sharp"]
    r32, r64 = TR.refs("special/sharp", case)
    s = F.linear(case["h"].double(), case["params"][TR.KEYS[0]].double(), case["params"][TR.KEYS[1]].double()).squeeze(-1)
    for b in range(case["h"].shape[0]):
        n = int(case["lengths"][b])
        assert abs(float(s[b, :n].max()) - 60.0) < 1e-3 and (n < 3 or float(s[b, :n].min()) < -59.0)
        assert float(r32["attn"][b].max()) == 1.0 and int((r32["attn"][b] != 0).sum()) <= 2  # one-hot; all but the runner-up underflow
    # the keep-scale the kernels use is the float32 one
    assert TR.drop_scale(0.2, torch.float32) == float(np.float32(1.0) / np.float32(0.8))
