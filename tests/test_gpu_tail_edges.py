"""GPU: the fused classifier tail (csrc/tail.hip: ss_tail_fwd -> ss_tail_bwd, one 1024-thread workgroup per clip each way) at the
edges of its widths, lengths, head and classes, against the float64 reference of tests/tail_ref.py.

Every case runs the forward with its stash, the inference form, and the backward twice: with float atomics on the three D-vectors
and with per-clip ``col_part`` rows summed by ss_colsum_f32.  Ragged cases run a second time with NaN behind every clip's length
(nothing may change by a bit); every output buffer has 256 sentinel floats behind it.

Tolerances are multiples of the reference's own error (``roi_cnn_ref.bound``): a tensor lies within ``k * e_ref + floor`` of the
float64 value, e_ref = max |float32 reference - float64 reference| on the same inputs, floor = 4 float32 ulps of the tensor's
largest magnitude.  Where the two references agree exactly for a structural reason (``tail_ref.exact_names``) k is 0.  The values
of k (K_FWD, K_CLIP, K_SUM; K_LONG for the two shapes at the LDS limit) and the ratios observed on the MI355X are in
docs/LAB_NOTES.md section 16.  g_bscore, which is 0 in exact arithmetic, has a
derived bound (``tail_ref.bscore_bound``).  At the five shapes of test_fused_tail_fwd_bwd the numbers of tests/test_gpu_kernels.py
stay upper bounds: the smaller tolerance applies at every element.  Integer and structural results (``correct``, keep patterns,
zeros, sentinels, bit-equalities) are exact.  Every figure is printed before it is asserted (``-s``: lines starting with ``RATIO``).
"""
import numpy as np
import pytest
import torch

import distill_ref as DR
import flat_ref as FR
import tail_ref as TR
from gpu_support import L, STASH, bits, cuda, make_weights, tail_call  # noqa: F401
from tail_ref import KEYS

pytestmark = pytest.mark.gpu

K_FWD = 16    # docs/LAB_NOTES.md section 16: twice the largest observed ratio (6.51, logits at T = 2049), rounded up to a power of two
K_CLIP = 4    # d_h, d_mid: 2 x 1.58 (d_h at D = 2, MID = 130)
K_SUM = 16    # g_gamma, g_beta, g_wscore, dW1, dW4: 2 x 7.15 (g_wscore of the sharp case; 7.06: dW1 at T = 2049)
K_LONG = (64, K_CLIP, 64)  # the LDS-limit shapes, T = 7 642 and 15 221: the pooled row is ONE serial chain of T additions per thread,
                           # its rounding grows with T where the reference's blocked sum does not: 2 x 31.4 (logits), 2 x 20.7 (dW1)
SENT = -7.0
SLACK = 256   # sentinel floats behind every output buffer
U = 2.0 ** -24
SS_ERR_ARG, SS_ERR_UNSUPPORTED = -1, -3
EPS = float(np.float32(0.05))
NO_DROP = (0.0, 0, 0)
DROP = (5, (7 << 40) + 12345)  # seed, and an offset whose low and high words are both non-zero


class Buf:
    """A device tensor of ``shape`` filled with SENT (``zero``: with 0) and SLACK more sentinels behind it."""

    def __init__(self, shape, zero=False, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + SLACK,), SENT, device="cuda", dtype=dtype)
        if zero:
            self.flat[:self.n] = 0
        self.t = self.flat[:self.n].view(shape)
        self.zero = zero

    @property
    def ptr(self):
        return self.flat.data_ptr()

    def intact(self):
        return bool((self.flat[self.n:] == SENT).all())

    def untouched(self):
        return self.intact() and bool((self.t == (0 if self.zero else SENT)).all())


def dims_of(case):
    B, T, D = case["h"].shape
    return B, T, D, case["params"][KEYS[4]].shape[0], case["params"][KEYS[7]].shape[0]


def clip_of(case, b):
    """Clip b alone, as a B = 1 case."""
    return dict(h=case["h"][b:b + 1].clone(), lengths=case["lengths"][b:b + 1], y=case["y"][b:b + 1], params=case["params"])


class Tail:
    """The device copy of a case and the two launches on fresh sentinel-guarded buffers."""

    def __init__(self, L, case, nan_pad=False):
        self.L, self.dims = L, dims_of(case)
        h = case["h"].clone()
        if nan_pad:
            for b in range(h.shape[0]):
                h[b, int(case["lengths"][b]):] = float("nan")
        self.h, self.len, self.y = cuda(h), cuda(case["lengths"].to(torch.int32)), cuda(case["y"])
        self.P = {k: cuda(case["params"][k]) for k in KEYS}

    def fwd(self, drop=NO_DROP, infer=False, denom=None, dims=None, d_logits=True):
        B, T, D, MID, C = self.dims
        o = dict(attn=Buf((B, T)), xhat=Buf((B, D)), rstd=Buf((B,)), ln=Buf((B, D)), mid=Buf((B, MID)), mid_d=Buf((B, MID)),
                 logits=Buf((B, C)), d_logits=Buf((B, C)), loss=Buf((1,), zero=True), correct=Buf((1,), zero=True, dtype=torch.int32))
        ptr = lambda k: None if infer or (k == "d_logits" and not d_logits) else o[k].ptr  # noqa: E731
        st = self.L.load().ss_tail_fwd(self.h.data_ptr(), self.len.data_ptr(), *(self.P[k].data_ptr() for k in KEYS),
                                       None if infer else self.y.data_ptr(), *(dims or self.dims), 1e-5, *drop, EPS,
                                       float(B if denom is None else denom), *(ptr(k) for k in STASH), o["logits"].ptr, ptr("d_logits"),
                                       ptr("loss"), ptr("correct"), self.L.stream())
        torch.cuda.synchronize()
        return st, o

    def bwd(self, o, drop=NO_DROP, col=False):
        B, T, D, MID, C = self.dims
        P = self.P
        g = dict(d_mid=Buf((B, MID)), d_h=Buf((B, T, D)), g_gamma=Buf((D,), zero=True), g_beta=Buf((D,), zero=True),
                 g_wscore=Buf((D,), zero=True), g_bscore=Buf((1,), zero=True))
        if col:
            g["col_part"] = Buf((B, 3, D))
        st = self.L.load().ss_tail_bwd(self.h.data_ptr(), self.len.data_ptr(), P[KEYS[0]].data_ptr(), P[KEYS[2]].data_ptr(),
                                       P[KEYS[4]].data_ptr(), P[KEYS[6]].data_ptr(), o["attn"].ptr, o["xhat"].ptr, o["rstd"].ptr,
                                       o["mid"].ptr, o["d_logits"].ptr, B, T, D, MID, C, *drop, g["d_mid"].ptr, g["d_h"].ptr,
                                       g["g_gamma"].ptr, g["g_beta"].ptr, g["g_wscore"].ptr, g["g_bscore"].ptr,
                                       g["col_part"].ptr if col else None, self.L.stream())
        if col and st == 0:
            for k, name in enumerate(("g_gamma", "g_beta", "g_wscore")):
                self.L.call("ss_colsum_f32", g["col_part"].ptr + 4 * k * D, B, D, 3 * D, g[name].ptr, self.L.stream())
        torch.cuda.synchronize()
        return st, g


def check(tag, name, got, r32, r64, k, fails, exact, cap=None):
    """|got - float64| <= k * e_ref + floor at every element (k = 0 where e_ref is 0, which only a tensor of ``exact`` may have),
    and never looser than ``cap``.  Prints the k the tensor would have needed; collects failures so that a case reports them all."""
    ref64, ref32 = r64[name].double().reshape(-1), r32[name].double().reshape(-1)
    g = got.detach().double().cpu().reshape(-1)
    assert g.shape == ref64.shape, (tag, name, g.shape, ref64.shape)
    b, e_ref, floor = TR.bound(ref32, ref64, k)
    assert e_ref > 0 or name in exact, f"{tag} {name}: e_ref = 0 on a tensor that is not structurally exact"
    tol = torch.full_like(ref64, b)
    if cap is not None:
        tol = torch.minimum(tol, cap(ref64))
    err = float((g - ref64).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
    need = TR.needed_k(err, e_ref, floor)
    print(f"RATIO {tag} {name}: err {err:.3e} e_ref {e_ref:.3e} floor {floor:.3e} k_needed {need:.2f}")
    if not bool(((g - ref64).abs() <= tol).all()):  # (NaN compares false)
        i = int((g - ref64).abs().argmax())
        fails.append(f"{tag} {name}: err {err:.3e} at flat {i} (got {float(g[i]):.7g}, ref {float(ref64[i]):.7g}); bound {b:.3e} = "
                     f"{k} * {e_ref:.3e} + {floor:.3e}, k needed {need:.1f}" + ("; capped by the older contract" if cap else ""))
    return need


def flush(fails):
    if fails:
        pytest.fail(f"{len(fails)} checks failed:\n" + "\n".join(fails[:40]), pytrace=False)


def same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


def launches(L, case, drop, nan_pad, backward):
    """Forward, inference form, and both backward forms of a case -> (outputs by name, every Buf).  Statuses are asserted."""
    t = Tail(L, case, nan_pad)
    st, o = t.fwd(drop)
    assert st == 0, st
    st, inf = t.fwd(drop, infer=True)
    assert st == 0, st
    assert same_bits(inf["logits"].t, o["logits"].t), "the inference form's logits"
    assert all(inf[k].untouched() for k in inf if k != "logits"), "the inference form wrote to a buffer it was not given"
    out = {k: v.t for k, v in o.items()}
    bufs = list(o.values()) + [inf["logits"]]
    if backward:
        st, a = t.bwd(o, drop)
        assert st == 0, st
        st, c = t.bwd(o, drop, col=True)
        assert st == 0, st
        assert same_bits(a["d_h"].t, c["d_h"].t) and same_bits(a["d_mid"].t, c["d_mid"].t), "the two backward forms"
        out.update({k: v.t for k, v in a.items()})
        out.update({k + "/col": v.t for k, v in c.items()})
        bufs += list(a.values()) + list(c.values())
    return out, bufs


def run_case(L, tag, case, fails, ks=None, caps=None, drop=NO_DROP, keep=None, backward=True):
    """Everything the module docstring promises for one case; -> the outputs by name."""
    k_fwd, k_clip, k_sum = ks or (K_FWD, K_CLIP, K_SUM)
    caps = caps or {}
    r32, r64 = TR.refs(tag, case, keep, drop[0])
    exact = TR.exact_names(case)
    B, T, D, MID, C = dims_of(case)
    lengths = [int(n) for n in case["lengths"]]
    out, bufs = launches(L, case, drop, False, backward)
    det = [k for k in out if k.split("/")[0] not in ("loss", "g_gamma", "g_beta", "g_wscore", "g_bscore") or k.endswith("/col")]
    assert all(bool(torch.isfinite(out[k].float()).all()) for k in out), [k for k in out if not bool(torch.isfinite(out[k].float()).all())]
    if min(lengths) < T:  # NaN behind every clip's length: not a bit may move (sums of B atomics: any order, so to (B - 1) u)
        out2, bufs2 = launches(L, case, drop, True, backward)
        bufs += bufs2
        for k in det:
            if not same_bits(out[k], out2[k]):
                fails.append(f"{tag} {k}: changes with what lies behind the clips' lengths (max diff {float((out[k] - out2[k]).abs().max())})")
        for k in set(out) - set(det):  # sums of B float atomics, in any order: each is within (B - 1) u of the magnitudes added
            # of the exact sum, so two of them are within twice that of each other
            if k == "g_bscore":
                continue  # (held to its derived bound in both runs)
            mag = out["loss"].abs() if k == "loss" else out["col_part/col"][:, ("g_gamma", "g_beta", "g_wscore").index(k)].abs().sum(0)
            if not bool(((out[k] - out2[k]).abs() <= 2 * (B - 1) * U * mag).all()):
                fails.append(f"{tag} {k}: changes with what lies behind the clips' lengths")
    if not all(b.intact() for b in bufs):
        fails.append(f"{tag}: a sentinel behind an output buffer was overwritten")
    # ---- structure
    for b, n in enumerate(lengths):
        if bool(out["attn"][b, n:].any()):
            fails.append(f"{tag}: attn[{b}, {n}:] is not exactly 0")
        if n == 1 and float(out["attn"][b, 0]) != 1.0:
            fails.append(f"{tag}: attn[{b}, 0] = {float(out['attn'][b, 0])!r} for a clip of length 1")
        if backward and bool(out["d_h"][b, n:].any()):
            fails.append(f"{tag}: d_h[{b}, {n}:] is not exactly 0")
    if drop[0] == 0.0 and not same_bits(out["mid"], out["mid_d"]):
        fails.append(f"{tag}: mid_d differs from mid without dropout")
    if int(out["correct"]) != r64["correct"]:
        fails.append(f"{tag}: correct {int(out['correct'])}, reference {r64['correct']}")
    # ---- values
    for name in TR.FWD:
        check(tag, name, out[name], r32, r64, k_fwd, fails, exact, caps.get(name))
    if backward:
        for name in TR.CLIP:
            check(tag, name, out[name], r32, r64, k_clip, fails, exact, caps.get(name))
        stash = {k: out[k].double().cpu() for k in ("d_mid", "ln", "d_logits", "mid_d")}
        got = {"dW1": stash["d_mid"].t() @ stash["ln"], "dW4": stash["d_logits"].t() @ stash["mid_d"]}  # the GEMMs over the stash
        gb = TR.bscore_bound(case, r64)
        for form in ("", "/col"):
            got.update({k: out[k + form] for k in ("g_gamma", "g_beta", "g_wscore")})
            for name in TR.SUMS if form == "" else TR.SUMS[:3]:
                check(tag + (" col_part" if form else ""), name, got[name], r32, r64, k_sum, fails, exact, caps.get(name))
            err = abs(float(out["g_bscore" + form]))
            print(f"RATIO {tag} g_bscore{form}: |value| {err:.3e} derived bound {gb:.3e} fraction {err / gb if gb else 0.0:.3f}")
            if not err <= gb:
                fails.append(f"{tag} g_bscore{form}: {err:.3e}, which is 0 in exact arithmetic, above the derived bound {gb:.3e}")
    return out


# ------------------------------------------------------------------------------------------------ one-axis sweeps and corners
SWEEP = TR.sweep_specs()


@pytest.mark.parametrize("tag", list(SWEEP))
def test_sweep(L, tag):
    fails = []
    run_case(L, "sweep/" + tag, TR.random_case(*SWEEP[tag]), fails)
    flush(fails)


# ------------------------------------------------------------------------------------------------ the older contract's shapes
def contract_caps(Hd):
    rel = lambda a, r: (lambda ref: a * max(float(ref.abs().max()), 0.0) + 1e-8 * (r == "g") + 1e-4 * ref.abs())  # noqa: E731
    return dict(logits=lambda ref: (3e-6 if Hd == 192 else 1e-5) + 1e-5 * ref.abs(),
                loss=lambda ref: torch.full_like(ref, 3e-6 * max(1.0, float(ref.abs().max()))),
                d_h=rel(2e-5, "h"), g_gamma=rel(2e-5, "g"), g_beta=rel(2e-5, "g"), g_wscore=rel(2e-5, "g"), dW1=rel(2e-5, "w"),
                dW4=rel(2e-5, "w"))


CONTRACT = TR.contract_specs()


@pytest.mark.parametrize("tag", list(CONTRACT))
def test_contract_shapes_keep_the_older_bounds(L, tag):
    """The five shapes of test_fused_tail_fwd_bwd against float64: k * e_ref + floor, and its hand-set numbers as upper bounds."""
    fails = []
    run_case(L, "contract/" + tag, TR.random_case(*CONTRACT[tag]), fails, caps=contract_caps(CONTRACT[tag][2] // 2))
    flush(fails)


# ------------------------------------------------------------------------------------------------ numerical edges
SPECIAL = TR.special_cases()


def test_sharp_scores(L):
    """Scores spread over +-60: a softmax that is one-hot to float32, exponentials that underflow."""
    fails = []
    out = run_case(L, "special/sharp", SPECIAL["sharp"], fails)
    assert float(out["attn"].max()) == 1.0
    flush(fails)


def test_flat_row(L):
    """A clip whose only frame is the constant 0.5: xhat is exactly 0, ln exactly beta, rstd 1 / sqrt(eps) to 2 ulp."""
    fails = []
    case = SPECIAL["flat"]
    out = run_case(L, "special/flat", case, fails)
    beta = cuda(case["params"][KEYS[3]])
    assert not bool(bits(out["xhat"].cpu().numpy()).any()), "xhat is not +0.0 everywhere"
    assert all(same_bits(out["ln"][b], beta) for b in range(out["ln"].shape[0]))
    want = 1.0 / np.sqrt(float(np.float32(1e-5)))
    assert float((out["rstd"].double().cpu() - want).abs().max()) <= 2 * TR.ulp32(want)
    flush(fails)


def test_all_clips_of_length_one(L):
    fails = []
    run_case(L, "special/all-length-1", SPECIAL["all-length-1"], fails)
    flush(fails)


# ------------------------------------------------------------------------------------------------ dropout
DROPS = TR.drop_specs()


@pytest.mark.parametrize("MID", TR.DROP_MIDS)
@pytest.mark.parametrize("p", TR.DROP_PS)
def test_dropout_both_directions(L, p, MID):
    """Forward: the keep pattern of the host Philox, values to its 2 ulp.  Backward, twice on identical inputs: d_mid(p) is +0.0
    where the host drops or mid <= 0 and elsewhere the bits of float32(d_mid(0) * float32(1 / (1 - p))).  Then the whole forward
    and backward against float64 with that mask."""
    case = TR.random_case(*DROPS[f"MID{MID}"])
    B = case["h"].shape[0]
    drop = (p,) + DROP
    t = Tail(L, case)
    st, o = t.fwd(drop)
    assert st == 0
    mid, mid_d = o["mid"].t.cpu().numpy().reshape(-1), o["mid_d"].t.cpu().numpy().reshape(-1)
    keep, want, bnd = FR.dropout_expected(mid, B * MID, p, *DROP)
    assert 0 < int(keep.sum()) < keep.size
    assert not bits(mid_d)[~keep].any(), "a dropped element of mid_d is not +0.0"
    assert np.array_equal(mid_d != 0, keep & (mid > 0)), "the keep pattern of mid_d"
    assert bool((np.abs(mid_d.astype(np.float64) - want) <= bnd).all())
    (st0, g0), (stp, gp) = t.bwd(o, NO_DROP), t.bwd(o, drop)
    assert st0 == 0 and stp == 0
    d0, dp = g0["d_mid"].t.cpu().numpy().reshape(-1), gp["d_mid"].t.cpu().numpy().reshape(-1)
    zero = ~keep | (mid <= 0)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    print(f"p={p} MID={MID}: {int(keep.sum())}/{keep.size} kept, {int(zero.sum())} zero in d_mid, "
          f"{int((bits(dp)[zero] != 0).sum())} of them not +0.0")
    assert not bits(dp)[zero].any(), "d_mid is not +0.0 where the host drops or mid <= 0"
    assert np.array_equal(bits(dp)[~zero], bits((d0 * scale).astype(np.float32))[~zero]), "d_mid(p) != d_mid(0) * float32(1 / (1 - p))"
    fails = []
    run_case(L, f"drop/p{p}-MID{MID}", case, fails, drop=drop, keep=torch.from_numpy(keep.reshape(B, MID).copy()))
    flush(fails)


def test_dropout_rows_are_independent(L):
    """Clip b of a B = 3 launch is, bit for bit, a B = 1 launch on that clip with offset + b * MID / 4."""
    case = TR.random_case(*DROPS["MID128"])
    B, T, D, MID, C = dims_of(case)
    p, (seed, offset) = 0.2, DROP
    t = Tail(L, case)
    st, o = t.fwd((p, seed, offset))
    st2, g = t.bwd(o, (p, seed, offset), col=True)
    assert st == 0 and st2 == 0
    for b in range(B):
        drop = (p, seed, offset + b * MID // 4)
        t1 = Tail(L, clip_of(case, b))
        # (the length of clip b is below T for b > 0: the B = 1 launch keeps the padded T)
        st, o1 = t1.fwd(drop, denom=B)
        st2, g1 = t1.bwd(o1, drop, col=True)
        assert st == 0 and st2 == 0
        for k in STASH + ("logits", "d_logits"):
            assert same_bits(o1[k].t[0], o[k].t[b]), (b, k)
        for k in ("d_mid", "d_h", "col_part"):
            assert same_bits(g1[k].t[0], g[k].t[b]), (b, k)


# ------------------------------------------------------------------------------------------------ the loss forms at the lane edges
LOSS = TR.loss_specs()


def loss_check(tag, out, ref, fails):
    e_loss = abs(float(out["loss"]) - ref["loss"]) / ref["loss_bound"]
    d = out["d_logits"].double().cpu().numpy()
    counts = ref["grad_bound"].max(1) > 0  # (a row that does not count has a zero bound: it must be exactly zero)
    assert ref["grad_bound"][counts].min() > 0 and not d[~counts].any() and not ref["grad"][~counts].any()
    e_grad = float((np.abs(d - ref["grad"])[counts] / ref["grad_bound"][counts]).max())
    print(f"RATIO loss/{tag}: loss err / bound {e_loss:.3f}, d_logits err / bound {e_grad:.3f}")
    if not (e_loss <= 1.0 and e_grad <= 1.0 and int(out["correct"]) == ref["correct"]):
        fails.append(f"loss/{tag}: loss err / bound {e_loss:.3f}, d_logits err / bound {e_grad:.3f}, correct {int(out['correct'])} "
                     f"(reference {ref['correct']})")


@pytest.mark.parametrize("C", TR.LOSS_C)
def test_loss_forms_past_one_trip_of_the_lane_loop(L, C):
    """ss_tail_fwd_w, _mix (without and with weights) and _kd, with dropout on: the stash and logits are ss_tail_fwd's bits; loss,
    d_logits and correct against tests/distill_ref.py on the kernel's own logits within its derived bound.  Row 1 of the weighted
    and mix forms carries a label outside the classes: a zero gradient row that adds nothing."""
    case = TR.random_case(*LOSS[f"C{C}"])
    dims = dims_of(case)
    B = dims[0]
    g = torch.Generator().manual_seed(40 + C)
    w = make_weights(g, C)
    y = case["y"]
    y_out = y.clone()
    y_out[1] = C
    y_b = torch.randint(0, C, (B,), generator=g)
    teacher = torch.randn(B, C, generator=g) * 3
    lam = 0.3125
    den = float(w[y_out[y_out < C]].sum())
    t = Tail(L, case)
    P, h_d, len_d = t.P, t.h, t.len
    y_d, yo_d, yb_d, w_d, t_d = cuda(y), cuda(y_out), cuda(y_b), cuda(w), cuda(teacher)
    den_d, lam_d = torch.tensor([den], device="cuda"), torch.tensor([lam], device="cuda")
    drop = (0.2,) + DROP
    plain = tail_call(L, "ss_tail_fwd", P, h_d, len_d, y_d, dims, EPS, (float(B),), drop=drop)
    assert not same_bits(plain["mid"], plain["mid_d"])
    z = plain["logits"].double().cpu().numpy()
    mix = (yb_d.data_ptr(), lam_d.data_ptr())
    forms = {
        "w": ("ss_tail_fwd_w", yo_d, (w_d.data_ptr(), den_d.data_ptr()), (), (), dict(y=y_out, w=w, den=den)),
        "mix": ("ss_tail_fwd_mix", yo_d, (float(B), None, None), mix, (), dict(y=y_out, y_b=y_b, lam=lam)),
        "mix_w": ("ss_tail_fwd_mix", yo_d, (1.0, w_d.data_ptr(), den_d.data_ptr()), mix, (), dict(y=y_out, y_b=y_b, lam=lam, w=w, den=den)),
        "kd": ("ss_tail_fwd_kd", y_d, (float(B), None, None), (None, None), (t_d.data_ptr(), C, 0.25, 2.0), dict(y=y, alpha=0.25, tau=2.0)),
    }
    fails = []
    for form, (name, lab_d, norm, labels, soft, kw) in forms.items():
        out = tail_call(L, name, P, h_d, len_d, lab_d, dims, EPS, norm, labels, soft, drop=drop)
        for k in STASH + ("logits",):
            assert same_bits(out[k], plain[k]), (form, k)
        ref = DR.evaluate(z, teacher.numpy() if form == "kd" else z, kw["y"].numpy(), kw.get("tau", 1.0), kw.get("alpha", 0.0), EPS,
                          float(B), None if "w" not in kw else kw["w"].numpy(), kw.get("den"),
                          None if "y_b" not in kw else kw["y_b"].numpy(), kw.get("lam", 1.0))
        loss_check(f"C{C}-{form}", out, ref, fails)
        if form != "kd":
            assert not bool(out["d_logits"][1].any()) and not ref["grad"][1].any(), form
    flush(fails)


# ------------------------------------------------------------------------------------------------ the 60 KiB LDS conditions
LDS = TR.lds_specs()


def longer(spec):
    return spec[:1] + (spec[1] + 1,) + spec[2:]


def test_lds_limit_forward(L):
    """T + 2 D + MID + C = 15 360 floats: runs and matches; one more frame: SS_ERR_UNSUPPORTED, nothing written."""
    fails = []
    run_case(L, "lds/fwd", TR.random_case(*LDS["fwd"]), fails, ks=K_LONG, backward=False)
    flush(fails)
    st, o = Tail(L, TR.random_case(*longer(LDS["fwd"]))).fwd()
    assert st == SS_ERR_UNSUPPORTED and all(b.untouched() for b in o.values())


@pytest.mark.parametrize("which", ["bwd-C4", "bwd-C3"])
def test_lds_limit_backward(L, which):
    """MID + D + 2 T + C = 15 360 floats (C = 4; with C = 3 the sum is odd: 15 359): runs and matches; one more frame is 15 362
    (15 361): the forward still runs, the backward returns SS_ERR_UNSUPPORTED and writes nothing."""
    fails = []
    run_case(L, "lds/" + which, TR.random_case(*LDS[which]), fails, ks=K_LONG)
    flush(fails)
    t = Tail(L, TR.random_case(*longer(LDS[which])))
    st, o = t.fwd()
    assert st == 0
    for col in (False, True):
        st, g = t.bwd(o, col=col)
        assert st == SS_ERR_UNSUPPORTED and all(b.untouched() for b in g.values())


def test_argument_checks(L):
    case = TR.random_case(2, 5, 64, 8, 3, "full", 15)
    t = Tail(L, case)
    B, T, D, MID, C = t.dims
    for i in range(5):  # a zero size
        dims = list(t.dims)
        dims[i] = 0
        st, o = t.fwd(dims=dims)
        assert st == SS_ERR_ARG and all(b.untouched() for b in o.values()), dims
    st, o = t.fwd(drop=(1.0, 1, 1))
    assert st == SS_ERR_ARG and all(b.untouched() for b in o.values())
    st, o = t.fwd(d_logits=False)  # labels without a place for the gradient
    assert st == SS_ERR_ARG and all(b.untouched() for b in o.values())
    st, o = t.fwd()
    assert st == 0
    st, g = t.bwd(o, drop=(1.0, 1, 1))
    assert st == SS_ERR_ARG and all(b.untouched() for b in g.values())
