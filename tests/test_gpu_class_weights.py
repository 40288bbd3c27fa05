"""GPU: class-weighted cross entropy -- ss_class_weight_sum, ss_ce_ls_w_fwd_bwd, ss_tail_fwd_w, ss_eval_accum_w through the C ABI,
``Trainer(class_weights=)``, ``evaluate*(class_weights=)`` and ``fit(class_weights="balanced")``.

The reference value everywhere is ``torch.nn.functional.cross_entropy(logits.double(), y, weight=w.double(), label_smoothing=eps)``
on the CPU with its autograd gradient.  Every measured figure is printed before it is compared."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import weights as W  # noqa: E402
from gpu_support import L, WORDS, cuda, make_weights, ss, tail_call, write_clips  # noqa: E402, F401

U = 2.0 ** -24
I32_MAX = 2 ** 31 - 1
LOSS_BOUND = 10 * 9.781275e-08  # the run-to-run atomic noise tests/test_gpu_data_parallel.py allows on a loss


def make_rows(g, B, C):
    """3 * N(0, 1) logits; with three rows or more, row 1 has a 40-wide gap above the rest and row 2 two equal maxima."""
    lg = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    if B >= 3:
        plant_gap(lg, 1, int(y[1]))
        plant_tie(lg, 2, C)
    return lg, y


def plant_gap(lg, b, j):
    lg[b] = torch.linspace(-1, 1, lg.shape[1])
    lg[b, j] = 41.0


def plant_tie(lg, b, C):
    top = float(lg[b].max()) + 1.0
    lg[b, C - 1] = top
    lg[b, C // 2 - (C == 2)] = top


def reference(lg, y, w, eps, den=None):
    """float64 on the CPU: (loss, d loss / d logits).  ``den``: the normaliser, if it is not the sum of w[y] over these rows."""
    x = lg.double().clone().requires_grad_(True)
    if den is None:
        loss = F.cross_entropy(x, y, weight=w.double(), label_smoothing=eps)
    else:
        loss = F.cross_entropy(x, y, weight=w.double(), label_smoothing=eps, reduction="sum") / den
    loss.backward()
    return float(loss.detach()), x.grad


def weight_sum(L, y_d, w_d, C):
    out = torch.full((1,), -7.0, device="cuda")
    L.call("ss_class_weight_sum", y_d.data_ptr(), y_d.numel(), w_d.data_ptr(), C, out.data_ptr(), L.stream())
    return out


def ce_w(L, lg_d, y_d, w_d, den_d, eps, want_grad=True, want_correct=True):
    B, C = lg_d.shape
    d = torch.full((B, C), 9.0, device="cuda") if want_grad else None
    loss = torch.zeros(1, device="cuda")
    correct = torch.zeros(1, device="cuda", dtype=torch.int32) if want_correct else None
    L.call("ss_ce_ls_w_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, w_d.data_ptr(), den_d.data_ptr(), L.ptr(d),
           loss.data_ptr(), L.ptr(correct), L.stream())
    torch.cuda.synchronize()
    return d, loss, correct


def check_rows(L, tag, lg, y, w, eps):
    """One batch through ss_class_weight_sum + ss_ce_ls_w_fwd_bwd against the float64 reference, with the tolerances the
    unweighted kernel holds in tests/test_gpu_kernels.py::test_ce_label_smoothing (loss 2e-6 * max(1, |loss|), gradient
    atol 1e-7 + rtol 1e-5); then the same rows as a slice of a longer label vector (a data-parallel rank's shard)."""
    B, C = lg.shape
    lg_d, y_d, w_d = cuda(lg), cuda(y), cuda(w)
    hits = int((torch.from_numpy(np.argmax(lg.numpy(), 1)) == y).sum())
    g2 = torch.Generator().manual_seed(B + C)
    y_long = torch.cat([torch.randint(0, C, (4,), generator=g2), y, torch.randint(0, C, (5,), generator=g2)])
    for what, labels, sl in (("own rows", y, slice(0, B)), ("slice of a global batch", y_long, slice(4, 4 + B))):
        labels_d = cuda(labels)
        den = weight_sum(L, labels_d, w_d, C)
        d, loss, correct = ce_w(L, lg_d, labels_d[sl].contiguous(), w_d, den, eps)
        den64 = float(w.double()[labels].sum())
        loss_ref, grad_ref = reference(lg, y, w, eps, den64)
        if what == "own rows":  # (torch's own mean reduction divides by the same sum)
            assert abs(loss_ref - reference(lg, y, w, eps)[0]) < 1e-12
        e_loss = abs(float(loss) - loss_ref)
        err = (d.double().cpu() - grad_ref).abs()
        print(f"{tag} {what}: loss err {e_loss:.3e} (ref {loss_ref:.6f}), d_logits max err {float(err.max()):.3e} "
              f"(ref scale {float(grad_ref.abs().max()):.3e}), den {float(den):.7f} vs {den64:.7f}")
        assert e_loss < 2e-6 * max(1.0, abs(loss_ref))
        assert bool((err <= 1e-7 + 1e-5 * grad_ref.abs()).all()), float((err - 1e-5 * grad_ref.abs()).max())
        assert int(correct) == hits
    # NULL d_logits and NULL correct stay legal
    den = weight_sum(L, y_d, w_d, C)
    _, loss2, _ = ce_w(L, lg_d, y_d, w_d, den, eps, want_grad=False, want_correct=False)
    assert abs(float(loss2) - reference(lg, y, w, eps)[0]) < 2e-6 * max(1.0, abs(float(loss2)))


# --------------------------------------------------------------------------------------------- 1. the weighted CE kernel
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("C", [2, 5, 37, 100])
@pytest.mark.parametrize("B", [1, 17, 64, 65, 257])
def test_weighted_ce_kernel(L, B, C, eps):
    """B: one row, part of a wave, a full wave, a wave + 1, two 256-thread blocks + 1.  A batch of one row cannot hold the two
    planted rows besides a random one: it is run three times, once with each."""
    g = torch.Generator().manual_seed(1000 * B + C)
    w = make_weights(g, C)
    lg, y = make_rows(g, B, C)
    check_rows(L, f"B={B} C={C} eps={eps}", lg, y, w, eps)
    if B == 1:
        gap, tie = lg.clone(), lg.clone()
        plant_gap(gap, 0, int(y[0]))
        plant_tie(tie, 0, C)
        check_rows(L, f"B=1 C={C} eps={eps} gap", gap, y, w, eps)
        check_rows(L, f"B=1 C={C} eps={eps} tie", tie, y, w, eps)
        y_other = (y + 1) % C  # the gap above a class that is not the label: a loss near 40 w[y]
        check_rows(L, f"B=1 C={C} eps={eps} gap, other label", gap, y_other, w, eps)


# --------------------------------------------------------------------------------------------- 2. w == 1 is the old kernel
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("C", [2, 5, 37, 100])
@pytest.mark.parametrize("B", [1, 17, 64, 65, 257])
def test_unit_weights_give_the_bits_of_the_unweighted_kernel(L, B, C, eps):
    g = torch.Generator().manual_seed(77 * B + C)
    lg, y = make_rows(g, B, C)
    lg_d, y_d = cuda(lg), cuda(y)
    ones, den = torch.ones(C, device="cuda"), torch.full((1,), float(B), device="cuda")
    d_w, loss_w, correct_w = ce_w(L, lg_d, y_d, ones, den, eps)
    d_u, loss_u = torch.full((B, C), 5.0, device="cuda"), torch.zeros(1, device="cuda")
    correct_u = torch.zeros(1, device="cuda", dtype=torch.int32)
    L.call("ss_ce_ls_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, float(B), d_u.data_ptr(), loss_u.data_ptr(),
           correct_u.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(d_w, d_u), float((d_w - d_u).abs().max())
    assert int(correct_w) == int(correct_u)
    if B <= 64:  # one wave: one atomic into a zero, no order to differ in (tests/test_gpu_eval_accum.py)
        assert loss_w.cpu().numpy().tobytes() == loss_u.cpu().numpy().tobytes(), (float(loss_w), float(loss_u))
    else:
        assert abs(float(loss_w) - float(loss_u)) <= (B - 1) * U * abs(float(loss_u))


def tail_inputs(B, T, C, Hd, lengths):
    g = torch.Generator().manual_seed(B * 7 + T)
    sd = {k: v for k, v in W.make_state_dict(31 + B, 84, C, False, hidden=Hd).items() if k.startswith(("pool.", "head."))}
    h = torch.randn(B, T, 2 * Hd, generator=g)
    for b in range(B):
        h[b, lengths[b]:] = 0
    y = torch.randint(0, C, (B,), generator=g)
    return {k: cuda(v) for k, v in sd.items()}, h, y


def test_fused_tail_unit_weights_give_the_bits_of_the_unweighted_tail(L):
    B, T, C, Hd, lengths = 7, 11, 5, 192, [4, 1, 5, 9, 2, 11, 3]
    P, h, y = tail_inputs(B, T, C, Hd, lengths)
    h_d, len_d, y_d = cuda(h), cuda(torch.tensor(lengths, dtype=torch.int32)), cuda(y)
    dims = (B, T, 2 * Hd, 128, C)
    ones, den = torch.ones(C, device="cuda"), torch.full((1,), float(B), device="cuda")
    for eps in (0.0, 0.05):
        old = tail_call(L, "ss_tail_fwd", P, h_d, len_d, y_d, dims, eps, (float(B),))
        new = tail_call(L, "ss_tail_fwd_w", P, h_d, len_d, y_d, dims, eps, (ones.data_ptr(), den.data_ptr()))
        for k in ("logits", "d_logits", "attn", "xhat", "rstd", "ln", "mid", "mid_d"):
            assert torch.equal(old[k], new[k]), k
        assert int(old["correct"]) == int(new["correct"])
        # (seven atomics in an order that may differ)
        assert abs(float(old["loss"]) - float(new["loss"])) <= (B - 1) * U * abs(float(old["loss"]))


@pytest.mark.parametrize("C", [5, 100])
def test_fused_tail_weighted_loss_and_gradient(L, C):
    """ss_tail_fwd_w (a wave per row, classes across the lanes; C = 100 needs two passes) on its own logits: loss and d_logits
    against the float64 reference with the tolerances of the weighted CE kernel above; the normaliser is that of a longer label
    vector.  A row with a label outside the classes gets a zero gradient row and adds nothing."""
    B, T, Hd, lengths = 7, 11, 192, [4, 1, 5, 9, 2, 11, 3]
    P, h, y = tail_inputs(B, T, C, Hd, lengths)
    g = torch.Generator().manual_seed(C)
    w = make_weights(g, C)
    y_long = torch.cat([y, torch.randint(0, C, (6,), generator=g)])
    w_d = cuda(w)
    y_long_d = cuda(y_long)
    den = weight_sum(L, y_long_d, w_d, C)
    h_d, len_d = cuda(h), cuda(torch.tensor(lengths, dtype=torch.int32))
    dims = (B, T, 2 * Hd, 128, C)
    out = tail_call(L, "ss_tail_fwd_w", P, h_d, len_d, cuda(y), dims, 0.05, (w_d.data_ptr(), den.data_ptr()))
    logits = out["logits"].cpu()
    loss_ref, grad_ref = reference(logits, y, w, 0.05, float(w.double()[y_long].sum()))
    err = (out["d_logits"].double().cpu() - grad_ref).abs()
    print(f"tail C={C}: loss err {abs(float(out['loss']) - loss_ref):.3e}, d_logits max err {float(err.max()):.3e}")
    assert abs(float(out["loss"]) - loss_ref) < 2e-6 * max(1.0, abs(loss_ref))
    assert bool((err <= 1e-7 + 1e-5 * grad_ref.abs()).all())
    assert int(out["correct"]) == int((torch.from_numpy(np.argmax(logits.numpy(), 1)) == y).sum())
    yb = y.clone()
    yb[0], yb[4] = -1, C
    keep = [b for b in range(B) if b not in (0, 4)]
    out = tail_call(L, "ss_tail_fwd_w", P, h_d, len_d, cuda(yb), dims, 0.05, (w_d.data_ptr(), den.data_ptr()))
    loss_ref, grad_ref = reference(logits[keep], y[keep], w, 0.05, float(w.double()[y_long].sum()))
    assert not bool(out["d_logits"][0].any()) and not bool(out["d_logits"][4].any())
    assert bool(((out["d_logits"].double().cpu()[keep] - grad_ref).abs() <= 1e-7 + 1e-5 * grad_ref.abs()).all())
    assert abs(float(out["loss"]) - loss_ref) < 2e-6 * max(1.0, abs(loss_ref))


# --------------------------------------------------------------------------------------------- 3. ss_class_weight_sum
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_class_weight_sum(L, n):
    C = 7
    g = torch.Generator().manual_seed(n)
    w = make_weights(g, C)
    y = torch.randint(0, C, (n,), generator=g)
    w_d, y_d = cuda(w), cuda(y)
    a, b = weight_sum(L, y_d, w_d, C), weight_sum(L, y_d, w_d, C)
    torch.cuda.synchronize()
    exact = float(w.double()[y].sum())
    print(f"n={n}: sum {float(a):.9g}, float64 {exact:.9g}, err {abs(float(a) - exact):.3e}, bound {(n - 1) * U * exact:.3e}")
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert abs(float(a) - exact) <= (n - 1) * U * exact  # (w > 0: the sum of |w[y]| is the sum)
    # labels outside the classes add nothing: the same labels with -1, C and 2^32 + 1 strewn in
    bad = torch.tensor([-1, C, 2 ** 32 + 1], dtype=torch.int64)
    pos = torch.randint(0, n + 1, (3,), generator=g).tolist()
    mixed = y.tolist()
    for p, v in sorted(zip(pos, bad.tolist()), reverse=True):
        mixed.insert(p, v)
    mixed_d = cuda(torch.tensor(mixed, dtype=torch.int64))
    c = weight_sum(L, mixed_d, w_d, C)
    torch.cuda.synchronize()
    assert abs(float(c) - exact) <= (n - 1) * U * exact
    if n == 1:
        assert float(c) == float(w[y[0]]) == float(a)


# --------------------------------------------------------------------------------------------- 4. ss_eval_accum_w
class Accum:
    def __init__(self, C):
        self.loss = torch.zeros(1, device="cuda")
        self.wsum = torch.zeros(1, device="cuda")
        self.correct = torch.zeros(1, device="cuda", dtype=torch.int32)
        self.conf = torch.zeros(C, C, device="cuda", dtype=torch.int32)
        self.first = torch.full((C, C), I32_MAX, device="cuda", dtype=torch.int32)
        self.err = torch.zeros(1, device="cuda", dtype=torch.int32)

    def add(self, L, lg_d, y_d, eps, first_row, w_d=None):
        B, C = lg_d.shape
        yt = torch.full((B,), 77, device="cuda", dtype=torch.int32)
        yp = torch.full((B,), 77, device="cuda", dtype=torch.int32)
        if w_d is None:
            L.call("ss_eval_accum", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, first_row, self.loss.data_ptr(),
                   self.correct.data_ptr(), self.conf.data_ptr(), self.first.data_ptr(), yt.data_ptr(), yp.data_ptr(),
                   self.err.data_ptr(), L.stream())
        else:
            L.call("ss_eval_accum_w", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, first_row, w_d.data_ptr(), self.loss.data_ptr(),
                   self.wsum.data_ptr(), self.correct.data_ptr(), self.conf.data_ptr(), self.first.data_ptr(), yt.data_ptr(),
                   yp.data_ptr(), self.err.data_ptr(), L.stream())
        torch.cuda.synchronize()
        return yt, yp


def weighted_rows(lg, y, w, eps):
    """float64, per row with a label inside the classes: the weighted loss l_b, w[y_b], and what float32 may lose on l_b --
    the bound of tests/test_gpu_eval_accum.py::Ref.f32_tolerance, (2 C + 10) u span with span = max(1, max |logit - lse|), with one
    more product per term and one more C-term sum for the weights, (3 C + 12) u span, times the largest weight (every term of l_b
    carries one weight)."""
    C = lg.shape[1]
    ok = (y >= 0) & (y < C)
    x, yy = lg.double()[ok], y[ok]
    lsm = torch.log_softmax(x, 1)
    l = F.cross_entropy(x, yy, weight=w.double(), label_smoothing=eps, reduction="none")
    span = lsm.abs().max(1).values.clamp(min=1.0)
    return l.numpy(), w.double()[yy].numpy(), ((3 * C + 12) * U * float(w.max()) * span).numpy()


def sums_tolerance(l, wy, row_tol):
    """-> (tolerance of the float32 sum of the losses, of the float32 sum of the weights), any order of summation."""
    n = len(l)
    return float(row_tol.sum() + (n - 1) * U * np.abs(l).sum()), float((n - 1) * U * wy.sum())


@pytest.mark.parametrize("C", [2, 5, 100])
@pytest.mark.parametrize("B", [1, 64, 65, 300])
def test_eval_accum_w(L, B, C):
    g = torch.Generator().manual_seed(31 * B + C)
    w = make_weights(g, C)
    w_d = cuda(w)
    for eps in (0.0, 0.05):
        acc_w, acc_u = Accum(C), Accum(C)
        rows = []
        for call in range(2):  # two consecutive calls into the same accumulators
            lg, y = make_rows(g, B, C)
            if call == 1 and B >= 64:  # rows that count nowhere
                y[0], y[B - 1], y[B // 2] = -1, C, 2 ** 32 + 1
            lg_d, y_d = cuda(lg), cuda(y)
            got = acc_w.add(L, lg_d, y_d, eps, 1000 + call * B, w_d)
            want = acc_u.add(L, lg_d, y_d, eps, 1000 + call * B)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert torch.equal(acc_w.conf, acc_u.conf) and torch.equal(acc_w.first, acc_u.first)
            assert int(acc_w.correct) == int(acc_u.correct) and int(acc_w.err) == int(acc_u.err) == int(call == 1 and B >= 64)
            rows.append(weighted_rows(lg, y, w, eps))
            l, wy, row_tol = (np.concatenate([r[k] for r in rows]) for k in range(3))
            assert int(acc_w.conf.sum()) == len(l)
            tol_num, tol_den = sums_tolerance(l, wy, row_tol)
            num, den = float(acc_w.loss), float(acc_w.wsum)
            ref = float(l.sum() / wy.sum())
            # num / den - N / D = (num - N) / den + (N / D) (D - den) / den
            tol = (tol_num + abs(ref) * tol_den) / den
            print(f"B={B} C={C} eps={eps} rows={len(l)}: loss sum err {abs(num - l.sum()):.3e} (tol {tol_num:.3e}), weight sum err "
                  f"{abs(den - wy.sum()):.3e} (tol {tol_den:.3e}), mean loss err {abs(num / den - ref):.3e} (tol {tol:.3e})")
            assert abs(num - l.sum()) <= tol_num and abs(den - wy.sum()) <= tol_den
            assert abs(num / den - ref) <= tol
        if B >= 64:
            want_rows = 2 * B - 3
            assert int(acc_w.conf.sum()) == want_rows


# --------------------------------------------------------------------------------------------- 5. / 6. the trainer's step
STEP_W = (0.4, 2.1, 1.0, 0.6, 0.9)
CASES = {"landmarks": dict(roi=None, B=5, T=7, lengths=[7, 1, 4, 7, 2]), "roi32": dict(roi=(32, 32), B=3, T=5, lengths=[5, 1, 3])}


def step_case(name):
    c = CASES[name]
    sd = W.make_state_dict(11, 12, 5, c["roi"] is not None)
    X, Lh, R, y = W.make_inputs(11, c["B"], c["T"], 12, 5, c["roi"], lengths=c["lengths"])
    return sd, X, Lh, R, y


def fresh_model(ss, sd, use_roi):
    m = ss.BiGRUClassifier(12, 5, use_roi=use_roi, hidden=192)
    m.load_state_dict(sd)
    return m.cuda().eval()


def fused_step(ss, name, rows=slice(None), world=1, rank=0, y_global=None):
    """-> (loss, gradient bucket, this step's logits) of one ``Trainer(class_weights=STEP_W).step`` on ``rows`` of the case."""
    sd, X, Lh, R, y = step_case(name)
    m = fresh_model(ss, sd, R is not None)
    tr = ss.Trainer(m, dropout=False, class_weights=STEP_W, world_size=world)
    tr.rank = rank
    Xd, Ld, yd = cuda(X[rows]), cuda(Lh[rows]), cuda(y[rows])
    Rd = cuda(R[rows]) if R is not None else None
    loss, _ = tr.step(Xd, Ld, Rd, yd, y_global=y_global)
    torch.cuda.synchronize()
    logits = m._workspace(Xd, Rd, train=True, slot=0).logits.cpu().clone()
    return float(loss), m.flat_grads.clone(), logits, m


@pytest.fixture(scope="module")
def one_process(ss):
    return {}


def one_process_step(ss, cache, name):
    if name not in cache:
        cache[name] = fused_step(ss, name)
    return cache[name]


@pytest.mark.parametrize("name", ["landmarks", "roi32"])
def test_trainer_step_matches_the_autograd_path(ss, one_process, name):
    """``Trainer(class_weights=w).step`` against ``model(X, lengths)`` -> torch's weighted loss -> ``backward()``, the path of
    INTEGRATION.md section 2.  tests/test_gpu_model.py holds each of the two paths to the oracle within 2e-4 * max|ref| + 2e-3 * |ref|
    per tensor (pool.score.bias, whose true gradient is zero: below 1e-6 on both sides); the same bound is held here between
    the two.  The returned loss against the float64 reference on the step's own logits: the fused tail's 3e-6 * max(1, |loss|)."""
    sd, X, Lh, R, y = step_case(name)
    loss, bucket, logits, m = one_process_step(ss, one_process, name)
    w = torch.tensor(STEP_W)
    loss_ref, _ = reference(logits, y, w, 0.05)
    print(f"{name}: step loss {loss:.7f}, float64 on its logits {loss_ref:.7f}, diff {abs(loss - loss_ref):.3e}")
    assert abs(loss - loss_ref) < 3e-6 * max(1.0, abs(loss_ref))
    m2 = fresh_model(ss, sd, R is not None)
    out = m2(cuda(X), cuda(Lh), cuda(R) if R is not None else None)
    assert float((out.detach().cpu() - logits).abs().max()) < 5e-5
    F.cross_entropy(out, cuda(y), weight=w.cuda(), label_smoothing=0.05).backward()
    G = m._views_of(bucket)
    worst = 0.0
    for k, p in m2.named_parameters():
        got, ref = G[k].cpu(), p.grad.cpu()
        if k == "pool.score.bias":
            assert float(got.abs().max()) < 1e-6 and float(ref.abs().max()) < 1e-6
            continue
        scale = max(float(ref.abs().max()), 1e-4)
        worst = max(worst, float((got - ref).abs().max()) / scale)
        bad = (got - ref).abs() > 2e-4 * scale + 2e-3 * ref.abs()
        assert not bad.any(), f"{k}: max err {float((got - ref).abs().max()):.3e} vs scale {scale:.3e}"
    print(f"{name}: worst gradient difference between the fused step and the autograd path: {worst:.3e} of the tensor's scale")


def test_shards_add_up(ss, one_process):
    """The landmark-only batch cut 3 / 2 over two ``Trainer(world_size=2)`` objects without a process group (no collective is
    issued), each stepping on its rows with ``y_global`` = all five labels: the two gradient buckets sum to the one-process bucket,
    the two losses to the one-process loss.  What differs is the grouping of float32 sums and the order of float atomics: the
    losses are held to the atomic-order noise tests/test_gpu_data_parallel.py allows on a loss (10 x 9.78e-08), the buckets, per
    tensor, to what tests/test_gpu_kernels.py allows between two summation orders of one gradient (atol 2e-5 * max|ref| + 1e-8,
    rtol 1e-4).  A step normalised by its OWN rows instead would be off by the factors 5.0 / 3.1 and 5.0 / 1.5."""
    sd, X, Lh, R, y = step_case("landmarks")
    loss1, bucket1, _, m = one_process_step(ss, one_process, "landmarks")
    y_all = cuda(y)
    parts = [fused_step(ss, "landmarks", rows=rows, world=2, rank=r, y_global=y_all) for r, rows in enumerate((slice(0, 3), slice(3, 5)))]
    loss2 = parts[0][0] + parts[1][0]
    print(f"one process {loss1:.8f}, two shards {parts[0][0]:.8f} + {parts[1][0]:.8f} = {loss2:.8f}, diff {abs(loss1 - loss2):.3e}")
    assert abs(loss1 - loss2) <= LOSS_BOUND
    own = fused_step(ss, "landmarks", rows=slice(0, 3), world=2, rank=0)[0]  # (default y_global = its own rows: another number)
    assert abs(own - parts[0][0]) > 1e-2
    G1, G2 = m._views_of(bucket1), m._views_of(parts[0][1] + parts[1][1])
    for k in G1:
        ref, got = G1[k].cpu(), G2[k].cpu()
        err = (got - ref).abs()
        assert bool((err <= 2e-5 * float(ref.abs().max()) + 1e-8 + 1e-4 * ref.abs()).all()), (k, float(err.max()), float(ref.abs().max()))


# --------------------------------------------------------------------------------------------- 7. / 8. evaluation and fit
COUNTS = (8, 5, 2)
EVAL_W = (0.5, 1.0, 1.9)


@pytest.fixture(scope="module")
def clip_dir(tmp_path_factory):
    """3 words x (8, 5, 2) clips, built the way test_harness_fit_evaluate_checkpoint builds its directory."""
    return write_clips(str(tmp_path_factory.mktemp("cw") / "clips_npz"), WORDS, counts=COUNTS)


def test_evaluate_under_class_weights(ss, clip_dir):
    from silent_speech_amd import harness as Hn

    info = Hn.scan_clips(clip_dir)
    store = ss.DeviceClipStore(info["files"], info["label_to_id"], max_t=24)
    n = len(store)
    assert n == 15
    torch.manual_seed(3)
    model = ss.BiGRUClassifier(info["x_dim"], 3, use_roi=True, roi_emb=32, hidden=192).cuda()
    w = torch.tensor(EVAL_W)
    loss_h, acc_h, y_true, y_pred = Hn.evaluate(model, store, batch_size=4, class_weights=EVAL_W)
    res = Hn.evaluate_device(model, store, batch_size=4, class_weights=EVAL_W)
    # the logits of the same batches, read back
    model.eval()
    logits = []
    with torch.no_grad():
        for lo in range(0, n, 4):
            X, T, R, _ = store.batch(list(range(lo, min(n, lo + 4))), augment=False)
            logits.append(model(X, T, R).cpu())
    logits, y = torch.cat(logits), torch.tensor(y_true)
    assert y.tolist() == store.y.cpu().tolist()
    l, wy, row_tol = weighted_rows(logits, y, w, 0.05)
    tol_num, tol_den = sums_tolerance(l, wy, row_tol)
    ref = float(l.sum() / wy.sum())
    assert abs(ref - reference(logits, y, w, 0.05)[0]) < 1e-12
    tol = (tol_num + abs(ref) * tol_den) / float(wy.sum()) * (1 + 1e-6)
    print(f"weighted validation loss: evaluate {loss_h:.8f}, evaluate_device {res.loss:.8f}, float64 {ref:.8f}, tol {tol:.3e}")
    assert abs(loss_h - ref) <= tol and abs(res.loss - ref) <= tol
    # both sum the same 15 float32 losses (same row function, same logits) in their own order, and 15 weights
    pair = (2 * (n - 1) * U * float(np.abs(l).sum()) + abs(ref) * (n - 1) * U * float(wy.sum())) / float(wy.sum()) * (1 + 1e-6)
    assert abs(loss_h - res.loss) <= pair, (loss_h, res.loss, pair)
    assert abs(res.weight_sum - wy.sum()) <= tol_den and abs(res.loss - res.loss_sum / res.weight_sum) < 1e-12
    # accuracy and confusion: exact
    assert res.acc == acc_h and res.n == n
    conf = np.zeros((3, 3), np.int64)
    for t, p in zip(y_true, y_pred):
        conf[t, p] += 1
    assert np.array_equal(res.confusion, conf)
    assert res.y_true.cpu().tolist() == y_true and res.y_pred.cpu().tolist() == y_pred
    assert y_pred == np.argmax(logits.numpy(), 1).tolist()
    # the unweighted figures are another number, and are what they were
    plain = Hn.evaluate_device(model, store, batch_size=4)
    assert plain.weight_sum == n and abs(plain.loss - res.loss) > 1e-4 and np.array_equal(plain.confusion, conf)
    # two ranks without a group, numerators and denominators added by hand: the loss of the whole store, whatever the cut
    parts = [Hn.evaluate_device(model, store, batch_size=4, rank=r, world_size=2, class_weights=EVAL_W) for r in range(2)]
    assert [p.n for p in parts] == [8, 7]
    by_hand = sum(p.loss_sum for p in parts) / sum(p.weight_sum for p in parts)
    print(f"two shards by hand {by_hand:.8f}, one rank {res.loss:.8f}, diff {abs(by_hand - res.loss):.3e}, tol {tol:.3e}")
    assert abs(by_hand - ref) <= tol and abs(by_hand - res.loss) <= pair
    assert np.array_equal(parts[0].confusion + parts[1].confusion, conf)
    # (the mean of the two per-shard means is NOT that number: why the per-batch averaging of the reference was not kept)
    assert abs(sum(p.loss * p.n for p in parts) / n - ref) > 10 * tol
    store.check()


def test_fit_with_balanced_weights_on_device_planned_batches(ss, clip_dir, tmp_path):
    from silent_speech_amd import harness as Hn

    out = str(tmp_path / "word_model.pt")
    logs, history = [], []
    best = Hn.fit(clip_dir, out, epochs=2, batch_size=4, patience=5, max_t=24, lr=3e-3, log=logs.append, plan="device",
                  history=history, class_weights="balanced")
    assert len([ln for ln in logs if ln.startswith("ep ")]) == 2 and len(history) == 2
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) and h["train_loss"] > 0 and h["val_loss"] > 0 for h in history)
    assert best > 0 and any("saved" in ln for ln in logs) and os.path.exists(out)
    model, id_to_label, max_t, use_roi = ss.load_classifier(out)
    assert max_t == 24 and use_roi and sorted(id_to_label.values()) == WORDS


# --------------------------------------------------------------------------------------------- 9. the bf16 engine
def test_bf16_engine_weighted_step(ss):
    """One weighted step of the bf16 engine at the smallest training shape of tests/test_gpu_model_c5.py (B = 6, T = 7, 100 words):
    the engine hands the same ``ce`` tuple to the same fused tail, so the loss is that of the float64 reference on the step's own
    logits within the tail's 3e-6 * max(1, |loss|)."""
    C5 = dict(roi_emb=64, hidden=512, cnn_channels=(16, 32, 64, 96))
    sd = W.make_state_dict(3, 84, 100, True, **C5)
    X, Lh, R, y = W.make_inputs(3, 6, 7, 84, 100, (96, 96))
    m = ss.BiGRUClassifier(84, 100, use_roi=True, precision="bf16", **C5)
    m.load_state_dict(sd)
    m.cuda().eval()
    w = make_weights(torch.Generator().manual_seed(5), 100)
    tr = ss.Trainer(m, dropout=False, class_weights=w)
    Xd, Rd = cuda(X), cuda(R)
    loss, correct = tr.step(Xd, cuda(Lh), Rd, cuda(y))
    torch.cuda.synchronize()
    logits = m._workspace(Xd, Rd, train=True, slot=0).logits.cpu()
    loss_ref, _ = reference(logits, y, w, 0.05)
    print(f"bf16 weighted step: loss {float(loss):.7f}, float64 on its logits {loss_ref:.7f}")
    assert abs(float(loss) - loss_ref) < 3e-6 * max(1.0, abs(loss_ref))
    assert int(correct) == int((torch.from_numpy(np.argmax(logits.numpy(), 1)) == y).sum())
    assert bool(torch.isfinite(m.flat_grads).all()) and float(tr.grad_norm()) > 0
    m.check_health()
