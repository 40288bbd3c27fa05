"""GPU: ss_eval_accum (csrc/eval.hip) against NumPy -- a float64 log-softmax and a stable argmax.

Exact: confusion, first_seen, correct, y_true_out, y_pred_out.  The loss: one wave (B <= 64) is bit-equal to
ss_ce_ls_fwd_bwd(denom=1, d_logits=NULL) on the same rows; above that it is within the order-free bound of a float sum,
(n - 1) * 2^-24 * sum |l_b|, of the float64 sum of the per-row losses l_b, each taken from ss_ce_ls_fwd_bwd one row at a time."""
import numpy as np
import pytest
import torch

from gpu_support import L  # noqa: F401

pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1


def make_rows(rng, B, C):
    """Logits with exact ties planted at the maximum (every third row; every sixth one at the true class)."""
    lg = rng.normal(size=(B, C)).astype(np.float32) * 3
    y = rng.integers(0, C, B).astype(np.int64)
    if C >= 2:
        for b in range(0, B, 3):
            top = np.float32(lg[b].max() + 1)
            j, k = rng.choice(C, 2, replace=False)
            if b % 6 == 0:
                j = y[b]
                k = (j + 1 + rng.integers(0, C - 1)) % C
            lg[b, j] = lg[b, k] = top
    return lg, y


class Accum:
    def __init__(self, C, dev="cuda"):
        self.loss = torch.zeros(1, device=dev)
        self.correct = torch.zeros(1, device=dev, dtype=torch.int32)
        self.conf = torch.zeros(C, C, device=dev, dtype=torch.int32)
        self.first = torch.full((C, C), I32_MAX, device=dev, dtype=torch.int32)
        self.err = torch.zeros(1, device=dev, dtype=torch.int32)

    def add(self, L, lg, y, eps, first_row, outs=True):
        B, C = lg.shape
        lg_d, y_d = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
        yt = torch.full((B,), 77, device="cuda", dtype=torch.int32) if outs else None
        yp = torch.full((B,), 77, device="cuda", dtype=torch.int32) if outs else None
        L.call("ss_eval_accum", lg_d.data_ptr(), y_d.data_ptr(), B, C, eps, first_row, self.loss.data_ptr(),
               self.correct.data_ptr(), self.conf.data_ptr(), self.first.data_ptr(), L.ptr(yt), L.ptr(yp), self.err.data_ptr(),
               L.stream())
        torch.cuda.synchronize()
        return (yt.cpu().numpy(), yp.cpu().numpy()) if outs else None


class Ref:
    """The same accumulators in NumPy; rows with a label outside [0, C) add nothing."""

    def __init__(self, C):
        self.C, self.correct = C, 0
        self.conf = np.zeros((C, C), np.int32)
        self.first = np.full((C, C), I32_MAX, np.int32)
        self.losses, self.spans = [], []  # per row: the float64 loss, max(1, max_c |logit_c - lse|)

    def f32_tolerance(self):
        """What float32 may lose against the float64 losses.  Per row: exp and log are a few ulp, the C-term sums of exp(.) and of
        (logit_c - lse) lose at most (C - 1) ulp of their size each, and every quantity is at most ``span`` = max(1, max |logit - lse|)
        large: (2 C + 10) * 2^-24 * span.  Summing n rows in any order adds (n - 1) * 2^-24 * sum |l_b|."""
        return (2 * self.C + 10) * 2.0 ** -24 * sum(self.spans) + (len(self.losses) - 1) * 2.0 ** -24 * np.abs(self.losses).sum()

    def add(self, lg, y, eps, first_row):
        B, C = lg.shape
        x = lg.astype(np.float64)
        lsm = x - x.max(1, keepdims=True)
        lsm = lsm - np.log(np.exp(lsm).sum(1, keepdims=True))
        pred = np.argmax(lg, 1)  # first among equals
        yt, yp = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
        for b in range(B):
            if not 0 <= y[b] < C:
                continue
            t, p = int(y[b]), int(pred[b])
            yt[b], yp[b] = t, p
            self.conf[t, p] += 1
            self.first[t, p] = min(self.first[t, p], first_row + b)
            self.correct += int(t == p)
            self.losses.append((1 - eps) * -lsm[b, t] + eps * -lsm[b].mean())
            self.spans.append(max(1.0, float(np.abs(lsm[b]).max())))
        return yt, yp


def ce_loss_sum(L, lg, y, eps, into):
    """ss_ce_ls_fwd_bwd(denom=1, d_logits=NULL) of these rows added into ``into`` (1,)."""
    lg_d, y_d = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
    L.call("ss_ce_ls_fwd_bwd", lg_d.data_ptr(), y_d.data_ptr(), lg.shape[0], lg.shape[1], eps, 1.0, None, into.data_ptr(), None,
           L.stream())
    torch.cuda.synchronize()


def ce_row_losses(L, lg, y, eps):
    """l_b of every row: ss_ce_ls_fwd_bwd one row at a time (one wave, one atomic into a zero: exact)."""
    B, C = lg.shape
    lg_d, y_d = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
    out = torch.zeros(B, device="cuda")
    for b in range(B):
        L.call("ss_ce_ls_fwd_bwd", lg_d.data_ptr() + 4 * b * C, y_d.data_ptr() + 8 * b, 1, C, eps, 1.0, None, out.data_ptr() + 4 * b,
               None, L.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("B", [1, 17, 64, 65, 300])
@pytest.mark.parametrize("C", [1, 2, 5, 100, 130])
def test_eval_accum_matches_numpy(L, C, B):
    rng = np.random.default_rng(1000 * C + B)
    for eps in (0.0, 0.05):
        for first_row in (0, 1000):
            acc, ref = Accum(C), Ref(C)
            ce_sum = torch.zeros(1, device="cuda")
            rows = []
            for call in range(2):  # two consecutive calls into the same accumulators
                lg, y = make_rows(rng, B, C)
                fr = first_row + call * B
                got_t, got_p = acc.add(L, lg, y, eps, fr)
                want_t, want_p = ref.add(lg, y, eps, fr)
                assert np.array_equal(got_t, want_t) and np.array_equal(got_p, want_p)
                assert np.array_equal(acc.conf.cpu().numpy(), ref.conf)
                assert np.array_equal(acc.first.cpu().numpy(), ref.first)
                assert int(acc.correct) == ref.correct and int(acc.conf.sum()) == (call + 1) * B
                loss = np.float32(acc.loss.item())
                if B <= 64:
                    ce_loss_sum(L, lg, y, eps, ce_sum)
                    assert loss.tobytes() == np.float32(ce_sum.item()).tobytes(), (loss, ce_sum.item())
                else:
                    rows.append(ce_row_losses(L, lg, y, eps))
                    lb = np.concatenate(rows)
                    bound = (len(lb) - 1) * 2.0 ** -24 * np.abs(lb).sum()
                    print(f"C={C} B={B} eps={eps} rows={len(lb)}: |loss_sum - sum| = {abs(float(loss) - lb.sum()):.3e}, bound {bound:.3e}")
                    assert abs(float(loss) - lb.sum()) <= bound
                assert abs(float(loss) - sum(ref.losses)) <= ref.f32_tolerance()  # the float64 log-softmax itself
            assert int(acc.err) == 0


def test_eval_accum_skips_rows_with_a_label_outside_the_classes(L):
    """Labels -1, C and 2^32 + 1 (which a cast to int would turn into class 1): never an index, -1 in both outputs, the flag set,
    and the accumulators are those of the batch without these rows (first_seen keeps the other rows' positions)."""
    B, C, eps = 70, 5, 0.05
    rng = np.random.default_rng(9)
    lg, y = make_rows(rng, B, C)
    bad = {0: -1, 13: C, 14: -1, 40: 2 ** 32 + 1, 66: C, 69: -1}
    yb = y.copy()
    for b, v in bad.items():
        yb[b] = v
    acc, ref = Accum(C), Ref(C)
    got_t, got_p = acc.add(L, lg, yb, eps, 1000)
    want_t, want_p = ref.add(lg, yb, eps, 1000)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_p, want_p)
    assert all(got_t[b] == -1 and got_p[b] == -1 for b in bad) and (got_t >= 0).sum() == B - len(bad)
    assert int(acc.err) == 1
    assert np.array_equal(acc.conf.cpu().numpy(), ref.conf) and int(acc.conf.sum()) == B - len(bad)
    assert np.array_equal(acc.first.cpu().numpy(), ref.first) and int(acc.correct) == ref.correct
    keep = np.array([b for b in range(B) if b not in bad])
    lb = ce_row_losses(L, lg[keep], y[keep], eps)
    assert abs(float(acc.loss) - lb.sum()) <= (len(lb) - 1) * 2.0 ** -24 * np.abs(lb).sum()
    # NULL outputs are legal, and the flag stays the caller's: a clean batch does not clear it
    acc.add(L, lg, y, eps, 2000, outs=False)
    assert int(acc.err) == 1 and int(acc.conf.sum()) == 2 * B - len(bad)
