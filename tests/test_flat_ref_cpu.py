"""CPU: the host references of tests/flat_ref.py against torch and Random123's known answers, and the conditions under which
tests/test_gpu_flat_kernels.py may call its integer checks exact.  This file is what makes those references trustworthy
without a GPU."""
import numpy as np
import pytest
import torch

import batch_plan_ref as P
import flat_ref as FR
import optim_ref as OR

KAT_WORDS = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]  # Random123 kat_vectors: Philox4x32-10, counter 0, key 0


@pytest.mark.parametrize("eps", [1e-8, 2.0 ** -10])
def test_adam_clip_expected_against_torch_clip_and_adam(eps):
    """Five steps against ``clip_grad_norm_`` + ``torch.optim.Adam`` on float64 tensors, fed the float32 betas and eps.  After
    each step both sides carry on from the reference's p, m, v rounded to float32, as the kernel's buffers would (torch's state
    is set by hand).  What differs inside a step is four scalars that the kernel takes rounded to float32 (sumsq, 1e-6,
    step_size, inv_sqrt_bc2), each off by at most 2**-24 relatively: 1e-6 (17 * 2**-24) of the largest m, v and of the largest
    move of a weight.  The large eps puts the denominator's two terms on one scale, so that an eps on the wrong side of the
    bias correction would show."""
    rng = np.random.default_rng(5)
    n, lr = 1000, 3e-4
    p, _, m, v = FR.optimiser_case(n, 3)
    scales = (4.0, 0.02, 60.0, 0.6, 0.0)  # norms about 6.3 (clipped), 0.03 (not), 95, 0.95 (at the edge), 0
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=float(np.float32(lr)), betas=(float(np.float32(0.9)), float(np.float32(0.999))),
                           eps=float(np.float32(eps)))
    for step, scale in zip((1, 2, 3, 7, 10000), scales):
        g = (rng.standard_normal(n) * 0.05 * scale).astype(np.float32)
        sumsq = np.float32(np.sum(g.astype(np.float64) ** 2))
        want, bound = FR.adam_clip_expected(p, g, m, v, sumsq, step, lr=lr, eps=eps)
        with torch.no_grad():
            tp.copy_(torch.from_numpy(p.astype(np.float64)))
        opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                             exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
        tp.grad = torch.from_numpy(g.astype(np.float64))
        total = torch.nn.utils.clip_grad_norm_([tp], 1.0)
        opt.step()
        assert abs(float(total) - np.sqrt(float(sumsq))) <= 2.0 ** -24 * float(total)
        assert np.abs(want["m"] - opt.state[tp]["exp_avg"].numpy()).max() <= 1e-6 * np.abs(want["m"]).max()
        assert np.abs(want["v"] - opt.state[tp]["exp_avg_sq"].numpy()).max() <= 1e-6 * np.abs(want["v"]).max()
        moved = np.abs(want["p"] - p).max()
        assert np.abs(want["p"] - tp.detach().numpy()).max() <= 1e-6 * moved and 1e-5 < moved < 1e-2, (step, moved)
        if scale == 0.0:  # g = 0: the moments only decay
            assert np.array_equal(want["m"], float(np.float32(0.9)) * m.astype(np.float64))
            assert np.array_equal(want["v"], float(np.float32(0.999)) * v.astype(np.float64))
        # the bounds: a few ulp of the operands, never zero
        for k, size in (("m", np.abs(m)), ("v", v), ("p", np.abs(p))):
            assert (bound[k] > 0).all() and (bound[k] <= 64 * OR.f32_ulp(np.maximum(size, np.abs(want[k])))).all(), (k, step)
        p, m, v = (want[k].astype(np.float32) for k in "pmv")


def test_adam_scalars_are_the_host_codes():
    s = FR.adam_scalars(1)
    assert s["omb1"] == 1.0 - s["beta1"] and s["omb2"] == 1.0 - s["beta2"]  # (Sterbenz: exact in float32, hence in double)
    assert s["beta1"] == float(np.float32(0.9)) != 0.9
    assert s["step_size"] == float(np.float32(float(np.float32(3e-4)) / (1.0 - s["beta1"])))
    big = FR.adam_scalars(10000)
    assert big["step_size"] == float(np.float32(3e-4)) and 1.0 < big["inv_sqrt_bc2"] < 1.0001
    # the coefficient: no clip below max_norm, the scale folded in, sumsq = 0 is fine
    assert FR.clip_coef(0.0) == 1.0 and FR.clip_coef(0.0, 0.25) == 0.25
    assert FR.clip_coef(1.0) == 1.0 / (1.0 + float(np.float32(1e-6)))
    assert abs(FR.clip_coef(4.0) - 0.5) < 1e-6 and abs(FR.clip_coef(64.0, 0.25) - 0.25 * 0.5) < 1e-6


def test_dropout_words_are_the_published_philox_words():
    """Counter 0 under key 0 is the stream of seed 0 at offset 0; the counter wraps at 2**64, so it is also the second quad of
    the stream at offset 2**64 - 1; the carry out of the low word lands in the second counter word."""
    assert FR.dropout_words(4, 0, 0).tolist() == KAT_WORDS
    assert FR.dropout_words(8, 0, 2 ** 64 - 1)[4:].tolist() == KAT_WORDS
    assert FR.dropout_words(3, 0, 0).tolist() == KAT_WORDS[:3]
    w = FR.dropout_words(16, 77, 2 ** 32 - 2)
    for q in range(4):
        one = P.philox4x32((2 ** 32 - 2 + q) & 0xFFFFFFFF, (2 ** 32 - 2 + q) >> 32, 0, 0, 77, 0)
        assert w[4 * q:4 * q + 4].tolist() == [int(x) for x in one]
    assert w[8:12].tolist() == [int(x) for x in P.philox4x32(0, 1, 0, 0, 77, 0)]
    # a threshold on either side of each published word (as close as a float32 p comes) keeps or drops exactly that element
    x = np.float32([1.0, -2.0, 3.0, -0.0])
    for e, word in enumerate(KAT_WORDS):
        below = np.float32(word / 2 ** 32)
        below = below if float(below) * 2 ** 32 <= word else np.nextafter(below, np.float32(0))
        above = np.nextafter(below, np.float32(1))
        keep_b, want_b, _ = FR.dropout_expected(x, 4, below, 0, 0)
        keep_a, _, _ = FR.dropout_expected(x, 4, above, 0, 0)
        assert keep_b[e] and not keep_a[e]
        assert keep_b.tolist() == [w_ >= int(float(below) * 2 ** 32) for w_ in KAT_WORDS]
        assert want_b[e] == float(x[e]) / (1.0 - float(below))


def test_dropout_expected_edges():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(1001).astype(np.float32)
    x[5], x[6] = -0.0, 0.0
    keep, want, bound = FR.dropout_expected(x, 1001, 0.0, 9, 2 ** 64 - 2)
    assert keep.all() and np.array_equal(want, x.astype(np.float64)) and np.signbit(want[5])  # p = 0: the identity
    keep, want, _ = FR.dropout_expected(x, 1001, 1e-10, 9, 3)
    assert keep.all() and np.array_equal(want, x.astype(np.float64) / (1.0 - float(np.float32(1e-10))))
    keep, want, bound = FR.dropout_expected(x, 1001, 0.2, 9, 5 << 40)
    assert 0.75 < keep.mean() < 0.85 and np.array_equal(want[~keep], np.zeros((~keep).sum())) and not np.signbit(want[~keep]).any()
    assert np.array_equal(bound, 2 * OR.f32_ulp(want))
    relu_of = rng.standard_normal(1001).astype(np.float32)
    relu_of[:3] = [0.0, -0.0, 1e-30]
    keep_r, want_r, _ = FR.dropout_expected(x, 1001, 0.2, 9, 5 << 40, relu_of)
    assert np.array_equal(keep_r, keep & (relu_of > 0)) and not keep_r[0] and not keep_r[1] and keep_r[2] == keep[2]
    assert np.array_equal(want_r, np.where(keep_r, want, 0.0))
    top = FR.DROPOUT_PS[-1]
    keep, want, _ = FR.dropout_expected(x, 1001, top, 9, 0)
    assert top == 1.0 - 2.0 ** -24 and np.array_equal(keep, FR.dropout_words(1001, 9, 0) >= 2 ** 32 - 256)
    assert np.array_equal(want[keep], x[keep].astype(np.float64) * 2.0 ** 24)
    # a shorter n is a prefix, and a stream offset by one counter is the stream moved by four elements
    assert np.array_equal(FR.dropout_expected(x, 10, 0.5, 9, 7)[0], FR.dropout_expected(x, 1001, 0.5, 9, 7)[0][:10])
    assert np.array_equal(FR.dropout_words(40, 9, 8)[:36], FR.dropout_words(40, 9, 7)[4:])


def test_dropout_keep_scale_in_float32_is_within_one_rounding_of_the_float64_one():
    """What lets ``dropout_expected`` state 2 ulp although the kernel rounds three times (1 - p, the reciprocal, the product):
    for every p the GPU tests use, float32(1 / float32(1 - p)) is within 2**-24 of 1 / (1 - p)."""
    for p in FR.DROPOUT_PS:
        p32 = np.float32(p)
        scale32 = float(np.float32(1.0) / (np.float32(1.0) - p32))
        scale64 = 1.0 / (1.0 - float(p32))
        assert abs(scale32 - scale64) <= 2.0 ** -24 * scale64, p


def test_softmax_topk_expected_against_torch_on_tie_free_rows():
    rng = np.random.default_rng(4)
    for B, C, k in ((1, 1, 1), (5, 3, 3), (7, 10, 3), (4, 64, 64), (5, 65, 5), (9, 100, 3), (3, 130, 64)):
        logits = np.stack([(rng.permutation(C) * 0.037 - 1.5) for _ in range(B)]).astype(np.float32)
        probs, idx = FR.softmax_topk_expected(logits, k)
        tp, ti = torch.topk(torch.softmax(torch.from_numpy(logits).double(), dim=1), k, dim=1)
        assert np.array_equal(idx, ti.numpy()) and np.abs(probs - tp.numpy()).max() <= 1e-15
    # ties go to the lower index, slots past C are (0, -1), -inf comes last with probability 0
    probs, idx = FR.softmax_topk_expected(np.float32([[1.0, 3.0, 3.0], [2.0, -np.inf, 2.0]]), 5)
    assert idx.tolist() == [[1, 2, 0, -1, -1], [0, 2, 1, -1, -1]]
    assert probs[1].tolist() == [0.5, 0.5, 0.0, 0.0, 0.0] and probs[0, 0] == probs[0, 1] > probs[0, 2] > 0


def test_active_frames_expected():
    assert FR.active_frames_expected([2, 0, 5, 1], 4, 3).tolist() == [6, 0, 1, 6, 7, 8, 9]
    assert FR.active_frames_expected([-1, 9], 2, 2).tolist() == [2, 2, 3]
    assert FR.active_frames_expected([0, 0], 2, 4).tolist() == [0]


@pytest.mark.parametrize("n", FR.SUMSQ_NS)
def test_exact_sumsq_inputs_stay_below_two_to_the_24(n):
    """All squares are non-negative integers, so the largest partial sum any order of adds can meet is the total -- twice the
    total where the GPU test adds a second call onto the first."""
    x = FR.sumsq_exact_input(n)
    assert x.dtype == np.float32 and x.shape == (n,) and set(np.unique(x).tolist()) <= {0.0, 1.0, 2.0}
    total = int((x.astype(np.int64) ** 2).sum())
    calls = 2 if n <= FR.SUMSQ_TWICE_MAX_N else 1
    assert calls * total < 2 ** 24, (n, total)
    assert n < 100 or total > n  # (not all zeros: about 5 n / 3)
    assert np.array_equal(FR.sumsq_exact_input(n), x)


def test_sumsq_grid_and_chain():
    assert FR.sumsq_grid(1) == (1, 256) and FR.sumsq_grid(1024) == (1, 256) and FR.sumsq_grid(1028) == (2, 512)
    assert FR.sumsq_grid(262144) == (256, 65536) and FR.sumsq_grid(3145731) == (256, 65536)
    # n = 786 436: thread 0 takes one unrolled trip and nothing else; n = 3 145 731: three unrolled trips
    assert FR.sumsq_chain(786436) == 1 + 6 + 1 + 0 + 1 + 6 + 3 + 256
    assert FR.sumsq_chain(3145731) == 1 + 6 + 3 + 0 + 1 + 6 + 3 + 256
    assert FR.sumsq_chain(786432) == 1 + 3 + 0 + 3 + 1 + 6 + 3 + 256
    assert FR.sumsq_chain(5) == 1 + 3 + 0 + 1 + 1 + 6 + 3 + 1
