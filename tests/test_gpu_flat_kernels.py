"""GPU: the flat streaming kernels past their grid caps -- ``ss_sumsq_f32``, ``ss_adam_clip`` (csrc/optim.hip), ``ss_zero_f32x2``,
``ss_copy_rows_f32``, ``ss_train_prologue`` (csrc/step_helpers.hip), ``ss_dropout`` and ``ss_softmax_topk`` (csrc/pool_head.hip)
-- through the C ABI against the host references of tests/flat_ref.py (float64 or integers; tests/test_flat_ref_cpu.py pins
those without a GPU).

Each of the streaming kernels is a grid-stride loop over 16-byte lanes with a capped grid and a tail for ``n & 3``; the sizes
below are the smallest that reach the second trip of each loop, both sides of each cap, the seam between an unrolled loop and
its remainder, and the tail.  Every buffer a kernel writes is over-allocated by ``GUARD`` words of random bits behind its last
16-byte lane, and those words are the same afterwards.  Bounds are derived in ``flat_ref`` (Adam, dropout, the sum's chain of
adds) or next to the check (softmax); every test prints its largest error / bound ratio."""
import numpy as np
import pytest
import torch

import flat_ref as FR
import optim_ref as OR
from gpu_support import L  # noqa: F401
from test_gpu_ema_resume import ADAM, GUARD, NS, bits, guarded, optimiser_inputs

pytestmark = pytest.mark.gpu


def guard_fill(values, seed, dtype=torch.float32):
    """-> (device buffer holding ``values`` with the guard words behind it, as ``dtype``; the allocation's bits on the host)."""
    values = torch.as_tensor(values).reshape(-1)
    n = values.numel()
    g = torch.Generator().manual_seed(seed)
    host = torch.randint(-2 ** 31, 2 ** 31 - 1, ((n + 3) // 4 * 4 + GUARD,), generator=g, dtype=torch.int64).to(torch.int32)
    host[:n] = values.contiguous().view(torch.int32)
    return host.cuda().view(dtype), host


def random_bits(n, seed):
    """n words of arbitrary bit patterns + the guard -> (device float32 view, host int32)."""
    return guarded(n, seed)


def ratio(err, bound):
    return float((err / bound).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------- ss_sumsq_f32
@pytest.mark.parametrize("n", FR.SUMSQ_NS)
def test_sumsq_is_exact_on_small_integers(L, n):
    """Integers in {0, 1, 2}: every partial sum is an integer below 2**24 (asserted on the host in test_flat_ref_cpu.py), so
    the result is the integer sum bit for bit in any order of adds.  The kernel adds onto the word it is given."""
    x = FR.sumsq_exact_input(n)
    total = int((x.astype(np.int64) ** 2).sum())
    x_d = torch.from_numpy(x).cuda()
    acc, acc0 = guard_fill(torch.tensor([0.0]), n)
    L.call("ss_sumsq_f32", x_d.data_ptr(), n, acc.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert float(acc[0]) == float(total), (n, float(acc[0]), total)
    if n <= FR.SUMSQ_TWICE_MAX_N:
        L.call("ss_sumsq_f32", x_d.data_ptr(), n, acc.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert float(acc[0]) == float(2 * total), (n, float(acc[0]), 2 * total)
    assert torch.equal(bits(acc)[1:], acc0[1:])
    assert np.array_equal(x_d.cpu().numpy(), x)


@pytest.mark.parametrize("n", [1310723, 3145731])
def test_sumsq_of_normal_values_against_float64(L, n):
    """All terms are non-negative, so the relative error of the sum is at most that of the longest chain of rounded operations
    a term goes through, ``k u / (1 - k u)`` with k = ``flat_ref.sumsq_chain(n)`` (computed from n and the grid)."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    want = float((x.double() ** 2).sum())
    x_d, acc = x.cuda(), torch.zeros(1, device="cuda")
    L.call("ss_sumsq_f32", x_d.data_ptr(), n, acc.data_ptr(), L.stream())
    torch.cuda.synchronize()
    k = FR.sumsq_chain(n)
    bound = k * FR.U / (1 - k * FR.U) * want
    err = abs(float(acc[0]) - want)
    print(f"sumsq n={n}: chain {k}, err / bound {err / bound:.4f}")
    assert err <= bound, (n, k, float(acc[0]), want)
    assert abs(np.sqrt(float(acc[0])) - np.sqrt(want)) <= bound / np.sqrt(want)  # the norm the clip coefficient is made of


# ---------------------------------------------------------------------------------------------------------- ss_adam_clip
ADAM_NS_LARGE = [524287, 524288, 524289, 1048579, 1572867]  # both sides of 2048 x 256, two full sweeps + a tail, three
MAX_NORM = 1.0
SUMSQS = [0.0, 1e-12, MAX_NORM ** 2, 4 * MAX_NORM ** 2, 1e6]
STEPS = [1, 7, 10000]
GRAD_SCALES = [1.0, 0.25]
ALL_COMBOS = [(s, q, gs) for s in STEPS for q in SUMSQS for gs in GRAD_SCALES]
# a large n runs one combination per sumsq value: every step and both scales among them
LARGE_COMBOS = [(1, 0.0, 0.25), (7, 1e-12, 1.0), (10000, MAX_NORM ** 2, 0.25), (1, 4 * MAX_NORM ** 2, 1.0), (7, 1e6, 0.25)]


def run_adam_clip(L, host, n, step, sumsq, grad_scale, seed):
    """One ``ss_adam_clip`` launch on guarded copies of the host arrays (p, g, m, v) with the sumsq word written by the test
    -> dict of the new p, m, v (NumPy); asserts the guards, g and the sumsq word are untouched."""
    dev = [guard_fill(torch.from_numpy(a), seed + i) for i, a in enumerate(host)]
    ssq = torch.tensor([sumsq], dtype=torch.float32).cuda()
    P_, G_, M_, V_ = (d[0] for d in dev)
    L.call("ss_adam_clip", P_.data_ptr(), G_.data_ptr(), M_.data_ptr(), V_.data_ptr(), n, ssq.data_ptr(), grad_scale, MAX_NORM,
           *ADAM[2:], step, L.stream())
    torch.cuda.synchronize()
    for (d, d0), name in zip(dev, "pgmv"):
        assert torch.equal(bits(d)[n:], d0[n:]), f"{name}: guard words"
    assert torch.equal(bits(G_), dev[1][1]) and float(ssq[0]) == float(np.float32(sumsq))
    return dict(p=P_[:n].cpu().numpy(), m=M_[:n].cpu().numpy(), v=V_[:n].cpu().numpy())


def check_adam(got, host, step, sumsq, grad_scale, worst, what):
    want, bound = FR.adam_clip_expected(*host, np.float32(sumsq), step, lr=ADAM[2], max_norm=MAX_NORM, beta1=ADAM[3],
                                        beta2=ADAM[4], eps=ADAM[5], grad_scale=grad_scale)
    for k in "mvp":
        err = np.abs(got[k].astype(np.float64) - want[k])
        worst[k] = max(worst[k], ratio(err, bound[k]))
        assert (err <= bound[k]).all(), (what, k, ratio(err, bound[k]), int(np.argmax(err / bound[k])))
    assert not np.array_equal(got["p"], host[0])  # (the step did something)


@pytest.mark.parametrize("n", NS + ADAM_NS_LARGE)
def test_adam_clip_against_float64(L, n):
    p, m, v, _, grads = optimiser_inputs(n, 300 + n)
    host = tuple(t.numpy() for t in (p, grads[1], m, v))
    worst = dict(p=0.0, m=0.0, v=0.0)
    for i, (step, sumsq, grad_scale) in enumerate(ALL_COMBOS if n <= max(NS) else LARGE_COMBOS):
        got = run_adam_clip(L, host, n, step, sumsq, grad_scale, 10 * i)
        check_adam(got, host, step, sumsq, grad_scale, worst, (n, step, sumsq, grad_scale))
    print(f"adam_clip n={n}: largest err / bound  m {worst['m']:.4f}  v {worst['v']:.4f}  p {worst['p']:.4f}")


@pytest.mark.parametrize("n", [1025, 524289])
def test_adam_clip_with_no_gradient_only_decays_the_moments(L, n):
    """sumsq = 0 and g = 0: m and v become float32(beta * m) and float32(beta * v) -- the product of two float32 numbers is
    exact in float64, rounded once --, p moves by the decayed moments alone."""
    p, m, v, _, _ = optimiser_inputs(n, 500 + n)
    host = (p.numpy(), np.zeros(n, np.float32), m.numpy(), v.numpy())
    got = run_adam_clip(L, host, n, 7, 0.0, 1.0, 3)
    s = FR.adam_scalars(7, *ADAM[2:])
    assert np.array_equal(got["m"], (s["beta1"] * host[2].astype(np.float64)).astype(np.float32))
    assert np.array_equal(got["v"], (s["beta2"] * host[3].astype(np.float64)).astype(np.float32))
    check_adam(got, host, 7, 0.0, 1.0, dict(p=0.0, m=0.0, v=0.0), n)


# ------------------------------------------------------------------------------------------------------------ ss_dropout
DROP_NS_SMALL = [1, 2, 5, 1023]
OFFSETS = [0, 5 << 40, 2 ** 32 - 3, 2 ** 64 - 2]  # ..., the low counter word carries inside the first lanes, the counter wraps
DROP_SEED = 0x9E3779B97F4A7C15


def dropout_input(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    x[::7] = -0.0
    if n > 3:
        x[3] = 0.0
    relu_of = torch.randn(n, generator=g)
    relu_of[::5] = 0.0
    relu_of[1::11] = -0.0
    return x, relu_of


def check_dropout(L, x, n, p, seed, offset, relu_of, in_place, worst):
    """One launch; the zero pattern is exactly ``dropout_expected``'s (dropped elements are +0.0, kept ones carry the sign of
    x), kept values within its bound; x (out of place), relu_of and the guards are untouched."""
    what = (n, p, hex(offset), relu_of is not None, in_place)
    x_d, x0 = guard_fill(x, n + 1)
    y_d, y0 = (x_d, x0) if in_place else random_bits(n, n + 2)
    r_d = None if relu_of is None else relu_of.cuda()
    L.call("ss_dropout", x_d.data_ptr(), y_d.data_ptr(), n, p, seed, offset, None if r_d is None else r_d.data_ptr(), L.stream())
    torch.cuda.synchronize()
    keep, want, bound = FR.dropout_expected(x.numpy(), n, p, seed, offset, None if relu_of is None else relu_of.numpy())
    got, got_bits = y_d[:n].cpu().numpy(), bits(y_d)[:n].numpy()
    assert not got_bits[~keep].any(), (what, "a dropped element is not +0.0", int(np.flatnonzero(got_bits * ~keep)[0]))
    err = np.abs(got[keep].astype(np.float64) - want[keep])
    worst[0] = max(worst[0], ratio(err, bound[keep]))
    assert (err <= bound[keep]).all(), (what, ratio(err, bound[keep]))
    assert np.array_equal(np.signbit(got[keep]), np.signbit(want[keep])), what
    assert np.array_equal(got[keep] != 0, x.numpy()[keep] != 0), what
    assert torch.equal(bits(y_d)[n:], y0[n:]), (what, "guard words")
    if not in_place:
        assert torch.equal(bits(x_d), x0), what
    if r_d is not None:
        assert torch.equal(bits(r_d), bits(relu_of)), what
    return keep


@pytest.mark.parametrize("n", DROP_NS_SMALL)
def test_dropout_small_against_philox(L, n):
    """Every p, every offset; with and without ``relu_of``; out of place and with y == x."""
    x, relu_of = dropout_input(n, n)
    worst, kept = [0.0], {}
    for p in FR.DROPOUT_PS:
        for offset in OFFSETS:
            for r in (None, relu_of):
                for in_place in (False, True):
                    keep = check_dropout(L, x, n, p, DROP_SEED, offset, r, in_place, worst)
                    if r is None:
                        kept[(p, offset)] = keep
    print(f"dropout n={n}: largest err / bound {worst[0]:.4f}")
    if n == 1023:  # the streams differ by offset, and p decides how much is kept
        assert len({kept[(0.5, o)].tobytes() for o in OFFSETS}) == len(OFFSETS)
        assert 0.42 < kept[(0.5, 0)].mean() < 0.58 and kept[(FR.DROPOUT_PS[-1], 0)].sum() == 0


# (n, offset, relu_of, y == x): one sweep of the capped grid is 2048 x 256 x 4 = 2 097 152 elements
DROP_LARGE = [(2097151, 5 << 40, False, False), (2097153, 2 ** 32 - 3, True, True), (4194309, 2 ** 64 - 2, False, True),
              (6291463, 0, True, False)]


@pytest.mark.parametrize("n,offset,with_relu,in_place", DROP_LARGE)
def test_dropout_large_against_philox(L, n, offset, with_relu, in_place):
    x, relu_of = dropout_input(n, n)
    worst = [0.0]
    keep = check_dropout(L, x, n, 0.2, DROP_SEED, offset, relu_of if with_relu else None, in_place, worst)
    print(f"dropout n={n}: kept {keep.mean():.4f}, largest err / bound {worst[0]:.4f}")
    assert abs(keep.mean() - (0.8 * float((relu_of > 0).float().mean()) if with_relu else 0.8)) < 2e-3


def test_dropout_refuses_bad_arguments(L):
    x, x0 = guard_fill(torch.randn(9), 1)
    y, y0 = random_bits(9, 2)
    lib = L.load()
    for args in ((None, y.data_ptr(), 9, 0.2), (x.data_ptr(), None, 9, 0.2), (x.data_ptr(), y.data_ptr(), 0, 0.2),
                 (x.data_ptr(), y.data_ptr(), 9, 1.0), (x.data_ptr(), y.data_ptr(), 9, -0.1)):
        assert lib.ss_dropout(*args, 1, 0, None, L.stream()) == -1, args
    torch.cuda.synchronize()
    assert torch.equal(bits(x), x0) and torch.equal(bits(y), y0)


# --------------------------------------------------------------------------------------------------------- ss_zero_f32x2
@pytest.mark.parametrize("na,nb", [(0, 5), (5, 0), (1, 3), (4, 4), (1027, 2), (2097153, 7), (3, 4194309)])
def test_zero_two_buffers(L, na, nb):
    a, a0 = random_bits(na, 3 * na + 1)
    b, b0 = random_bits(nb, 3 * nb + 2)
    L.call("ss_zero_f32x2", a.data_ptr() if na else None, na, b.data_ptr() if nb else None, nb, L.stream())
    torch.cuda.synchronize()
    for t, t0, n in ((a, a0, na), (b, b0, nb)):
        got = bits(t)
        assert not bool(got[:n].any()), (na, nb, int(torch.nonzero(got[:n])[0]))  # every word +0.0
        assert torch.equal(got[n:], t0[n:]), (na, nb, "guard words")


def test_zero_two_buffers_argument_check(L):
    a, a0 = random_bits(9, 1)
    lib, s = L.load(), L.stream()
    assert lib.ss_zero_f32x2(None, 0, None, 0, s) == 0  # nothing to do: ok, without a launch
    assert lib.ss_zero_f32x2(a.data_ptr(), 0, a.data_ptr(), 0, s) == 0
    assert lib.ss_zero_f32x2(None, 5, a.data_ptr(), 5, s) == -1 and lib.ss_zero_f32x2(a.data_ptr(), 5, None, 1, s) == -1
    assert lib.ss_zero_f32x2(a.data_ptr(), -1, a.data_ptr(), 5, s) == -1 and lib.ss_zero_f32x2(a.data_ptr(), 5, a.data_ptr(), -1, s) == -1
    assert lib.ss_zero_f32x2(a.data_ptr() + 4, 5, None, 0, s) == -1 and lib.ss_zero_f32x2(None, 0, a.data_ptr() + 8, 5, s) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(a), a0)


# ------------------------------------------------------------------------------------------------------ ss_copy_rows_f32
@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(1, 1, 1, 1), (7, 84, 84, 148), (7, 84, 148, 84), (7680, 84, 84, 148),
                                                     (6243, 85, 90, 97)])  # the last two: above 2048 x 256 elements
def test_copy_rows(L, rows, cols, ld_src, ld_dst):
    src, src0 = random_bits(rows * ld_src, rows + 1)
    dst, dst0 = random_bits(rows * ld_dst, rows + 2)
    L.call("ss_copy_rows_f32", src.data_ptr(), ld_src, dst.data_ptr(), ld_dst, rows, cols, L.stream())
    torch.cuda.synchronize()
    want = dst0.clone()
    want[:rows * ld_dst].view(rows, ld_dst)[:, :cols] = src0[:rows * ld_src].view(rows, ld_src)[:, :cols]
    assert torch.equal(bits(dst), want) and torch.equal(bits(src), src0)
    assert not torch.equal(want, dst0)


def test_copy_rows_argument_check(L):
    src, src0 = random_bits(7 * 84, 1)
    dst, dst0 = random_bits(7 * 84, 2)
    lib, s = L.load(), L.stream()
    S, D = src.data_ptr(), dst.data_ptr()
    assert lib.ss_copy_rows_f32(S, 83, D, 84, 7, 84, s) == -1 and lib.ss_copy_rows_f32(S, 84, D, 83, 7, 84, s) == -1  # ld < cols
    assert lib.ss_copy_rows_f32(None, 84, D, 84, 7, 84, s) == -1 and lib.ss_copy_rows_f32(S, 84, None, 84, 7, 84, s) == -1
    assert lib.ss_copy_rows_f32(S, 84, D, 84, 0, 84, s) == -1 and lib.ss_copy_rows_f32(S, 84, D, 84, 7, 0, s) == -1
    torch.cuda.synchronize()
    assert torch.equal(bits(src), src0) and torch.equal(bits(dst), dst0)


# ----------------------------------------------------------------------------------------------------- ss_train_prologue
N_SCALARS, SCALAR_WORDS = 5, 16
# (n_grads, (B, T, cols, E, ld_z), ld_x): the grid is capped at 1024 x 256 threads -- 1 048 576 gradient quads' worth of
# 16-byte lanes or 262 144 copied elements; the last shape copies 756 000 elements and has more than 256 clips
PROLOGUE_CASES = [(5, (5, 7, 84, 64, 148), 84), (1048575, (37, 90, 180, 64, 250), 187), (1048579, (300, 30, 84, 64, 148), 84),
                  (2097161, (5, 7, 84, 64, 148), 90)]


def prologue_lengths(B, T, seed):
    """Lengths that include 0, 1 and T, and one above T."""
    l = np.random.default_rng(seed).integers(0, T + 1, B)
    l[:4] = [T, 0, 1, T + 5]
    return torch.from_numpy(l.astype(np.int64))


class Prologue:
    """The buffers of one ``ss_train_prologue`` call, all pre-filled with random bits, and the checks of what a call leaves."""

    def __init__(self, n_grads, shape, ld_x, seed):
        self.n_grads, (self.B, self.T, self.cols, self.E, self.ld_z), self.ld_x = n_grads, shape, ld_x
        self.rows = self.B * self.T
        self.grads, self.grads0 = random_bits(n_grads, seed)
        self.scal, self.scal0 = random_bits(SCALAR_WORDS, seed + 1)
        self.correct, self.correct0 = guard_fill(torch.tensor([12345], dtype=torch.int32), seed + 2, torch.int32)
        self.len64 = prologue_lengths(self.B, self.T, seed).cuda()
        self.len32, self.len32_0 = guard_fill(torch.full((self.B,), -7, dtype=torch.int32), seed + 3, torch.int32)
        # X: finite values (their bits are compared), Z and the frame list: random bits
        self.X = torch.randn(self.rows, ld_x, generator=torch.Generator().manual_seed(seed + 4)).cuda()
        self.Z, self.Z0 = random_bits(self.rows * self.ld_z, seed + 5)
        self.frames, self.frames0 = guard_fill(torch.full((1 + self.rows,), -9, dtype=torch.int32), seed + 6, torch.int32)

    def args(self, L, frames=True, X=True, len64=True, **over):
        a = dict(grads=self.grads.data_ptr(), n_grads=self.n_grads, scal=self.scal.data_ptr(), n_scal=N_SCALARS,
                 correct=self.correct.data_ptr(), len64=self.len64.data_ptr() if len64 else None, len32=self.len32.data_ptr(),
                 B=self.B, X=self.X.data_ptr() if X else None, ld_x=self.ld_x, Z=self.Z.data_ptr(), ld_z=self.ld_z, rows=self.rows,
                 cols=self.cols, frames=self.frames.data_ptr() if frames else None, E=self.E)
        a.update(over)
        return list(a.values()) + [L.stream()]

    def untouched(self):
        return all(torch.equal(bits(t), t0) for t, t0 in ((self.grads, self.grads0), (self.scal, self.scal0),
                                                          (self.correct, self.correct0), (self.len32, self.len32_0),
                                                          (self.Z, self.Z0), (self.frames, self.frames0)))

    def check(self, frames=True, X=True, len64=True):
        n, B, T, cols, E, ld_z, rows = self.n_grads, self.B, self.T, self.cols, self.E, self.ld_z, self.rows
        g = bits(self.grads)
        assert not bool(g[:n].any()), ("grads", int(torch.nonzero(g[:n])[0]))
        assert torch.equal(g[n:], self.grads0[n:])
        s = bits(self.scal)
        assert not bool(s[:N_SCALARS].any()) and torch.equal(s[N_SCALARS:], self.scal0[N_SCALARS:])
        c = bits(self.correct)
        assert int(c[0]) == 0 and torch.equal(c[1:], self.correct0[1:])
        l32, l64 = bits(self.len32), self.len64.cpu()
        if len64:
            assert torch.equal(l32[:B].long(), l64) and torch.equal(l32[B:], self.len32_0[B:])
        else:
            assert torch.equal(l32, self.len32_0)
        z, want = bits(self.Z), self.Z0.clone()
        if X:
            wz = want[:rows * ld_z].view(rows, ld_z)
            wz[:, :cols] = bits(self.X)[:, :cols]
            if frames:
                pad = (torch.arange(T)[None, :] >= l64.clamp(0, T)[:, None]).reshape(-1)  # rows (b, t) outside every clip
                assert 0 < int(pad.sum()) < rows
                wz[pad, cols:cols + E] = 0
        assert torch.equal(z, want), ("Z", int(torch.nonzero(z != want)[0]))
        f = bits(self.frames)
        if frames:
            listed = torch.from_numpy(FR.active_frames_expected(l64.numpy(), B, T))
            assert torch.equal(f[:len(listed)], listed) and torch.equal(f[len(listed):], self.frames0[len(listed):])
        else:
            assert torch.equal(f, self.frames0)


@pytest.mark.parametrize("n_grads,shape,ld_x", PROLOGUE_CASES)
def test_train_prologue(L, n_grads, shape, ld_x):
    c = Prologue(n_grads, shape, ld_x, n_grads % 1000)
    L.call("ss_train_prologue", *c.args(L))
    torch.cuda.synchronize()
    c.check()


@pytest.mark.parametrize("form", ["frames", "X", "len64"])
def test_train_prologue_forms_with_a_null_pointer(L, form):
    """``frames`` null: the embedding columns and the list stay; ``X`` null (then ``frames`` is null too): Z stays; ``lengths64``
    null (then ``frames`` is null too): the int32 lengths stay."""
    n_grads, shape, ld_x = PROLOGUE_CASES[2]
    keep = dict(frames=dict(frames=False), X=dict(frames=False, X=False), len64=dict(frames=False, len64=False))[form]
    c = Prologue(n_grads, shape, ld_x, 77)
    L.call("ss_train_prologue", *c.args(L, **keep))
    torch.cuda.synchronize()
    c.check(**keep)


def test_train_prologue_refusals_write_nothing(L):
    c = Prologue(1029, (5, 7, 84, 64, 148), 84, 5)
    lib = L.load()
    bad = [dict(grads=None), dict(n_grads=0), dict(grads=c.grads.data_ptr() + 4, n_grads=1028), dict(n_scal=-1), dict(n_scal=257),
           dict(scal=None), dict(len32=None), dict(B=0), dict(Z=None), dict(rows=0), dict(cols=0), dict(ld_x=83), dict(ld_z=83),
           dict(E=-1), dict(ld_z=147), dict(rows=34)]  # ... ld_z < cols + E, rows no multiple of B
    for over in bad:
        assert lib.ss_train_prologue(*c.args(L, **over)) == -1, over
    assert lib.ss_train_prologue(*c.args(L, X=False)) == -1 and lib.ss_train_prologue(*c.args(L, len64=False)) == -1  # frames needs both
    torch.cuda.synchronize()
    assert c.untouched()
    assert lib.ss_train_prologue(*c.args(L)) == 0  # and the same call with good arguments runs
    torch.cuda.synchronize()
    c.check()


# ------------------------------------------------------------------------------------------------------- ss_softmax_topk
TOPK_CASES = [(1, 1, 1), (5, 3, 3), (7, 10, 3), (4, 64, 64), (5, 65, 5), (9, 100, 3), (3, 130, 64), (2, 3, 5)]
ROW_KINDS = ["random", "constant", "dup_same_lane", "dup_other_lane", "with_inf", "pm80"]


def topk_rows(kind, B, C, rng):
    """(B, C) float32 logits, or None where C is too small for the kind.  random: a permutation of a grid, 0.037 between
    neighbours.  dup_same_lane: the maximum at c and c + 64 (one lane's second trip); dup_other_lane: at c and c' < c + 64."""
    x = np.stack([rng.permutation(C) * 0.037 - 1.5 for _ in range(B)]).astype(np.float32)
    if kind == "constant":
        x[:] = rng.standard_normal((B, 1)).astype(np.float32)
    elif kind == "dup_same_lane":
        if C <= 64:
            return None
        for b in range(B):
            c = int(rng.integers(0, C - 64))
            x[b, c] = x[b, c + 64] = 7.25
    elif kind == "dup_other_lane":
        if C < 2:
            return None
        for b in range(B):
            c = int(rng.integers(0, C - 1))
            c2 = int(rng.integers(c + 1, min(C, c + 64)))
            x[b, c] = x[b, c2] = 7.25
    elif kind == "with_inf":
        if C < 2:
            return None
        for b in range(B):
            x[b, rng.choice(C, size=max(1, min(C - 1, C // 3)), replace=False)] = -np.inf
    elif kind == "pm80":
        x = np.where(rng.random((B, C)) < 0.5, 80.0, -80.0).astype(np.float32)
        x[:, int(rng.integers(0, C))] = 80.0
    return x


def topk_bound(logits, probs, idx):
    """Bound of each returned probability ``expf(l - m) / se`` in units of u = 2**-24 times itself, by rounded operations:
    the subtraction (at most half an ulp of l - m, which moves the exponential by that much relatively; exact where l = m),
    ``expf`` (1 ulp, HIP's documented accuracy: 2 u) -- once for the numerator and once, weighted by the probabilities, for the
    terms of the denominator; the denominator's ``ceil(C / 64)`` adds per lane, 6 levels of the wave tree; one division; one for
    the second order.  Everything below the smallest normal float32 may be flushed or rounded to a subnormal: 2**-126 on top."""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    C = lg.shape[1]
    with np.errstate(invalid="ignore"):
        sub = 0.5 * OR.f32_ulp(np.where(np.isfinite(lg), lg - lg.max(axis=1, keepdims=True), 0.0)) * (lg != lg.max(axis=1, keepdims=True))
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    sm = e / e.sum(axis=1, keepdims=True)
    sub_den = (sm * sub).sum(axis=1, keepdims=True)
    sub_num = np.take_along_axis(sub, np.maximum(idx, 0), axis=1)
    count = -(-C // 64) + 6 + 1 + 2 * 2 + 1
    return probs * (count * FR.U + sub_num + sub_den) + 2.0 ** -126


@pytest.mark.parametrize("B,C,k", TOPK_CASES)
def test_softmax_topk(L, B, C, k):
    rng = np.random.default_rng(100 * C + k)
    worst = 0.0
    for kind in ROW_KINDS:
        x = topk_rows(kind, B, C, rng)
        if x is None:
            continue
        x_d = torch.from_numpy(x).cuda()
        probs, probs0 = random_bits(B * k, C)
        idx, idx0 = guard_fill(torch.full((B * k,), -5, dtype=torch.int32), C + 1, torch.int32)
        L.call("ss_softmax_topk", x_d.data_ptr(), B, C, k, probs.data_ptr(), idx.data_ptr(), L.stream())
        torch.cuda.synchronize()
        want_p, want_i = FR.softmax_topk_expected(x, k)
        got_i = bits(idx)[:B * k].view(B, k).numpy()
        got_p = probs[:B * k].view(B, k).cpu().numpy()
        assert np.array_equal(got_i, want_i), (kind, got_i.tolist(), want_i.tolist())
        if k > C:
            assert (got_i[:, C:] == -1).all() and not bits(probs)[:B * k].view(B, k)[:, C:].any()  # (+0.0, -1) past C
        bound = topk_bound(x, want_p, want_i)
        err = np.abs(got_p.astype(np.float64) - want_p)
        worst = max(worst, ratio(err, bound))
        assert (err <= bound).all(), (kind, ratio(err, bound))
        if kind == "with_inf":
            assert (got_p[np.take_along_axis(x, np.maximum(want_i, 0), axis=1) == -np.inf] == 0).all()
        assert abs(got_p[:, :C].sum(axis=1) - 1).max() < 1e-5 or k < C
        assert torch.equal(bits(probs)[B * k:], probs0[B * k:]) and torch.equal(bits(idx)[B * k:], idx0[B * k:])
        assert np.array_equal(x_d.cpu().numpy(), x)
    print(f"softmax_topk B={B} C={C} k={k}: largest err / bound {worst:.4f}")


def test_softmax_topk_refuses_k_above_64_and_bad_arguments(L):
    x = torch.randn(3, 130).cuda()
    probs, probs0 = random_bits(3 * 65, 1)
    idx, idx0 = random_bits(3 * 65, 2)
    lib, s = L.load(), L.stream()
    assert lib.ss_softmax_topk(x.data_ptr(), 3, 130, 65, probs.data_ptr(), idx.data_ptr(), s) == -3  # SS_ERR_UNSUPPORTED
    for args in ((None, 3, 130, 3, probs.data_ptr(), idx.data_ptr()), (x.data_ptr(), 0, 130, 3, probs.data_ptr(), idx.data_ptr()),
                 (x.data_ptr(), 3, 0, 3, probs.data_ptr(), idx.data_ptr()), (x.data_ptr(), 3, 130, 0, probs.data_ptr(), idx.data_ptr()),
                 (x.data_ptr(), 3, 130, 3, None, idx.data_ptr()), (x.data_ptr(), 3, 130, 3, probs.data_ptr(), None)):
        assert lib.ss_softmax_topk(*args, s) == -1, args
    torch.cuda.synchronize()
    assert torch.equal(bits(probs), probs0) and torch.equal(bits(idx), idx0)
