"""CPU: mixup on the device-planned path -- the restatement of its two kernels (tests/mixup_ref.py), the quantile table, the policy's
validation and fingerprint rule, ``fit``'s refusals, and the presence of the new entry points in the built library."""
import numpy as np
import pytest

import batch_plan_ref as P
import mixup_ref as M

N_DRAWS = 20000


def _table(alpha=0.2, N=1024):
    from silent_speech_amd.device_data import mixup_table

    return mixup_table(alpha, N)


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_perm_is_a_permutation_and_the_rest_follows_it(B):
    rng = np.random.default_rng(B)
    lens, y = rng.integers(0, 25, B), rng.integers(0, 7, B)
    table = _table()
    for seed, first in ((0, 0), (7, 2 ** 40 + 5)):
        p = M.plan(lens, y, True, first, seed, 1.0, table)
        assert p["mixed"] and sorted(p["perm"].tolist()) == list(range(B))
        assert 0 <= p["k"] <= 256 and float(p["lam"]) == p["k"] / 256.0
        assert np.array_equal(p["y_b"], y[p["perm"]]) and np.array_equal(p["lens_m"], np.maximum(lens, lens[p["perm"]]))
        # the rank of (key, row): sorting the rows by their rank sorts the keys, rows ascending among equal keys
        keys = M.row_keys(first, B, seed)
        order = np.argsort(p["perm"])
        assert all((keys[a], a) < (keys[b], b) for a, b in zip(order[:-1], order[1:]))
    for augment, prob in ((False, 1.0), (True, 0.0)):
        q = M.plan(lens, y, augment, 3, 1, prob, table)
        assert not q["mixed"] and q["k"] == 256 and float(q["lam"]) == 1.0
        assert np.array_equal(q["perm"], np.arange(B)) and np.array_equal(q["y_b"], y) and np.array_equal(q["lens_m"], lens)


def test_equal_keys_rank_by_row():
    """The restatement's ranking (``mixup_ref.rank_keys``, what ``plan`` calls) against the kernel's rule counted row by row: the rows
    j with key_j < key_b, or key_j == key_b and j < b.  Keys drawn from four values, so most rows tie; with every key equal the
    permutation is the identity."""
    assert M.rank_keys(np.array([5, 1, 5, 1, 5], np.uint64)).tolist() == [2, 0, 3, 1, 4]
    assert M.rank_keys(np.full(9, 7, np.uint64)).tolist() == list(range(9))
    rng = np.random.default_rng(1)
    for B in (1, 2, 65, 257):
        keys = rng.integers(0, 4, B).astype(np.uint64) * np.uint64(0x40000000)
        want = [sum(1 for j in range(B) if (int(keys[j]), j) < (int(keys[b]), b)) for b in range(B)]
        assert M.rank_keys(keys).tolist() == want


def test_batch_draws_have_the_stated_probability_and_spread():
    """20 000 batches: the share that is mixed and the histogram of the table index (16 bins of 64 entries) lie within five
    binomial standard deviations of the stated probability -- the bound of tests/test_batch_plan_cpu.py."""
    N = 1024
    firsts = P._index_range(12345, N_DRAWS)
    u0, u1, _, _ = P.draw(firsts, M.TAG_MIXUP, 0, 99)
    for prob in (0.5, 0.25):
        share = float((u0 < np.uint64(P.thr(prob))).mean())
        print(f"mixup_prob {prob}: mixed share {share:.4f}")
        assert abs(share - prob) < 5 * np.sqrt(prob * (1 - prob) / N_DRAWS)
    at = P.mulhi(u1, N).astype(np.int64)
    assert at.min() >= 0 and at.max() < N
    counts = np.bincount(at // 64, minlength=16)
    p = 1.0 / 16
    print("table index histogram:", counts.tolist())
    assert np.all(np.abs(counts - N_DRAWS * p) < 5 * np.sqrt(N_DRAWS * p * (1 - p))), counts
    # the scalar path of the restatement agrees with the vectorised draws
    for i in (0, 1, 777):
        mixed, idx = M.batch_draw(12345 + i, 99, True, 0.5, N)
        assert mixed == bool(u0[i] < np.uint64(P.thr(0.5))) and idx == at[i]
    # the "mixp" stream is none of the others
    assert M.TAG_MIXUP == int.from_bytes(b"mixp", "big") and M.TAG_MIXUP not in (P.TAG_NOISE, P.TAG_SAMPLER, P.TAG_PLANNER)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("alpha", [0.2, 0.4, 1.0, 2.0])
def test_table_is_monotone_symmetric_and_in_range(alpha):
    t = _table(alpha)
    assert t.dtype == np.uint16 and t.shape == (1024,)
    k = t.astype(np.int64)
    assert k.min() >= 0 and k.max() <= 256 and np.all(np.diff(k) >= 0)
    assert np.array_equal(k + k[::-1], np.full(1024, 256))
    if alpha < 1:  # mass at the ends: more than half of the table within 1/8 of 0 or 1
        assert ((k <= 32) | (k >= 224)).mean() > 0.5
    if alpha > 1:
        assert ((k <= 32) | (k >= 224)).mean() < 0.1


@pytest.mark.parametrize("alpha", [0.2, 0.4, 1.0, 2.0])
def test_table_against_scipy(alpha):
    sp = pytest.importorskip("scipy.special")
    q = 256.0 * sp.betaincinv(alpha, alpha, (np.arange(1024) + 0.5) / 1024)
    err = np.abs(_table(alpha).astype(np.float64) - q)
    print(f"alpha {alpha}: max |k - 256 Q| = {err.max():.6f}")
    assert np.all(err <= 0.5 + 1e-6)


def test_alpha_one_is_the_uniform_table_and_other_sizes_work():
    i = np.arange(1024)
    assert np.array_equal(_table(1.0), np.floor(256 * (i + 0.5) / 1024 + 0.5).astype(np.uint16))
    small = _table(0.4, 64)
    assert small.shape == (64,) and np.array_equal(small.astype(int) + small[::-1].astype(int), np.full(64, 256))
    for bad in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=0.2, N=1000), dict(alpha=0.2, N=1),
                dict(alpha=1e-320)):  # (1 / alpha overflows: an error, not a table of NaN cast to integers)
        with pytest.raises(ValueError):
            _table(**bad)


@pytest.mark.parametrize("alpha", [1e-3, 8.0, 64.0, 1000.0, 1e12])
def test_table_at_the_ends_of_the_alpha_range(alpha):
    """Whatever finite alpha > 0 ``AugmentPolicy`` accepts gives a table, not NaN: monotone, symmetric, all mass at 0 and 1 as alpha
    goes to 0 and at 1/2 as it grows (the standard deviation of Beta(a, a) is 1 / (2 sqrt(2 a + 1)))."""
    k = _table(alpha).astype(np.int64)
    assert k.min() >= 0 and k.max() <= 256 and np.all(np.diff(k) >= 0) and np.array_equal(k + k[::-1], np.full(1024, 256))
    if alpha < 1:
        assert ((k == 0) | (k == 256)).mean() > 0.99
    else:
        sd = 256.0 / (2.0 * np.sqrt(2.0 * alpha + 1.0))
        assert abs(k.astype(float).std() - sd) <= 0.05 * sd + 0.5, (k.std(), sd)
        assert np.abs(k - 128).max() <= 6 * sd + 1


# ------------------------------------------------------------------------------------------------ the blend
def test_blend_restatement():
    rng = np.random.default_rng(3)
    B, T = 5, 3
    R = rng.integers(0, 256, (B, T, 4, 8), dtype=np.uint8)
    X = rng.normal(size=(B, T, 7)).astype(np.float32)
    perm = np.array([2, 1, 4, 0, 3])
    ident = np.arange(B)
    # k = 256 and the identity return the inputs, whatever the other one is
    for k in (0, 1, 128, 255, 256):
        assert np.array_equal(M.blend_u8(R, ident, k), R) and np.array_equal(M.blend_f32(X, ident, k), X)
    assert np.array_equal(M.blend_u8(R, perm, 256), R) and np.array_equal(M.blend_f32(X, perm, 256), X)
    assert np.array_equal(M.blend_u8(R, perm, 0), R[perm]) and np.array_equal(M.blend_f32(X, perm, 0), X[perm])
    # u8: the rounded mean, exactly, byte by byte in Python integers
    for k in (1, 77, 128, 255):
        got = M.blend_u8(R, perm, k)
        a, b = R.reshape(B, -1), R[perm].reshape(B, -1)
        want = [[(k * int(p) + (256 - k) * int(q) + 128) >> 8 for p, q in zip(ra, rb)] for ra, rb in zip(a, b)]
        assert got.reshape(B, -1).tolist() == want
        # between the two bytes, and within half a step of the real blend
        lo, hi = np.minimum(R, R[perm]), np.maximum(R, R[perm])
        assert np.all((got >= lo) & (got <= hi))
        assert np.abs(got - (k * R.astype(float) + (256 - k) * R[perm].astype(float)) / 256).max() <= 0.5
    ref, tol = M.blend_f64(X, perm, 128)
    assert np.allclose(ref, 0.5 * X.astype(np.float64) + 0.5 * X[perm]) and np.all(tol >= 0)
    assert M.passthrough_rows(perm, 128).tolist() == [False, True, False, False, False]
    assert M.passthrough_rows(perm, 256).all()


# ------------------------------------------------------------------------------------------------ policy, fit, fingerprint
def test_policy_fields_and_validation():
    import silent_speech_amd as ss

    p = ss.AugmentPolicy()
    assert (p.mixup_prob, p.mixup_alpha) == (0.0, 0.2) and not p.mixup_on
    assert not ss.AugmentPolicy(mixup_alpha=0.4).mixup_on and ss.AugmentPolicy(mixup_prob=0.1).mixup_on
    assert not ss.AugmentPolicy.lineage().mixup_on and ss.AugmentPolicy.lineage(mixup_prob=1.0, mixup_alpha=0.4).mixup_on
    for kw in (dict(mixup_prob=1.5), dict(mixup_prob=-0.1), dict(mixup_prob=float("nan")), dict(mixup_alpha=0.0),
               dict(mixup_alpha=-0.2), dict(mixup_alpha=float("inf")), dict(mixup_alpha="0.2")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ss.AugmentPolicy(**kw)


def test_fingerprint_carries_the_mixup_fields_only_when_it_is_on():
    import silent_speech_amd as ss
    from silent_speech_amd import checkpoint as Ck
    from silent_speech_amd import harness as Hn

    base = dict(seed=42, batch_size=16, world_size=1, max_t=24, lr=3e-3, labels=["aura", "no"], x_dim=20, use_roi=True, n_train=38,
                n_val=7, class_weights=None, ema_decay=None)
    old_keys = {"time_warp_prob", "time_warp_range", "scale_prob", "scale_range", "roi_shift_prob", "roi_shift_max"}
    lin = ss.AugmentPolicy.lineage()
    fp = Hn.run_fingerprint(**base, augment_policy=lin)
    assert set(fp["augment_policy"]) == old_keys
    assert fp["augment_policy"] == dict(time_warp_prob=0.5, time_warp_range=[0.8, 1.2], scale_prob=0.3, scale_range=[0.95, 1.05],
                                        roi_shift_prob=0.0, roi_shift_max=[0, 0])
    off = Hn.run_fingerprint(**base, augment_policy=ss.AugmentPolicy.lineage(mixup_alpha=0.4))  # alpha alone: mixup is off
    assert Ck.fingerprint_difference(fp, off) is None
    on = Hn.run_fingerprint(**base, augment_policy=ss.AugmentPolicy.lineage(mixup_prob=0.5))
    assert set(on["augment_policy"]) == old_keys | {"mixup_prob", "mixup_alpha"}
    assert on["augment_policy"]["mixup_prob"] == 0.5 and on["augment_policy"]["mixup_alpha"] == 0.2
    assert Ck.fingerprint_difference(fp, on) == "augment_policy"
    other = Hn.run_fingerprint(**base, augment_policy=ss.AugmentPolicy.lineage(mixup_prob=0.5, mixup_alpha=0.4))
    assert Ck.fingerprint_difference(on, other) == "augment_policy"
    assert Hn.run_fingerprint(**base, augment_policy=None)["augment_policy"] is None


def test_fit_refuses_what_mixup_does_not_combine_with(tmp_path):
    """Raised before any device or clip is touched: the clip directory does not exist."""
    import silent_speech_amd as ss
    from silent_speech_amd import harness as Hn

    pol = ss.AugmentPolicy(mixup_prob=0.5)
    nowhere, out = str(tmp_path / "no_such_dir"), str(tmp_path / "m.pt")
    with pytest.raises(ValueError, match="data-parallel"):
        Hn.fit(nowhere, out, plan="device", augment_policy=pol, world_size=2, rank=1)
    with pytest.raises(ValueError, match="data-parallel"):
        Hn.fit(nowhere, out, plan="device", augment_policy=pol, process_group=object())
    with pytest.raises(ValueError, match="freeze_cnn"):
        Hn.fit(nowhere, out, plan="device", augment_policy=pol, freeze_cnn=True, init_from=str(tmp_path / "x.pt"))
    with pytest.raises(ValueError, match="plan='device'"):
        Hn.fit(nowhere, out, plan="host", augment_policy=pol)
    with pytest.raises(ValueError, match="1024"):
        Hn.fit(nowhere, out, plan="device", augment_policy=pol, batch_size=2048)


# ------------------------------------------------------------------------------------------------ the library
def test_new_entry_points_exist_and_the_abi_version_stays():
    from silent_speech_amd import _lib

    lib = _lib.load()
    for name in ("ss_batch_plan_mixup", "ss_batch_mixup", "ss_ce_ls_mix_fwd_bwd", "ss_tail_fwd_mix"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ss_abi_version() == 3
    assert len(_lib.SIGNATURES["ss_tail_fwd_mix"]) == len(_lib.SIGNATURES["ss_tail_fwd_w"]) + 3
    # NULL pairs are refused on the host, before any launch
    assert lib.ss_batch_mixup(None, 4, 4, None, None, None, 16, None, None, 1, 1, None) == -1
    assert lib.ss_batch_plan_mixup(None, None, 1025, 1, 0, 0, 0.5, None, 1024, None, None, None, None, None, None) == -1
