"""CPU: the planning scheme of csrc/batch.hip (ss_epoch_sample, ss_batch_plan) as restated in tests/batch_plan_ref.py --
Philox known answers, the reference's per-clip rules (train_model_official.py:143-172) checked exhaustively over small
shapes, the golden plain batch reproduced through the maps, and the distributions of every draw.

The GPU suite (tests/test_gpu_batch_plan.py) compares the kernels with this restatement exactly; this file is what makes the
restatement trustworthy without a GPU."""
import os
import re

import numpy as np
import pytest

import batch_plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567890ABCDEF


def test_philox_known_answers():
    """Random123's kat_vectors for Philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % int(v) for v in P.philox4x32(*ctr, *key)) == want
    # vectorised == one at a time, and the draw index is split into the two low counter words
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 64 - 1], np.uint64)
    vec = P.draw(idx, P.TAG_PLANNER, 1, SEED)
    for n, i in enumerate(idx.tolist()):
        one = P.philox4x32(i & 0xFFFFFFFF, i >> 32, P.TAG_PLANNER, 1, SEED & 0xFFFFFFFF, SEED >> 32)
        assert [int(v[n]) for v in vec] == [int(v) for v in one]
    assert P.thr(0.7) == 3006477107 and P.thr(0.35) == 1503238553 and P.thr(1.0) == 2 ** 32 and P.thr(0.0) == 0
    assert int(P.mulhi(0xFFFFFFFF, 28)) == 27 and int(P.mulhi(0, 28)) == 0


def test_the_library_declares_and_exports_the_two_entry_points():
    """Fails on a tree without the feature: the header, the ctypes table and the built library all carry both symbols."""
    from silent_speech_amd import _lib

    txt = open(os.path.join(ROOT, "include", "ss_hotpath.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in (("ss_epoch_sample", 9), ("ss_batch_plan", 22)):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert len(_lib.SIGNATURES[name]) == n_args
        assert hasattr(_lib.load(), name)
    assert _lib.load().ss_abi_version() == 3  # additive: no version bump
    # argument checks are host code: they answer without a GPU (nothing is launched)
    lib, one = _lib.load(), 1 << 20  # any non-NULL address: refused before it is used
    assert lib.ss_batch_plan(one, 4, one, one, None, None, one, 6, 24, 1, 0, 0, 0.7, 0.35, 3, one, one, None, one, one, one, None) == -3
    assert lib.ss_batch_plan(one, 4, one, one, None, None, one, 6, 24, 1, 0, 0, 1.5, 0.35, 2, one, one, None, one, one, one, None) == -1
    assert lib.ss_batch_plan(one, 4, one, one, one, None, one, 6, 24, 1, 0, 0, 0.7, 0.35, 2, one, one, one, one, one, one, None) == -1
    assert lib.ss_batch_plan(one, 0, one, one, None, None, one, 6, 24, 1, 0, 0, 0.7, 0.35, 2, one, one, None, one, one, one, None) == -1
    assert lib.ss_batch_plan(one, 4, one, one, None, None, one, 6, 24, 1, 0, 0, 0.7, 0.35, 2, one, one, None, one, one, None, None) == -1
    assert lib.ss_epoch_sample(one, 6, one, 0, 0, 10, 0, one, None) == -1
    assert lib.ss_epoch_sample(one, 6, one, 2, 0, 0, 0, one, None) == -1


def test_noise_seed_differs_from_batch_to_batch():
    from silent_speech_amd.device_data import philox_noise_seed

    seeds = [philox_noise_seed(42, r) for r in range(0, 4096 * 16, 16)] + [philox_noise_seed(42, 2 ** 40)]
    assert len(set(seeds)) == len(seeds) and all(0 <= s < 2 ** 64 for s in seeds)
    assert [philox_noise_seed(s, r) for s, r in ((42, 0), (7, 2 ** 33 + 5))] == [P.noise_seed(42, 0), P.noise_seed(7, 2 ** 33 + 5)]
    assert philox_noise_seed(0, 0) == 0x9E3779B97F4A7C15


def _reference_lens(T_kept, Tr, max_t):
    """train_model_official.py:155-172: clip_pad_trim, then T_use = min(T_eff, Tr, max_t) for a clip with ROI frames."""
    t_eff = min(T_kept, max_t)
    return t_eff if Tr is None else min(t_eff, Tr, max_t)


@pytest.mark.parametrize("max_t", [8, 30])
def test_rules_hold_for_every_small_shape(max_t):
    """T in [1, 40] x r_len in {none, 0, T-3, T, T+3} x 3000 draw indices each, augmentation on and off."""
    n_rows, first = 3000, 2 ** 32 - 1500  # the rows straddle the 32-bit boundary of the draw index
    dropped_somewhere = 0
    for T in range(1, 41):
        for Tr in (None, 0, T - 3, T, T + 3):  # None: the clip has no "roi" array; 0: it has an empty one
            if Tr is not None and Tr < 0:
                continue
            # three clips in the store, the middle one under test: offsets are not zero
            x_off, x_len, r_off, r_len = P.store_tables([(5, 5), (T, Tr), (7, None)])
            y = [3, 1, 4]
            for augment in (True, False):
                pl = P.plan(np.ones(n_rows, np.int64), x_off, x_len, r_off, r_len, y, max_t, augment, first, SEED)
                xmap, nmap, rmap, lens, k = pl["xmap"], pl["nmap"], pl["rmap"], pl["lens"], pl["k"]
                assert not pl["bad"] and np.all(pl["y_out"] == 1)
                want = np.array([_reference_lens(T - kk, Tr, max_t) for kk in k])
                assert np.array_equal(lens, want)
                inside = np.arange(max_t)[None, :] < lens[:, None]
                assert np.all(xmap[~inside] == -1) and np.all(nmap[~inside] == -1) and np.all(rmap[~inside] == -1)
                src = xmap - x_off[1]
                assert np.all(src[inside] >= 0) and np.all(src[inside] < T)                      # inside the clip
                assert np.all((np.diff(src, axis=1) > 0)[inside[:, 1:]])                        # strictly increasing
                if T <= 12 or not augment:
                    assert not k.any() and np.array_equal(src[inside], np.broadcast_to(np.arange(max_t), src.shape)[inside])
                if not augment:
                    assert np.all(nmap == -1)
                # frames 0 and T-1 are never dropped; the dropped ones are exactly the d0 / d1 reported
                d0, d1 = pl["d0"], pl["d1"]
                assert np.all(d0[k >= 1] >= 1) and np.all(d0[k >= 1] <= T - 2)
                assert np.all(d1[k == 2] > d0[k == 2]) and np.all(d1[k == 2] <= T - 2)
                full = P.plan(np.ones(n_rows, np.int64), x_off, x_len, None, None, y, 64, augment, first, SEED)
                fsrc = full["xmap"] - x_off[1]
                for b in np.flatnonzero(k)[:50]:
                    kept = fsrc[b, :full["lens"][b]].tolist()
                    gone = sorted(set(range(T)) - set(kept))
                    assert gone == ([d0[b]] if k[b] == 1 else [d0[b], d1[b]]) and kept[0] == 0 and kept[-1] == T - 1
                # noise rows: all of the row or none of it; ROI rows are never dropped
                assert np.all((nmap == 0) == (inside & pl["noisy"][:, None]))
                if Tr is None:
                    assert np.all(rmap == -1)
                else:
                    assert np.array_equal(rmap[inside], (r_off[1] + np.broadcast_to(np.arange(max_t), rmap.shape))[inside])
                    assert rmap.max() < r_off[1] + Tr
                dropped_somewhere += int(k.sum())
    assert dropped_somewhere > 0


def test_out_of_range_indices_give_empty_rows_and_are_reported():
    x_off, x_len, r_off, r_len = P.store_tables([(20, 20), (15, None)])
    pl = P.plan([0, 2, -1, 1, 2 ** 31 - 1], x_off, x_len, r_off, r_len, [5, 6], 16, True, 0, SEED)
    assert pl["bad"] and pl["lens"].tolist()[1:3] == [0, 0] and pl["lens"][4] == 0 and pl["lens"][0] > 0 and pl["lens"][3] > 0
    for b in (1, 2, 4):
        assert np.all(pl["xmap"][b] == -1) and np.all(pl["nmap"][b] == -1) and np.all(pl["rmap"][b] == -1) and pl["y_out"][b] == 0
    assert pl["y_out"][[0, 3]].tolist() == [5, 6]
    assert not P.plan([0, 1], x_off, x_len, r_off, r_len, [5, 6], 16, True, 0, SEED)["bad"]


def test_maps_reproduce_the_reference_plain_batch(golden_dir):
    """The maps applied with NumPy indexing to the six golden clips (clip4 has no ROI frames) == what the reference's own
    NPZWordDataset(augment=False) + collate_fn produced, bit for bit."""
    d = np.load(os.path.join(golden_dir, "dataset.npz"), allow_pickle=True)
    n, max_t = int(d["n_clips"]), int(d["max_t"])
    rois = [d[f"clip{k}::roi"] if f"clip{k}::roi" in d.files else None for k in range(n)]
    assert rois[4] is None and sum(r is not None for r in rois) == 5
    clips = [(len(d[f"clip{k}::X"]), None if rois[k] is None else len(rois[k])) for k in range(n)]
    x_off, x_len, r_off, r_len = P.store_tables(clips)
    Xs = np.concatenate([d[f"clip{k}::X"] for k in range(n)], 0)
    Rs = np.concatenate([r for r in rois if r is not None], 0)
    y = [{"no": 0, "yes": 1}[str(d[f"clip{k}::label"])] for k in range(n)]
    pl = P.plan(np.arange(n), x_off, x_len, r_off, r_len, y, max_t, False, 12345, SEED)
    assert np.array_equal(P.gather(Xs, pl["xmap"], Xs.shape[1:]), d["plain::X"])
    assert np.array_equal(P.gather(Rs, pl["rmap"], Rs.shape[1:]), d["plain::R"])
    assert np.array_equal(pl["lens"], d["plain::T"]) and np.array_equal(pl["y_out"], d["plain::y"])
    assert np.all(pl["nmap"] == -1)


# ---------------------------------------------------------------------------------------------- distributions
# Bounds: five binomial standard deviations of the stated probability at the stated number of draws -- derived from the
# scheme, not from what it gave.  For the record, seed 0x1234567890abcdef gives P(noise) 0.7049, P(drop) 0.3541,
# P(k=2 | drop) 0.5032, class counts 3897 - 4120.
N_DRAWS = 20000


def _sigma(p, n):
    return np.sqrt(p * (1 - p) / n)


def test_augmentation_draws_have_the_reference_distributions():
    T = 30
    noisy, k, d0, d1 = P.decisions(np.full(N_DRAWS, T), 0, SEED)
    assert abs(noisy.mean() - 0.7) < 5 * _sigma(0.7, N_DRAWS) < 0.0163               # 0.7 +- 0.0162
    drop = k > 0
    assert abs(drop.mean() - 0.35) < 5 * _sigma(0.35, N_DRAWS) < 0.0169              # 0.35 +- 0.0169
    n_drops = int(drop.sum())
    assert abs((k == 2).sum() / n_drops - 0.5) < 5 * np.sqrt(0.25 / n_drops)
    # every interior position is dropped equally often (a frame of a pair counts once per frame)
    pos = np.concatenate([d0[k >= 1], d1[k == 2]])
    assert pos.min() == 1 and pos.max() == T - 2
    n_dropped, p = len(pos), 1.0 / (T - 2)
    counts = np.bincount(pos, minlength=T)[1:T - 1]
    assert np.all(np.abs(counts - n_dropped * p) < 5 * np.sqrt(n_dropped * p * (1 - p))), counts
    # pairs: the two frames are distinct, and every unordered pair is possible (uniform over pairs: the smaller one of a
    # uniform pair is position j with probability (T - 2 - j) / C(T-2, 2))
    two = k == 2
    assert np.all(d0[two] < d1[two])
    n2, n_pairs = int(two.sum()), (T - 2) * (T - 3) // 2
    for j in (1, 10, 20):
        pj = (T - 2 - j) / n_pairs
        assert abs((d0[two] == j).sum() - n2 * pj) < 5 * np.sqrt(n2 * pj * (1 - pj))
    # noise and drop are independent draws
    both = (noisy & drop).mean()
    assert abs(both - 0.7 * 0.35) < 5 * _sigma(0.7 * 0.35, N_DRAWS)
    # a short clip is never dropped from; without augmentation nothing is drawn
    assert not P.decisions(np.full(N_DRAWS, 12), 0, SEED)[1].any()
    assert not any(v.any() for v in P.decisions(np.full(100, T), 0, SEED, augment=False)[:2])
    # another seed or another first row: another stream
    assert not np.array_equal(noisy, P.decisions(np.full(N_DRAWS, T), 0, SEED + 1)[0])
    assert np.array_equal(noisy[5:], P.decisions(np.full(N_DRAWS - 5, T), 5, SEED)[0])


def test_sampler_is_class_balanced_and_uniform_inside_a_class():
    sizes = [50, 5, 1, 20, 124]
    rng = np.random.default_rng(0)
    labels = rng.permutation(np.repeat([0, 2, 3, 5, 9], sizes))  # class ids with gaps: absent classes are left out
    members, class_start = P.class_tables(labels)
    assert class_start.tolist() == [0, 50, 55, 56, 76, 200] and sorted(members.tolist()) == list(range(200))
    for c, (lo, hi) in zip([0, 2, 3, 5, 9], zip(class_start[:-1], class_start[1:])):
        assert np.all(labels[members[lo:hi]] == c)
    idx = P.sample_epoch(members, class_start, 0, N_DRAWS, SEED)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 200
    per_class = np.array([(labels[idx] == c).sum() for c in [0, 2, 3, 5, 9]])
    assert np.all(np.abs(per_class - 4000) < 5 * np.sqrt(N_DRAWS * 0.2 * 0.8)), per_class   # 4000 +- 283
    for c, size in zip([0, 2, 3, 5, 9], sizes):
        drawn = idx[labels[idx] == c]
        cnt = np.bincount(drawn, minlength=200)[np.flatnonzero(labels == c)]
        p = 1.0 / size
        assert np.all(np.abs(cnt - len(drawn) * p) <= 5 * np.sqrt(len(drawn) * p * (1 - p))), (c, cnt)
    # `first` addresses the same epoch: a rank's shard is a slice of the whole draw, also across the 32-bit boundary
    whole = P.sample_epoch(members, class_start, 2 ** 32 - 100, 300, SEED)
    assert np.array_equal(P.sample_epoch(members, class_start, 2 ** 32 - 100 + 120, 180, SEED), whole[120:])
    assert not np.array_equal(P.sample_epoch(members, class_start, 0, 300, SEED + 1), idx[:300])
