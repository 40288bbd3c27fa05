"""CPU restatement of the device-side batch planning (csrc/batch.hip: ss_epoch_sample, ss_batch_plan) in NumPy integers.

Everything the kernels decide is integer arithmetic on Philox4x32-10 outputs, so this file is bit-equal to them by
construction of the scheme, not by tolerance:

  counter = (draw index low, draw index high, domain tag, sub-draw number), key = (seed low, seed high)
  mulhi(r, n) = (r * n) >> 32        a uniform integer below n
  thr(p)      = int(p * 2**32)       computed in double; an event of probability p is ``r < thr(p)``

The functions are vectorised over the draw index (arrays of uint64 holding 32-bit words); scalars work too.
"""
import numpy as np

TAG_NOISE, TAG_SAMPLER, TAG_PLANNER = 0x6E6F6973, 0x73616D70, 0x706C616E
M32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 (Salmon et al., SC'11; Random123): 4 counter words, 2 key words -> 4 output words, as uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & M32 for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(rounds):
        p0 = np.uint64(0xD2511F53) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def draw(index, tag, sub, seed):
    """The four words of sub-draw ``sub`` of draw ``index`` (64-bit, wraps) in the stream ``tag`` of ``seed``."""
    index = np.asarray(index, np.uint64)
    seed = int(seed) & MASK64
    return philox4x32(index & M32, index >> np.uint64(32), tag, sub, seed & 0xFFFFFFFF, seed >> 32)


def mulhi(r, n):
    return (np.asarray(r, np.uint64) * np.asarray(n, np.uint64)) >> np.uint64(32)


def thr(p):
    return int(float(p) * 4294967296.0)


def _index_range(first, count):
    with np.errstate(over="ignore"):
        return np.uint64(int(first) & MASK64) + np.arange(count, dtype=np.uint64)  # wraps modulo 2^64 like the kernel


def noise_seed(seed, first_row):
    """The seed ``DeviceClipStore.batch(rng="philox")`` hands to the gather's noise stream: distinct per batch."""
    return (int(seed) ^ (((int(first_row) + 1) * 0x9E3779B97F4A7C15) & MASK64)) & MASK64


# ---------------------------------------------------------------------------------------------- sampler
def class_tables(labels):
    """Clip ids grouped by class (classes in ascending id, ids ascending inside a class; absent classes left out)."""
    labels = np.asarray(labels)
    present = np.unique(labels)
    members = np.concatenate([np.flatnonzero(labels == c) for c in present]).astype(np.int32)
    sizes = [int((labels == c).sum()) for c in present]
    return members, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def sample_epoch(members, class_start, first, count, seed):
    """WeightedRandomSampler(1 / count(label), replacement=True): a uniform class, then a uniform member of it."""
    members, class_start = np.asarray(members, np.int64), np.asarray(class_start, np.int64)
    r0, r1, _, _ = draw(_index_range(first, count), TAG_SAMPLER, 0, seed)
    cls = mulhi(r0, len(class_start) - 1).astype(np.int64)
    size = class_start[cls + 1] - class_start[cls]
    return members[class_start[cls] + mulhi(r1, size).astype(np.int64)].astype(np.int32)


# ---------------------------------------------------------------------------------------------- planner
def decisions(T, first_row, seed, augment=True, noise_prob=0.7, drop_prob=0.35, drop_max=2):
    """Per row (T: array of clip lengths, row b draws index first_row + b) -> noisy (bool), k (0..2 frames dropped),
    d0 < d1 (the dropped source frames, ascending; 0 where unused)."""
    assert 1 <= drop_max <= 2
    T = np.asarray(T, np.int64)
    rows = _index_range(first_row, len(T))
    r0, r1, r2, r3 = draw(rows, TAG_PLANNER, 0, seed)
    q0 = draw(rows, TAG_PLANNER, 1, seed)[0]
    aug = bool(augment)
    noisy = aug & (r0 < np.uint64(thr(noise_prob)))
    drop = aug & (T > 12) & (r1 < np.uint64(thr(drop_prob)))
    k = np.where(drop, 1 + mulhi(r2, drop_max).astype(np.int64), 0)
    p0 = 1 + mulhi(r3, np.maximum(T - 2, 0)).astype(np.int64)
    p1 = 1 + mulhi(q0, np.maximum(T - 3, 0)).astype(np.int64)
    p1 = p1 + (p1 >= p0)
    two = k == 2
    d0 = np.where(two, np.minimum(p0, p1), np.where(k == 1, p0, 0))
    d1 = np.where(two, np.maximum(p0, p1), 0)
    return noisy, k, d0, d1


def plan(indices, x_off, x_len, r_off, r_len, y, max_t, augment, first_row=0, seed=0, noise_prob=0.7, drop_prob=0.35,
         drop_max=2):
    """ss_batch_plan.  ``r_off`` / ``r_len`` None: a store without ROI frames (rmap is None).  -> dict(xmap, nmap, rmap
    (B, max_t) int32, lens, y_out (B,) int64, bad (bool: some index was outside the store), noisy, k, d0, d1)."""
    idx = np.asarray(indices, np.int64)
    n = len(x_len)
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0)
    T = np.asarray(x_len, np.int64)[safe]
    xo = np.asarray(x_off, np.int64)[safe]
    noisy, k, d0, d1 = decisions(T, first_row, seed, augment, noise_prob, drop_prob, drop_max)
    t_eff = np.maximum(np.minimum(T - k, max_t), 0)
    ro = np.full(len(idx), -1, np.int64)
    if r_off is not None:
        ro = np.asarray(r_off, np.int64)[safe]
        tr = np.maximum(np.asarray(r_len, np.int64)[safe], 0)
        t_eff = np.where(ro >= 0, np.minimum(t_eff, tr), t_eff)
    t_eff = np.where(valid, t_eff, 0)
    t = np.arange(max_t, dtype=np.int64)[None, :]
    inside = t < t_eff[:, None]
    s = t + ((k[:, None] >= 1) & (t >= d0[:, None]))
    s = s + ((k[:, None] == 2) & (s >= d1[:, None]))
    xmap = np.where(inside, xo[:, None] + s, -1).astype(np.int32)
    nmap = np.where(inside & noisy[:, None], 0, -1).astype(np.int32)
    rmap = None
    if r_off is not None:
        rmap = np.where(inside & (ro[:, None] >= 0), ro[:, None] + t, -1).astype(np.int32)
    y_out = np.where(valid, np.asarray(y, np.int64)[safe], 0)
    return dict(xmap=xmap, nmap=nmap, rmap=rmap, lens=t_eff.astype(np.int64), y_out=y_out, bad=bool((~valid).any()),
                noisy=noisy & valid, k=np.where(valid, k, 0), d0=d0, d1=d1)


def store_tables(clips):
    """Ragged-store tables of a list of (T, Tr or None) clips, laid out as DeviceClipStore does."""
    x_off, x_len, r_off, r_len = [], [], [], []
    xo = ro = 0
    for T, Tr in clips:
        x_off.append(xo)
        x_len.append(T)
        xo += T
        if Tr is None:
            r_off.append(-1)
            r_len.append(0)
        else:
            r_off.append(ro)
            r_len.append(Tr)
            ro += Tr
    return x_off, x_len, r_off, r_len


def gather(store, fmap, width_shape):
    """rows of ``store`` by a frame map, zeros where the map is -1 (what ss_batch_gather_* do without noise)."""
    out = np.zeros(fmap.shape + tuple(width_shape), store.dtype)
    m = fmap >= 0
    out[m] = store[fmap[m]]
    return out
