"""CPU restatement of the augmentation policy of the device-planned path (csrc/batch.hip: ss_batch_plan_aug,
ss_batch_gather_f32_aug, ss_batch_gather_u8_shift) in NumPy integers, on top of tests/batch_plan_ref.py (Philox, mulhi, thr and
the reference's own rules come from there).

Row b draws Philox counter (row low, row high, "plan", sub).  Sub-draws 0 and 1 are what ss_batch_plan uses them for; the policy
takes sub-draw 2 (w0..w3: warp decision, warp factor, scale decision, scale value) and sub-draw 3 (s0..s2: shift decision, dx,
dy).  Everything is integer arithmetic; the scale factor is two float32 operations, each rounded, which NumPy's float32
arithmetic restates exactly.
"""
import numpy as np

import batch_plan_ref as P


def warp_len(T, f_pm):
    """Frames of a clip of T frames warped by f_pm permille."""
    return np.maximum(5, (np.asarray(T, np.int64) * np.asarray(f_pm, np.int64)) // 1000)


def warp_src(j, T, L):
    """Source frame of warped position j: j * (T - 1) // (L - 1); j itself when L == T (also for T = 1)."""
    j, T, L = np.broadcast_arrays(np.asarray(j, np.int64), np.asarray(T, np.int64), np.asarray(L, np.int64))
    same = L == T
    return np.where(same, j, (j * (T - 1)) // np.where(same, 1, np.maximum(L - 1, 1)))


def roi_positions(T, Tr, L):
    """n_r: the warped positions whose source frame exists in a ROI track of Tr frames."""
    T, Tr, L = (np.asarray(v, np.int64) for v in (T, Tr, L))
    short = (Tr * (L - 1) + T - 2) // np.maximum(T - 1, 1)
    return np.where(Tr >= T, L, np.where(Tr <= 0, 0, short))


def decisions(T, has_roi, first_row, seed, augment=True, noise_prob=0.7, drop_prob=0.35, drop_max=2, warp_prob=0.0,
              warp_lo_pm=800, warp_hi_pm=1200, scale_prob=0.0, scale_lo=0.95, scale_span=0.1, shift_prob=0.0, shift_max=(0, 0)):
    """Per row -> dict(noisy, L, k, d0, d1 (positions of the WARPED clip), scale (float32), shift (n, 2) int32, warped)."""
    assert 1 <= drop_max <= 2
    T = np.asarray(T, np.int64)
    has_roi = np.broadcast_to(np.asarray(has_roi, bool), T.shape)
    rows = P._index_range(first_row, len(T))
    r0, r1, r2, r3 = P.draw(rows, P.TAG_PLANNER, 0, seed)
    q0 = P.draw(rows, P.TAG_PLANNER, 1, seed)[0]
    w0, w1, w2, w3 = P.draw(rows, P.TAG_PLANNER, 2, seed)
    s0, s1, s2, _ = P.draw(rows, P.TAG_PLANNER, 3, seed)
    aug = bool(augment)
    noisy = aug & (r0 < np.uint64(P.thr(noise_prob)))
    warped = aug & (T > 10) & (w0 < np.uint64(P.thr(warp_prob)))
    f = warp_lo_pm + P.mulhi(w1, warp_hi_pm - warp_lo_pm + 1).astype(np.int64)
    L = np.where(warped, warp_len(T, f), T)
    drop = aug & (L > 12) & (r1 < np.uint64(P.thr(drop_prob)))
    k = np.where(drop, 1 + P.mulhi(r2, drop_max).astype(np.int64), 0)
    p0 = 1 + P.mulhi(r3, np.maximum(L - 2, 0)).astype(np.int64)
    p1 = 1 + P.mulhi(q0, np.maximum(L - 3, 0)).astype(np.int64)
    p1 = p1 + (p1 >= p0)
    two = k == 2
    d0 = np.where(two, np.minimum(p0, p1), np.where(k == 1, p0, 0))
    d1 = np.where(two, np.maximum(p0, p1), 0)
    scaled = aug & (w2 < np.uint64(P.thr(scale_prob)))
    u = (w3 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)        # 24 bits: exact
    scale = np.where(scaled, np.float32(scale_lo) + np.float32(scale_span) * u, np.float32(1.0)).astype(np.float32)
    shifted = aug & has_roi & (s0 < np.uint64(P.thr(shift_prob)))
    mx, my = int(shift_max[0]), int(shift_max[1])
    dx = P.mulhi(s1, 2 * mx + 1).astype(np.int64) - mx
    dy = P.mulhi(s2, 2 * my + 1).astype(np.int64) - my
    shift = np.where(shifted[:, None], np.stack([dx, dy], 1), 0).astype(np.int32)
    return dict(noisy=noisy, L=L, k=k, d0=d0, d1=d1, scale=scale, shift=shift, warped=warped, f=np.where(warped, f, 1000),
                scaled=scaled, shifted=shifted)


def plan(indices, x_off, x_len, r_off, r_len, y, max_t, augment, first_row=0, seed=0, **policy):
    """ss_batch_plan_aug -> dict(xmap, nmap, rmap (B, max_t) int32, lens, y_out (B,) int64, row_scale (B,) float32, row_shift
    (B, 2) int32, bad, and the decisions).  ``policy``: the keywords of ``decisions``."""
    idx = np.asarray(indices, np.int64)
    n = len(x_len)
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0)
    T = np.asarray(x_len, np.int64)[safe]
    xo = np.asarray(x_off, np.int64)[safe]
    ro = np.full(len(idx), -1, np.int64)
    tr = np.zeros(len(idx), np.int64)
    if r_off is not None:
        ro = np.asarray(r_off, np.int64)[safe]
        tr = np.maximum(np.asarray(r_len, np.int64)[safe], 0)
    has_roi = valid & (ro >= 0)
    dec = decisions(T, has_roi, first_row, seed, augment, **policy)
    L, k, d0, d1 = dec["L"], dec["k"], dec["d0"], dec["d1"]
    t_eff = np.maximum(np.minimum(L - k, max_t), 0)
    t_eff = np.where(has_roi, np.minimum(t_eff, roi_positions(T, tr, L)), t_eff)
    t_eff = np.where(valid, t_eff, 0)
    t = np.arange(max_t, dtype=np.int64)[None, :]
    inside = t < t_eff[:, None]
    s = t + ((k[:, None] >= 1) & (t >= d0[:, None]))
    s = s + ((k[:, None] == 2) & (s >= d1[:, None]))
    xmap = np.where(inside, xo[:, None] + warp_src(s, T[:, None], L[:, None]), -1).astype(np.int32)
    nmap = np.where(inside & dec["noisy"][:, None], 0, -1).astype(np.int32)
    rmap = None
    if r_off is not None:
        rmap = np.where(inside & (ro[:, None] >= 0), ro[:, None] + warp_src(t, T[:, None], L[:, None]), -1).astype(np.int32)
    y_out = np.where(valid, np.asarray(y, np.int64)[safe], 0)
    row_scale = np.where(valid, dec["scale"], np.float32(1.0)).astype(np.float32)
    row_shift = np.where(valid[:, None], dec["shift"], 0).astype(np.int32)
    return dict(xmap=xmap, nmap=nmap, rmap=rmap, lens=t_eff.astype(np.int64), y_out=y_out, row_scale=row_scale,
                row_shift=row_shift, bad=bool((~valid).any()), noisy=dec["noisy"] & valid, k=np.where(valid, k, 0), d0=d0, d1=d1,
                L=L, warped=dec["warped"] & valid)


def policy_kwargs(policy):
    """The planner's arguments of a ``silent_speech_amd.AugmentPolicy``."""
    lo_pm, hi_pm = policy.warp_permille()
    lo, span = policy.scale_lo_span()
    return dict(warp_prob=policy.time_warp_prob, warp_lo_pm=lo_pm, warp_hi_pm=hi_pm, scale_prob=policy.scale_prob, scale_lo=lo,
                scale_span=span, shift_prob=policy.roi_shift_prob, shift_max=tuple(policy.roi_shift_max))


def gather_scaled(store, fmap, row_scale):
    """ss_batch_gather_f32_aug without noise: fl(src * s) per clip, zeros where the map is -1.  fmap (B, max_t)."""
    out = P.gather(np.asarray(store, np.float32), fmap, store.shape[1:])
    return (out * np.asarray(row_scale, np.float32)[:, None, None]).astype(np.float32)


def gather_shifted(store, fmap, row_shift):
    """ss_batch_gather_u8_shift: dst[b][t][y][x] = store[fmap[b][t]][clamp(y - dy)][clamp(x - dx)], zeros where the map is -1.
    store (N, H, W) uint8, fmap (B, max_t), row_shift (B, 2) = (dx, dy) per clip."""
    _, H, W = store.shape
    out = np.zeros(fmap.shape + (H, W), store.dtype)
    for b in range(fmap.shape[0]):
        dx, dy = int(row_shift[b][0]), int(row_shift[b][1])
        ys = np.clip(np.arange(H) - dy, 0, H - 1)
        xs = np.clip(np.arange(W) - dx, 0, W - 1)
        m = fmap[b] >= 0
        out[b][m] = store[fmap[b][m]][:, ys][:, :, xs]
    return out
