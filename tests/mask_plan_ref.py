"""CPU restatement of the masking augmentations of the device-planned path (csrc/batch.hip: ss_batch_plan_mask,
ss_batch_mask_apply) in NumPy integers, on top of tests/batch_plan_ref.py (Philox, mulhi and thr come from there).

Row b draws Philox counter (row low, row high, "plan", sub) under key = seed, the planner's own counter.  Sub-draws 0 - 3 are what
ss_batch_plan and ss_batch_plan_aug use them for; the masks take
  sub-draw 4 (m0..m2): time mask decision, width, start
  sub-draw 5 (c0..c3): band decision, width, start; cutout decision
  sub-draw 6 (q0..q3): rectangle width, height, x0, y0
with n = lens[b] (what the planner left) and has_roi = "the row's first ROI map entry is a frame".  Everything is integer
arithmetic, so the kernels are compared exactly.  A maximum of 0 switches its mask off.
"""
import numpy as np

import batch_plan_ref as P

STREAMS = ("both", "features", "roi")
FILLS = ("zero", "hold")
DEFAULTS = dict(time_mask_prob=0.0, time_mask_max=0, time_mask_streams="both", time_mask_fill="zero", feat_mask_prob=0.0,
                feat_mask_max=0, cutout_prob=0.0, cutout_max=(0, 0))


def decisions(n, has_roi, first_row, seed, D, H=0, W=0, augment=True, time_mask_prob=0.0, time_mask_max=0, feat_mask_prob=0.0,
              feat_mask_max=0, cutout_prob=0.0, cutout_max=(0, 0), **_unused):
    """Per row (n: planned lengths, row b draws index first_row + b) -> row_mask (len(n), 8) int32 =
    {t0, tw, col0, cw, x0, y0, rw, rh}; an inactive mask is width 0 at position 0, a row with n = 0 eight zeros."""
    n = np.asarray(n, np.int64)
    has_roi = np.broadcast_to(np.asarray(has_roi, bool), n.shape)
    rows = P._index_range(first_row, len(n))
    m0, m1, m2, _ = P.draw(rows, P.TAG_PLANNER, 4, seed)
    c0, c1, c2, c3 = P.draw(rows, P.TAG_PLANNER, 5, seed)
    q0, q1, q2, q3 = P.draw(rows, P.TAG_PLANNER, 6, seed)
    live = bool(augment) & (n > 0)
    i64 = lambda v: np.asarray(v).astype(np.int64)  # noqa: E731

    timed = live & (n >= 8) & (int(time_mask_max) >= 1) & (m0 < np.uint64(P.thr(time_mask_prob)))
    cap = np.minimum(int(time_mask_max), n // 4)
    tw = 1 + i64(P.mulhi(m1, np.maximum(cap, 0)))
    t0 = 1 + i64(P.mulhi(m2, np.maximum(n - tw, 0)))

    band = live & (int(feat_mask_max) >= 1) & (c0 < np.uint64(P.thr(feat_mask_prob)))
    cw = 1 + i64(P.mulhi(c1, min(int(feat_mask_max), D)))
    col0 = i64(P.mulhi(c2, D - cw + 1))

    mw, mh = int(cutout_max[0]), int(cutout_max[1])
    cut = live & has_roi & (mw >= 1) & (mh >= 1) & (c3 < np.uint64(P.thr(cutout_prob)))
    rw = 1 + i64(P.mulhi(q0, min(mw, W)))
    rh = 1 + i64(P.mulhi(q1, min(mh, H)))
    x0 = i64(P.mulhi(q2, np.maximum(W - rw + 1, 0)))
    y0 = i64(P.mulhi(q3, np.maximum(H - rh + 1, 0)))

    z = np.zeros_like(n)
    cols = [np.where(timed, t0, z), np.where(timed, tw, z), np.where(band, col0, z), np.where(band, cw, z),
            np.where(cut, x0, z), np.where(cut, y0, z), np.where(cut, rw, z), np.where(cut, rh, z)]
    return np.stack(cols, 1).astype(np.int32)


def plan_mask(xmap, nmap, rmap, lens, first_row, seed, D, H=0, W=0, augment=True, **policy):
    """ss_batch_plan_mask on the maps a planner wrote (rmap None: a store without ROI frames) -> (xmap, nmap, rmap, lens,
    row_mask); the inputs are not modified.  ``policy``: the keywords of ``decisions`` plus time_mask_streams / time_mask_fill."""
    pol = dict(DEFAULTS, **policy)
    assert pol["time_mask_streams"] in STREAMS and pol["time_mask_fill"] in FILLS
    xmap, nmap = np.array(xmap, np.int32), np.array(nmap, np.int32)
    rmap = None if rmap is None else np.array(rmap, np.int32)
    lens = np.array(lens, np.int64)
    max_t = xmap.shape[1]
    n = np.clip(lens, 0, max_t)
    has_roi = np.zeros(len(n), bool) if rmap is None else (n > 0) & (rmap[:, 0] >= 0)
    row_mask = decisions(n, has_roi, first_row, seed, D, H, W, augment, **pol)
    feat, roi = pol["time_mask_streams"] != "roi", pol["time_mask_streams"] != "features" and rmap is not None
    hold = pol["time_mask_fill"] == "hold"
    for b in range(len(n)):
        t0, tw = int(row_mask[b, 0]), int(row_mask[b, 1])
        if not tw:
            continue
        run = slice(t0, t0 + tw)
        if feat:
            xmap[b, run] = xmap[b, t0 - 1] if hold else -1
            if not hold:
                nmap[b, run] = -1
        if roi:
            rmap[b, run] = rmap[b, t0 - 1] if hold else -1
    return xmap, nmap, rmap, lens, row_mask


def apply(X, R, rmap, row_mask, fill):
    """ss_batch_mask_apply: X (B, max_t, >= D) f32 or None, R (B, max_t, H, W) u8 or None with rmap (B, max_t) -> copies with the
    band zeroed and the rectangle filled where rmap >= 0.  row_mask is what the planner writes (inside the row and the frame)."""
    X = None if X is None else np.array(X, np.float32)
    R = None if R is None else np.array(R, np.uint8)
    for b, (_, _, col0, cw, x0, y0, rw, rh) in enumerate(np.asarray(row_mask, np.int64)):
        if X is not None and cw:
            X[b, :, col0:col0 + cw] = 0.0
        if R is not None and rw and rh:
            mapped = np.asarray(rmap)[b] >= 0
            R[b, mapped, y0:y0 + rh, x0:x0 + rw] = fill
    return X, R


def policy_kwargs(policy):
    """The mask arguments of a ``silent_speech_amd.AugmentPolicy``."""
    return dict(time_mask_prob=policy.time_mask_prob, time_mask_max=policy.time_mask_max, time_mask_streams=policy.time_mask_streams,
                time_mask_fill=policy.time_mask_fill, feat_mask_prob=policy.feat_mask_prob, feat_mask_max=policy.feat_mask_max,
                cutout_prob=policy.cutout_prob, cutout_max=tuple(policy.cutout_max))
