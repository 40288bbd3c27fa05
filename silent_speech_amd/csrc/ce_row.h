// CrossEntropyLoss(weight=, label_smoothing=) of ONE logit row (train_model_official.py:405 and the class-weighted form of
// :406-414): the loss, d(loss)/d(logits) and the arg-max, shared by ce_ls_kernel (pool_head.hip), eval_accum_kernel (eval.hip)
// and the CE block of tail_fwd_kernel (tail.hip) and by their class-weighted entry points.
//
// Row with label y, log-softmax lp, p = exp(lp), smoothing eps, C classes, class weights w:
//   loss      = (1 - eps) * (-w[y] * lp[y]) + (eps / C) * (-sum_c w[c] * lp[c])                      (un-normalised)
//   d logit_c = [ p_c * A - ((c == y) * (1 - eps) * w[y] + (eps / C) * w[c]) ] / denom,  A = w[y] + eps * (sum_k w[k] / C - w[y])
// (A is (1 - eps) * w[y] + (eps / C) * sum_k w[k], written so that w == 1 gives exactly 1).
//
// WEIGHTED = false is the arithmetic the three kernels have always done -- the same operations in the same order, so their
// results keep their bits -- and never touches w.  WEIGHTED = true with every w[c] == 1.0f gives the same bits again: each
// weight enters as a factor of a product whose other factor is the unweighted term (x * 1 and fma(x, 1, s) round like x and
// s + x), sum_k w[k] = C exactly, A = 1 exactly.
//
// MIX = true is the two-label loss of a mixup batch (ss_ce_ls_mix_fwd_bwd, ss_tail_fwd_mix): labels y and yb, one factor lam,
//   loss      = lam * loss(y) + (1 - lam) * loss(yb),
//   d logit_c = [ p_c * A_mix - tgt_mix_c ] / denom,  tgt_mix = lam * tgt(y) + (1 - lam) * tgt(yb),  A_mix the same blend of the As
// (unweighted: A = 1 for both labels, so A_mix = 1 and never enters).  The formulas above still exist once: MIX adds the second
// label's terms and the blend behind them.  MIX = false (the default) is every operation the row has always had, in its order;
// MIX = true with lam == 1 gives those bits again (1 * x + 0 * z is x, fused or not, for finite z).
//
// Two forms, because the callers spread a row differently: ce_row (one thread walks the row) and ce_row_wave (the 64 lanes of a
// wave share it, classes lane, lane + 64, ...).  They differ in the order of their C-term sums, as the kernels always have.
#pragma once
#include "ss_common.h"

// One thread per row.  lr = the row's C logits, 0 <= yy < C (the caller checks).  d_row (may be NULL) gets the gradient row
// divided by denom; *am_out the lowest index among the equal maxima (torch.argmax).  Returns the row's loss, not divided.
// MIX: 0 <= yb < C too, and lam in [0, 1]; without MIX neither is read.
template <bool WEIGHTED, bool MIX = false>
__device__ __forceinline__ float ce_row(const float* __restrict__ lr, int yy, int C, float eps, const float* __restrict__ w,
                                        float denom, float* __restrict__ d_row, int* am_out, int yb = 0, float lam = 1.0f) {
  const float oml = 1.0f - lam;  // (MIX only)
  float m = lr[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (lr[c] > m) { m = lr[c]; am = c; }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(lr[c] - m);
  const float lse = m + logf(se);
  float slp = 0.f, sw = 0.f, wy = 1.f, wyb = 1.f, loss;
  if constexpr (WEIGHTED) {
    wy = w[yy];
    for (int c = 0; c < C; ++c) {
      slp += w[c] * (lr[c] - lse);
      sw += w[c];
    }
    loss = (1.0f - eps) * (wy * (lse - lr[yy])) + eps * (-slp / C);
    if constexpr (MIX) {
      wyb = w[yb];
      const float loss_b = (1.0f - eps) * (wyb * (lse - lr[yb])) + eps * (-slp / C);
      loss = lam * loss + oml * loss_b;
    }
  } else {
    for (int c = 0; c < C; ++c) slp += lr[c] - lse;
    loss = (1.0f - eps) * (lse - lr[yy]) + eps * (-slp / C);
    if constexpr (MIX) {
      const float loss_b = (1.0f - eps) * (lse - lr[yb]) + eps * (-slp / C);
      loss = lam * loss + oml * loss_b;
    }
  }
  if (d_row) {
    if constexpr (WEIGHTED) {
      float a = wy + eps * (sw / C - wy);
      if constexpr (MIX) a = lam * a + oml * (wyb + eps * (sw / C - wyb));
      for (int c = 0; c < C; ++c) {
        float pr = expf(lr[c] - lse);
        float tgt = (c == yy ? (1.0f - eps) * wy : 0.f) + (eps / C) * w[c];
        if constexpr (MIX) tgt = lam * tgt + oml * ((c == yb ? (1.0f - eps) * wyb : 0.f) + (eps / C) * w[c]);
        d_row[c] = (pr * a - tgt) / denom;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        float pr = expf(lr[c] - lse);
        float tgt = (c == yy ? (1.0f - eps) : 0.f) + eps / C;
        if constexpr (MIX) tgt = lam * tgt + oml * ((c == yb ? (1.0f - eps) : 0.f) + eps / C);
        d_row[c] = (pr - tgt) / denom;
      }
    }
  }
  *am_out = am;
  return loss;
}

// One wave per row; every lane of the wave calls it.  lg = the row's C logits (LDS or global), lane = 0..63.  d_row (not NULL)
// gets the gradient row divided by denom.  Returns the row's loss, not divided, and leaves the arg-max in *am_out (both in
// every lane).  MIX as in ce_row.
template <bool WEIGHTED, bool MIX = false>
__device__ __forceinline__ float ce_row_wave(const float* lg, int yy, int C, int lane, float eps, const float* __restrict__ w,
                                             float denom, float* __restrict__ d_row, int* am_out, int yb = 0, float lam = 1.0f) {
  const float oml = 1.0f - lam;  // (MIX only)
  float mx = -3.4e38f;
  int am = 0;
  for (int c = lane; c < C; c += 64)
    if (lg[c] > mx) { mx = lg[c]; am = c; }
  // wave arg-max, first index on ties (torch.argmax)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
  }
  float se = 0.f, sl = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(lg[c] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  float loss;
  if constexpr (WEIGHTED) {
    float sw = 0.f;
    for (int c = lane; c < C; c += 64) {
      sl += w[c] * (lg[c] - lse);
      sw += w[c];
    }
    sl = wave_sum(sl);
    sw = wave_sum(sw);
    const float wy = w[yy];
    float wyb = 1.f;
    float a = wy + eps * (sw / C - wy);
    if constexpr (MIX) {
      wyb = w[yb];
      a = lam * a + oml * (wyb + eps * (sw / C - wyb));
    }
    for (int c = lane; c < C; c += 64) {
      const float pr = expf(lg[c] - lse);
      float tgt = (c == yy ? (1.0f - eps) * wy : 0.f) + (eps / C) * w[c];
      if constexpr (MIX) tgt = lam * tgt + oml * ((c == yb ? (1.0f - eps) * wyb : 0.f) + (eps / C) * w[c]);
      d_row[c] = (pr * a - tgt) / denom;
    }
    loss = (1.0f - eps) * (wy * (lse - lg[yy])) + eps * (-sl / C);
    if constexpr (MIX) {
      const float loss_b = (1.0f - eps) * (wyb * (lse - lg[yb])) + eps * (-sl / C);
      loss = lam * loss + oml * loss_b;
    }
  } else {
    for (int c = lane; c < C; c += 64) sl += lg[c] - lse;
    sl = wave_sum(sl);
    for (int c = lane; c < C; c += 64) {
      const float pr = expf(lg[c] - lse);
      float tgt = (c == yy ? (1.0f - eps) : 0.f) + eps / C;
      if constexpr (MIX) tgt = lam * tgt + oml * ((c == yb ? (1.0f - eps) : 0.f) + eps / C);
      d_row[c] = (pr - tgt) / denom;
    }
    loss = (1.0f - eps) * (lse - lg[yy]) + eps * (-sl / C);
    if constexpr (MIX) {
      const float loss_b = (1.0f - eps) * (lse - lg[yb]) + eps * (-sl / C);
      loss = lam * loss + oml * loss_b;
    }
  }
  *am_out = am;
  return loss;
}
