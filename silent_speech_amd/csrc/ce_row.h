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
// Two forms, because the callers spread a row differently: ce_row (one thread walks the row) and ce_row_wave (the 64 lanes of a
// wave share it, classes lane, lane + 64, ...).  They differ in the order of their C-term sums, as the kernels always have.
#pragma once
#include "ss_common.h"

// One thread per row.  lr = the row's C logits, 0 <= yy < C (the caller checks).  d_row (may be NULL) gets the gradient row
// divided by denom; *am_out the lowest index among the equal maxima (torch.argmax).  Returns the row's loss, not divided.
template <bool WEIGHTED>
__device__ __forceinline__ float ce_row(const float* __restrict__ lr, int yy, int C, float eps, const float* __restrict__ w,
                                        float denom, float* __restrict__ d_row, int* am_out) {
  float m = lr[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (lr[c] > m) { m = lr[c]; am = c; }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(lr[c] - m);
  const float lse = m + logf(se);
  float slp = 0.f, sw = 0.f, wy = 1.f, loss;
  if constexpr (WEIGHTED) {
    wy = w[yy];
    for (int c = 0; c < C; ++c) {
      slp += w[c] * (lr[c] - lse);
      sw += w[c];
    }
    loss = (1.0f - eps) * (wy * (lse - lr[yy])) + eps * (-slp / C);
  } else {
    for (int c = 0; c < C; ++c) slp += lr[c] - lse;
    loss = (1.0f - eps) * (lse - lr[yy]) + eps * (-slp / C);
  }
  if (d_row) {
    if constexpr (WEIGHTED) {
      const float a = wy + eps * (sw / C - wy);
      for (int c = 0; c < C; ++c) {
        float pr = expf(lr[c] - lse);
        float tgt = (c == yy ? (1.0f - eps) * wy : 0.f) + (eps / C) * w[c];
        d_row[c] = (pr * a - tgt) / denom;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        float pr = expf(lr[c] - lse);
        float tgt = (c == yy ? (1.0f - eps) : 0.f) + eps / C;
        d_row[c] = (pr - tgt) / denom;
      }
    }
  }
  *am_out = am;
  return loss;
}

// One wave per row; every lane of the wave calls it.  lg = the row's C logits (LDS or global), lane = 0..63.  d_row (not NULL)
// gets the gradient row divided by denom.  Returns the row's loss, not divided, and leaves the arg-max in *am_out (both in
// every lane).
template <bool WEIGHTED>
__device__ __forceinline__ float ce_row_wave(const float* lg, int yy, int C, int lane, float eps, const float* __restrict__ w,
                                             float denom, float* __restrict__ d_row, int* am_out) {
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
    const float a = wy + eps * (sw / C - wy);
    for (int c = lane; c < C; c += 64) {
      const float pr = expf(lg[c] - lse);
      const float tgt = (c == yy ? (1.0f - eps) * wy : 0.f) + (eps / C) * w[c];
      d_row[c] = (pr * a - tgt) / denom;
    }
    loss = (1.0f - eps) * (wy * (lse - lg[yy])) + eps * (-sl / C);
  } else {
    for (int c = lane; c < C; c += 64) sl += lg[c] - lse;
    sl = wave_sum(sl);
    for (int c = lane; c < C; c += 64) {
      const float pr = expf(lg[c] - lse);
      const float tgt = (c == yy ? (1.0f - eps) : 0.f) + eps / C;
      d_row[c] = (pr - tgt) / denom;
    }
    loss = (1.0f - eps) * (lse - lg[yy]) + eps * (-sl / C);
  }
  *am_out = am;
  return loss;
}
