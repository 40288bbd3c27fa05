// softmax + top-k of ONE logit row by one wave (live_infer_official.py:223-226), shared by softmax_topk_kernel (pool_head.hip) and
// softmax_topk_t_kernel (calib.hip): probabilities as exp(l - max) / sum like torch.softmax, k selection sweeps (largest first,
// lowest index among equals).
// TEMPERED = false is the arithmetic ss_softmax_topk has always done (u is not read).  TEMPERED = true takes the softmax of u * l,
// u > 0 the inverse temperature: every exponent is u * (l - max), and since 1.0f * x is exact, u == 1.0f gives the bits of
// TEMPERED = false.  The order of the classes does not depend on u, so the indices never do.
#pragma once
#include "ss_common.h"

template <bool TEMPERED>
__device__ __forceinline__ float topk_exponent(float d, float u) {
  if constexpr (TEMPERED) return u * d;
  else return d;
}

// every lane of the wave calls it; lane 0 writes probs_row[0..k) and idx_row[0..k)
template <bool TEMPERED>
__device__ __forceinline__ void softmax_topk_row(const float* __restrict__ lr, int C, int k, float u, int lane,
                                                 float* __restrict__ probs_row, int32_t* __restrict__ idx_row) {
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, lr[c]);
  m = wave_max(m);
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(topk_exponent<TEMPERED>(lr[c] - m, u));
  se = wave_sum(se);
  float last_v = INFINITY;
  int last_i = -1;
  for (int j = 0; j < k; ++j) {
    // best entry that comes after (last_v, last_i) in the order "value descending, index ascending"
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = lr[c];
      const bool after = v < last_v || (v == last_v && c > last_i);
      if (after && (v > bv || (v == bv && c < bi))) { bv = v; bi = c; }
    }
    const float wv = wave_max(bv);
    int cand = (bv == wv) ? bi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    last_v = wv;
    last_i = cand;
    if (lane == 0) {
      const bool have = cand != 0x7fffffff;
      probs_row[j] = have ? expf(topk_exponent<TEMPERED>(wv - m, u)) / se : 0.f;
      idx_row[j] = have ? cand : -1;
    }
  }
}
