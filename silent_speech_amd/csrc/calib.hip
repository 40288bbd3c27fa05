// Post-hoc temperature scaling kept on the device: the fit of one scalar on the validation logits (ss_calib_moments +
// ss_calib_bisect, 35 enqueue-only pairs, nothing read back), the reliability bins and the rank histogram of the true class
// (ss_calib_bins) and the tempered form of the serving softmax (ss_softmax_topk_t).  DESIGN.md section "Calibrated confidences".
//
// Parametrised by the inverse temperature u = 1 / T.  Row with logits z (C floats), label y, m = max z:
//   e_c = exp(u (z_c - m)),  S0 = sum e_c,  S1 = sum e_c (z_c - m)
//   nll = log S0 - u (z_y - m)              g = d nll / du = S1 / S0 - (z_y - m)
// sum nll is convex in u, so sum g is non-decreasing in u and its sign brackets the optimum.
// No float atomics anywhere in this file: a fit gives the same bits on every run.
#include "ss_common.h"
#include "ce_row.h"
#include "topk_row.h"

namespace {

// state of a fit: doubles, in this order (include/ss_hotpath.h)
enum { ST_U, ST_LO, ST_HI, ST_NLL, ST_G, ST_NLL1, ST_ITER, ST_BOUND };
constexpr double CALIB_U_MIN = SS_CALIB_U_MIN, CALIB_U_MAX = SS_CALIB_U_MAX;

// One wave per row (classes lane, lane + 64, ...: any C), rows wave, wave + 4 * workgroups, ... in order.  Per-row arithmetic in
// float32, the sums over rows in float64: a wave adds its rows in the order it walks them, the four waves of a workgroup combine
// in a fixed tree, and every workgroup writes its own slot -- the partials are a pure function of (logits, y, u, grid).
__global__ __launch_bounds__(256) void calib_moments_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y, int N,
                                                            int C, const double* __restrict__ state,
                                                            double* __restrict__ partials, int* __restrict__ err_flag) {
  __shared__ double red[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float u = (float)state[ST_U];
  double s_nll = 0.0, s_g = 0.0;
  for (long r = (long)blockIdx.x * 4 + wave; r < N; r += (long)gridDim.x * 4) {  // (r is wave-uniform: whole waves walk together)
    const int64_t label = y[r];
    if (!ce_label_ok(label, C)) {  // never an index: the row counts nowhere (the rule of eval_accum_kernel)
      if (lane == 0) *err_flag = 1;
      continue;
    }
    const float* z = logits + r * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
    m = wave_max(m);
    float s0 = 0.f, s1 = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float d = z[c] - m, e = expf(u * d);
      s0 += e;
      s1 += e * d;
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    const float dy = z[label] - m;
    s_nll += (double)(logf(s0) - u * dy);
    s_g += (double)(s1 / s0 - dy);
  }
  if (lane == 0) {
    red[wave][0] = s_nll;
    red[wave][1] = s_g;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    partials[2 * (long)blockIdx.x + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// sum over the 64 lanes by a fixed butterfly: the same bits in every lane and on every run
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave: the partials summed in slot order (lane l adds slots l, l + 64, ...), then one step of the fixed schedule
// (include/ss_hotpath.h).  The state's u is always the point the NEXT ss_calib_moments evaluates -- except after the last
// iteration, where it stays the point just evaluated, so that nll and g are those of the u the fit returns.
__global__ __launch_bounds__(64) void calib_bisect_kernel(double* __restrict__ state, const double* __restrict__ partials, int n) {
  const int lane = threadIdx.x;
  double nll = 0.0, g = 0.0;
  for (int i = lane; i < n; i += 64) {
    nll += partials[2 * i];
    g += partials[2 * i + 1];
  }
  nll = wave_sum_f64(nll);
  g = wave_sum_f64(g);
  if (lane != 0) return;
  const int it = (int)state[ST_ITER];
  if (state[ST_BOUND] != 0.0 || it >= SS_CALIB_FIT_ITERS) return;  // pinned to a bound, or finished: the state is left alone
  const double u = state[ST_U];
  double lo = state[ST_LO], hi = state[ST_HI], next = u;
  state[ST_NLL] = nll;
  state[ST_G] = g;
  if (it == 0) {  // u == 1
    state[ST_NLL1] = nll;
    lo = CALIB_U_MIN;
    hi = CALIB_U_MAX;
    next = CALIB_U_MIN;
  } else if (it == 1) {  // u == U_MIN: a gradient that is not negative there puts the optimum at or below it
    if (g >= 0.0) state[ST_BOUND] = -1.0;
    else next = CALIB_U_MAX;
  } else if (it == 2) {  // u == U_MAX
    if (g <= 0.0) state[ST_BOUND] = 1.0;
    else next = sqrt(lo * hi);
  } else {
    if (g > 0.0) hi = u;
    else lo = u;
    if (it + 1 < SS_CALIB_FIT_ITERS) next = sqrt(lo * hi);
  }
  state[ST_U] = next;
  state[ST_LO] = lo;
  state[ST_HI] = hi;
  state[ST_ITER] = (double)(it + 1);
}

// One wave per row, rows by grid stride.  Integer atomics only: the sums do not depend on the order.
__global__ __launch_bounds__(256) void calib_bins_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y, int N, int C,
                                                         const float* __restrict__ inv_temp, int n_bins, int k_max,
                                                         int* __restrict__ bin_count, int* __restrict__ bin_hits,
                                                         unsigned long long* __restrict__ bin_conf_fx, int* __restrict__ rank_hist,
                                                         int* __restrict__ err_flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float u = inv_temp ? inv_temp[0] : 1.0f;
  for (long r = (long)blockIdx.x * 4 + wave; r < N; r += (long)gridDim.x * 4) {
    const int64_t label = y[r];
    if (!ce_label_ok(label, C)) {
      if (lane == 0) *err_flag = 1;
      continue;
    }
    const int yy = (int)label;
    const float* z = logits + r * C;
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < C; c += 64)
      if (z[c] > m) { m = z[c]; am = c; }
    // wave arg-max, lowest index among equal maxima (ce_row, torch.argmax)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
    if (am == 0x7fffffff) am = 0;  // (no logit above -inf: class 0, as ce_row answers)
    const float zy = z[yy];
    float s0 = 0.f;
    unsigned above = 0;
    for (int c = lane; c < C; c += 64) {
      s0 += expf(u * (z[c] - m));
      above += (z[c] > zy || (z[c] == zy && c < yy)) ? 1u : 0u;
    }
    s0 = wave_sum(s0);
    above = wave_sum_u32(above);
    if (lane == 0) {
      const float conf = 1.0f / s0;  // the largest class has exponent 0
      int bin = (int)floorf(conf * (float)n_bins);
      bin = bin < 0 ? 0 : (bin > n_bins - 1 ? n_bins - 1 : bin);
      atomicAdd(&bin_count[bin], 1);
      if (am == yy) atomicAdd(&bin_hits[bin], 1);
      atomicAdd(&bin_conf_fx[bin], (unsigned long long)llrint((double)conf * 4294967296.0));
      atomicAdd(&rank_hist[above < (unsigned)k_max ? (int)above : k_max], 1);
    }
  }
}

__global__ __launch_bounds__(256) void softmax_topk_t_kernel(const float* __restrict__ logits, int B, int C, int k,
                                                             const float* __restrict__ inv_temp, float* __restrict__ probs,
                                                             int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave together
  const float u = inv_temp ? inv_temp[0] : 1.0f;
  softmax_topk_row<true>(logits + (long)b * C, C, k, u, lane, probs + (long)b * k, idx + (long)b * k);
}

// workgroups of a row-per-wave grid-stride launch: four rows each, at least one, at most `cap`
inline int calib_grid(int N, int cap) {
  const long blocks = ((long)N + 3) / 4;
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

}  // namespace

extern "C" int ss_calib_moments(const float* logits, const int64_t* y, int N, int C, const double* state, double* partials,
                                int n_partials, int32_t* err_flag, ss_stream_t stream) {
  SS_REQUIRE(logits && y && state && partials && err_flag && N > 0, SS_ERR_ARG);
  SS_REQUIRE(C >= 2, SS_ERR_ARG);  // with one class g is identically zero
  SS_REQUIRE(n_partials >= 1 && n_partials <= SS_CALIB_MAX_PARTIALS, SS_ERR_ARG);
  // every slot is written, by its own workgroup; a workgroup without rows writes zeros
  hipLaunchKernelGGL(calib_moments_kernel, dim3(n_partials), dim3(256), 0, static_cast<hipStream_t>(stream), logits, y, N, C, state,
                     partials, err_flag);
  return ss_launch_status();
}

extern "C" int ss_calib_bisect(double* state, const double* partials, int n_partials, ss_stream_t stream) {
  SS_REQUIRE(state && partials, SS_ERR_ARG);
  SS_REQUIRE(n_partials >= 1 && n_partials <= SS_CALIB_MAX_PARTIALS, SS_ERR_ARG);
  hipLaunchKernelGGL(calib_bisect_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, partials, n_partials);
  return ss_launch_status();
}

extern "C" int ss_calib_bins(const float* logits, const int64_t* y, int N, int C, const float* inv_temp, int n_bins, int k_max,
                             int32_t* bin_count, int32_t* bin_hits, uint64_t* bin_conf_fx, int32_t* rank_hist, int32_t* err_flag,
                             ss_stream_t stream) {
  SS_REQUIRE(logits && y && bin_count && bin_hits && bin_conf_fx && rank_hist && err_flag && N > 0 && C > 0, SS_ERR_ARG);
  SS_REQUIRE(n_bins >= 1 && n_bins <= 64 && k_max >= 1 && k_max <= 64, SS_ERR_ARG);
  hipLaunchKernelGGL(calib_bins_kernel, dim3(calib_grid(N, 1024)), dim3(256), 0, static_cast<hipStream_t>(stream), logits, y, N, C,
                     inv_temp, n_bins, k_max, bin_count, bin_hits, reinterpret_cast<unsigned long long*>(bin_conf_fx), rank_hist,
                     err_flag);
  return ss_launch_status();
}

extern "C" int ss_softmax_topk_t(const float* logits, int B, int C, int k, const float* inv_temp, float* probs, int32_t* idx,
                                 ss_stream_t stream) {
  SS_REQUIRE(logits && probs && idx && B > 0 && C > 0 && k > 0, SS_ERR_ARG);
  SS_REQUIRE(k <= 64, SS_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(softmax_topk_t_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), logits, B, C, k,
                     inv_temp, probs, idx);
  return ss_launch_status();
}
