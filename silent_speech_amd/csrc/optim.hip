// Flat-bucket optimiser step: the gradient's sum of squares, the global-norm clip folded into Adam (plain, with the weight average,
// and grouped AdamW), the swap of two buckets, the two streams of a sharpness-aware step (perturb; restore + sum of squares), and
// the layer-wise adaptive step LAMB (moments + per-segment norms; apply).
// Replaces clip_grad_norm_ + torch.optim.Adam.step of train_model_official.py:403, 438-439.  All HBM-bound, grid-stride; every
// kernel but adam_clip_kernel in 16-byte lanes.
#include <math.h>

#include "ss_common.h"

namespace {

// The terms whose squares the sums below take: the elements of x themselves, or |w| g (the scale-invariant norm of ASAM; the
// product is rounded on its own, then squared).  In two halves, so that the walk can issue all loads of a trip before anything
// else: load<T>(i) reads item i (T = f32x4: floats [4i, 4i + 4); T = float: element i), term(i, raw) makes the term of it.
template <class T>
__device__ __forceinline__ T abs_times(const T& w, const T& g);
template <>
__device__ __forceinline__ float abs_times(const float& w, const float& g) { return fabsf(w) * g; }
template <>
__device__ __forceinline__ f32x4 abs_times(const f32x4& w, const f32x4& g) {
  return f32x4{fabsf(w[0]) * g[0], fabsf(w[1]) * g[1], fabsf(w[2]) * g[2], fabsf(w[3]) * g[3]};
}
template <class T>
struct Two {
  T a, b;
};
struct PlainTerms {
  const float* x;
  template <class T>
  __device__ __forceinline__ T load(long i) const { return reinterpret_cast<const T*>(x)[i]; }
  template <class T>
  __device__ __forceinline__ T term(long, const T& raw) const { return raw; }
};
struct AbsWeightTerms {
  const float *w, *g;
  template <class T>
  __device__ __forceinline__ Two<T> load(long i) const { return {reinterpret_cast<const T*>(w)[i], reinterpret_cast<const T*>(g)[i]}; }
  template <class T>
  __device__ __forceinline__ T term(long, const Two<T>& raw) const { return abs_times(raw.a, raw.b); }
};
// g, and on the way p = backup for the same elements (ss_sam_restore_sumsq: the weights come back while their gradient is read)
struct RestoreTerms {
  float* p;
  const float *backup, *g;
  template <class T>
  __device__ __forceinline__ Two<T> load(long i) const { return {reinterpret_cast<const T*>(backup)[i], reinterpret_cast<const T*>(g)[i]}; }
  template <class T>
  __device__ __forceinline__ T term(long i, const Two<T>& raw) const {
    reinterpret_cast<T*>(p)[i] = raw.a;
    return raw.b;
  }
};

// out += the sum of the squared terms of [0, n): written once for ss_sumsq_f32, ss_sumsq_absw_f32 and ss_sam_restore_sumsq -- the
// same walk, the same expressions, hence the same order of adds and the same contractions in all three.
template <class Terms>
__global__ __launch_bounds__(256) void sumsq_kernel(Terms t, long n, float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  const long n4 = n >> 2;
  // four trips' 16-byte loads in flight per thread (a dependent chain of single loads made the 28 MB bucket of config 5 a 28 us kernel:
  // 1 TB/s; one launch's atomics -- one per workgroup on one address, ~12 ns each -- bound the workgroup count from above)
  const long stride = (long)gridDim.x * 256;
  long q = (long)blockIdx.x * 256 + threadIdx.x;
  for (; q + 3 * stride < n4; q += 4 * stride) {
    const auto r0 = t.template load<f32x4>(q), r1 = t.template load<f32x4>(q + stride), r2 = t.template load<f32x4>(q + 2 * stride),
               r3 = t.template load<f32x4>(q + 3 * stride);
    const f32x4 v0 = t.term(q, r0), v1 = t.term(q + stride, r1), v2 = t.term(q + 2 * stride, r2), v3 = t.term(q + 3 * stride, r3);
    acc += (v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2] + v0[3] * v0[3]) + (v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2] + v1[3] * v1[3]) +
           (v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2] + v2[3] * v2[3]) + (v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2] + v3[3] * v3[3]);
  }
  for (; q < n4; q += stride) {
    const f32x4 v = t.term(q, t.template load<f32x4>(q));
    acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    float v = t.term(i, t.template load<float>(i));
    acc += v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// The ascent step of sharpness-aware minimisation, one pass: backup = w, w += e, g = 0, with e = scale g (SAM) or scale w^2 g
// (ADAPTIVE: ASAM) and scale = rho grad_scale / (sqrt(sumsq) grad_scale + 1e-12), taken once per thread from the device word.
// Two quads per lane and trip: four 16-byte loads in flight, six stores behind them; the n & 3 last elements by block 0, which
// also clears the few scalars the second pass adds onto (none of them is the sumsq word: the entry point refuses that).
struct SamParams {
  float *p, *g, *backup;
  long n;
  const float* sumsq;
  float grad_scale, rho;
  float* zero_f;
  int* zero_i;
  int n_zero_f, n_zero_i;
};
constexpr int SAM_MAX_SCALARS = 256;

template <bool ADAPTIVE>
__device__ __forceinline__ float sam_ascend(float scale, float w, float g) {
  return ADAPTIVE ? w + (scale * g) * (w * w) : w + scale * g;
}
template <bool ADAPTIVE>
__device__ __forceinline__ f32x4 sam_ascend(float scale, const f32x4& w, const f32x4& g) {
  return f32x4{sam_ascend<ADAPTIVE>(scale, w[0], g[0]), sam_ascend<ADAPTIVE>(scale, w[1], g[1]),
               sam_ascend<ADAPTIVE>(scale, w[2], g[2]), sam_ascend<ADAPTIVE>(scale, w[3], g[3])};
}

template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void sam_perturb_kernel(SamParams a) {
  const float scale = a.rho * a.grad_scale / (sqrtf(a.sumsq[0]) * a.grad_scale + 1e-12f);
  const long n4 = a.n >> 2;
  f32x4* p4 = reinterpret_cast<f32x4*>(a.p);
  f32x4* g4 = reinterpret_cast<f32x4*>(a.g);
  f32x4* b4 = reinterpret_cast<f32x4*>(a.backup);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const long stride = (long)gridDim.x * 256;
  long q = (long)blockIdx.x * 256 + threadIdx.x;
  for (; q + stride < n4; q += 2 * stride) {
    const f32x4 w0 = p4[q], w1 = p4[q + stride], g0 = g4[q], g1 = g4[q + stride];
    b4[q] = w0;
    b4[q + stride] = w1;
    p4[q] = sam_ascend<ADAPTIVE>(scale, w0, g0);
    p4[q + stride] = sam_ascend<ADAPTIVE>(scale, w1, g1);
    g4[q] = zero;
    g4[q + stride] = zero;
  }
  if (q < n4) {
    const f32x4 w = p4[q], g = g4[q];
    b4[q] = w;
    p4[q] = sam_ascend<ADAPTIVE>(scale, w, g);
    g4[q] = zero;
  }
  if (blockIdx.x == 0) {
    if ((long)threadIdx.x < (a.n & 3)) {
      const long i = (n4 << 2) + threadIdx.x;
      const float w = a.p[i], g = a.g[i];
      a.backup[i] = w;
      a.p[i] = sam_ascend<ADAPTIVE>(scale, w, g);
      a.g[i] = 0.f;
    }
    if ((int)threadIdx.x < a.n_zero_f) a.zero_f[threadIdx.x] = 0.f;
    if ((int)threadIdx.x < a.n_zero_i) a.zero_i[threadIdx.x] = 0;
  }
}

struct AdamParams {
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  const float* sumsq;
  float grad_scale, max_norm, step_size, beta1, beta2, eps, inv_sqrt_bc2;
};

// The clip coefficient and one element of clip + Adam, written once for the three Adam kernels: the same expressions, hence the
// same contractions, hence the same bits of p, m, v from every entry point.
__device__ __forceinline__ float adam_clip_coef(const AdamParams& a) {
  const float total = sqrtf(a.sumsq[0]) * a.grad_scale;
  return a.grad_scale * fminf(1.0f, a.max_norm / (total + 1e-6f));
}

// (two halves, so that adam_clip_kernel can go on reading p behind its stores of m and v, as it always has)
__device__ __forceinline__ float adam_clip_moments(const AdamParams& a, float coef, float g_raw, float& m, float& v) {
  const float g = g_raw * coef;
  m = a.beta1 * m + (1.0f - a.beta1) * g;
  v = a.beta2 * v + (1.0f - a.beta2) * g * g;
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  return m / denom;
}
__device__ __forceinline__ float adam_clip_apply(const AdamParams& a, float p, float quot) { return p - a.step_size * quot; }

__global__ __launch_bounds__(256) void adam_clip_kernel(AdamParams a) {
  const float coef = adam_clip_coef(a);
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < a.n; q += (long)gridDim.x * 256) {
    float m = a.m[q], v = a.v[q];
    const float quot = adam_clip_moments(a, coef, a.g[q], m, v);
    a.m[q] = m;
    a.v[q] = v;
    a.p[q] = adam_clip_apply(a, a.p[q], quot);
  }
}

// The weight average ema = d * ema + (1 - d) * p_new.  omd = 1 - d, taken once on the host in f32.  d = 0: 0 * ema + 1 * p_new,
// p_new exactly.
__device__ __forceinline__ float ema_elem(float d, float omd, float ema, float p_new) { return d * ema + omd * p_new; }

// One element of the fused update, written once for adam_clip_ema_kernel <false, true> and adamw_groups_kernel<EMA> <true, EMA>.
// DECAY: p1 = p * decay is rounded on its own (__fmul_rn: torch's in-place mul_; a plain product would be contracted into the
// update behind it), then m, v, p are adam_clip_moments / adam_clip_apply on p1.  decay = 1: p1 is p.
template <bool DECAY, bool EMA>
__device__ __forceinline__ void adam_update(const AdamParams& a, float coef, float decay, float d, float omd, float g, float& p,
                                            float& m, float& v, float& e) {
  p = adam_clip_apply(a, DECAY ? __fmul_rn(p, decay) : p, adam_clip_moments(a, coef, g, m, v));
  if (EMA) e = ema_elem(d, omd, e, p);
}
// (a quad: the four elements one after the other)
template <bool DECAY, bool EMA>
__device__ __forceinline__ void adam_update(const AdamParams& a, float coef, float decay, float d, float omd, const f32x4& g,
                                            f32x4& p, f32x4& m, f32x4& v, f32x4& e) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = p[k], mk = m[k], vk = v[k], ek = e[k];
    adam_update<DECAY, EMA>(a, coef, decay, d, omd, g[k], pk, mk, vk, ek);
    p[k] = pk; m[k] = mk; v[k] = vk; e[k] = ek;
  }
}
// Load, update and store item i of the bucket: T = f32x4, quad i (floats [4i, 4i + 4)), or T = float, element i.  `ema` is
// neither read nor written without EMA.
template <bool DECAY, bool EMA, class T>
__device__ __forceinline__ void adam_update_at(const AdamParams& a, float coef, float decay, float* ema, float d, float omd, long i) {
  T* pp = reinterpret_cast<T*>(a.p) + i;
  T* mp = reinterpret_cast<T*>(a.m) + i;
  T* vp = reinterpret_cast<T*>(a.v) + i;
  T* ep = reinterpret_cast<T*>(ema) + i;
  T p = *pp, m = *mp, v = *vp, e = {};
  if (EMA) e = *ep;
  const T g = reinterpret_cast<const T*>(a.g)[i];
  adam_update<DECAY, EMA>(a, coef, decay, d, omd, g, p, m, v, e);
  *mp = m;
  *vp = v;
  *pp = p;
  if (EMA) *ep = e;
}

// adam_clip_kernel + the weight average in the same pass: five 16-byte loads and four 16-byte stores per lane and iteration (nine
// streams of n floats against seven), the n & 3 last elements by block 0.
__global__ __launch_bounds__(256) void adam_clip_ema_kernel(AdamParams a, float* ema, float d, float omd) {
  const float coef = adam_clip_coef(a);
  const long n4 = a.n >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256)
    adam_update_at<false, true, f32x4>(a, coef, 1.0f, ema, d, omd, q);
  if (blockIdx.x == 0 && (long)threadIdx.x < (a.n & 3))
    adam_update_at<false, true, float>(a, coef, 1.0f, ema, d, omd, (n4 << 2) + threadIdx.x);
}

// Grouped AdamW: adam_clip_ema_kernel with a decoupled weight decay and a learning rate per segment of the bucket.  The segment
// table travels by value (kernel arguments) and is only ever indexed by the loop counter below, which is the same in every lane:
// bounds, step size and decay of the segment in hand are scalar loads, no lane looks anything up and nothing goes to scratch.
// Every workgroup walks all segments and strides over the quads of each.  The workgroup that takes a segment's first 256 quads
// moves on from segment to segment (first_block, from the host: the segments' 256-quad pieces are dealt round the grid one behind
// the other), so a bucket of many small segments costs no workgroup more trips than an even share.  With every segment starting
// at workgroup 0 that one made a dependent load-store trip per segment: 16.6 us against 5.3 us on the 1.08 M floats and 22
// segments of config 2.
// The update is adam_update<true, EMA> with the segment's decay and step size.
constexpr int ADAMW_MAX_SEGMENTS = 64, ADAMW_MAX_GROUPS = 8;
struct AdamwSegments {
  long end[ADAMW_MAX_SEGMENTS];  // segment s is [end[s-1], end[s]), end[-1] = 0; every end but the last a multiple of 4; the last n
  float step_size[ADAMW_MAX_SEGMENTS], decay[ADAMW_MAX_SEGMENTS];
  int first_block[ADAMW_MAX_SEGMENTS];  // the workgroup that takes the segment's first 256 quads, in [0, gridDim.x)
  int n_seg;
};

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(AdamParams a, AdamwSegments t, float* ema, float d, float omd) {
  const float coef = adam_clip_coef(a);
  AdamParams b = a;  // (the segment's step size in the place adam_clip_apply reads it from)
  float decay = 1.0f;
  long q0 = 0;
  for (int s = 0; s < t.n_seg; ++s) {
    const long q1 = t.end[s] >> 2;
    b.step_size = t.step_size[s];
    decay = t.decay[s];
    int piece = (int)blockIdx.x - t.first_block[s];
    if (piece < 0) piece += gridDim.x;
    for (long q = q0 + (long)piece * 256 + threadIdx.x; q < q1; q += (long)gridDim.x * 256)
      adam_update_at<true, EMA, f32x4>(b, coef, decay, ema, d, omd, q);
    q0 = q1;
  }
  // the n & 3 last elements lie in the last segment (every other end is a multiple of 4): b and decay still are that segment's
  if (blockIdx.x == 0 && (long)threadIdx.x < (a.n & 3))
    adam_update_at<true, EMA, float>(b, coef, decay, ema, d, omd, (a.n & ~3L) + threadIdx.x);
}

// LAMB (You et al. 2020): the Adam direction plus the weight decay, rescaled per segment (one parameter tensor) by |w| / |u|.  Two
// streams with a small reduction between them, on the walk of adamw_groups_kernel (by-value table, wave-uniform segment loop,
// first_block dealing, the n & 3 last elements by block 0 in the last segment):
//   lamb_moments_kernel  reads g, m, v, p; writes m, v (adam_clip_moments: the bits of adam_clip_kernel); forms u and leaves the
//                        float64 sums of p^2 and u^2 of every (segment, workgroup) that holds quads of the segment in `scratch`
//   lamb_norms_kernel    one workgroup per segment adds those partials up in a fixed order -> sqrt P, sqrt U and the trust ratio
//   lamb_apply_kernel    recomputes u from the stored m, v, p (lamb_direction again: the same bits) and takes p -= (lr_s r_s) u
// Nothing is added with atomics: every sum below has one order, whatever the schedule, so two runs give the same bits.
struct LambSegments {
  long end[ADAMW_MAX_SEGMENTS];  // as AdamwSegments
  float wd[ADAMW_MAX_SEGMENTS], lr[ADAMW_MAX_SEGMENTS];
  int first_block[ADAMW_MAX_SEGMENTS];
  int n_seg;
};

// u = wd p + bc1 m / (sqrt(v) inv_sqrt_bc2 + eps): the quotient is adam_clip_moments' expression on the same operands, the product
// bc1 * quot is rounded on its own and then fused into the sum
__device__ __forceinline__ float lamb_direction(const AdamParams& a, float bc1, float wd, float p, float m, float v) {
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  return fmaf(wd, p, __fmul_rn(bc1, m / denom));
}

// The workgroup's piece of segment s (the 256-quad pieces of a segment are dealt round the grid from first_block[s] on), and
// whether the workgroup adds anything to the segment's sums: it holds quads of it, or it is block 0 with the n & 3 last elements
__device__ __forceinline__ int lamb_piece(const LambSegments& t, int s, int block, int blocks) {
  const int piece = block - t.first_block[s];
  return piece < 0 ? piece + blocks : piece;
}
__device__ __forceinline__ bool lamb_contributes(const LambSegments& t, int s, int block, int blocks, long n) {
  const long q0 = s ? t.end[s - 1] >> 2 : 0, q1 = t.end[s] >> 2;
  return q0 + (long)lamb_piece(t, s, block, blocks) * 256 < q1 || (block == 0 && s == t.n_seg - 1 && (n & 3));
}

__device__ __forceinline__ double wave_sum_f64(double v) {  // (a butterfly: every lane ends with the same bits)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Moments and squares of item i: T = f32x4 (quad i) or float (element i).  The squares are f32 products, widened, added in f64.
template <class T>
__device__ __forceinline__ void lamb_moments_at(const AdamParams& a, float coef, float bc1, float wd, long i, double& sum_p, double& sum_u);
template <>
__device__ __forceinline__ void lamb_moments_at<float>(const AdamParams& a, float coef, float bc1, float wd, long i, double& sum_p,
                                                       double& sum_u) {
  float m = a.m[i], v = a.v[i];
  const float p = a.p[i];
  adam_clip_moments(a, coef, a.g[i], m, v);
  a.m[i] = m;
  a.v[i] = v;
  const float u = lamb_direction(a, bc1, wd, p, m, v);
  sum_p += (double)__fmul_rn(p, p);
  sum_u += (double)__fmul_rn(u, u);
}
template <>
__device__ __forceinline__ void lamb_moments_at<f32x4>(const AdamParams& a, float coef, float bc1, float wd, long i, double& sum_p,
                                                       double& sum_u) {
  f32x4* mp = reinterpret_cast<f32x4*>(a.m) + i;
  f32x4* vp = reinterpret_cast<f32x4*>(a.v) + i;
  f32x4 m = *mp, v = *vp;
  const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i], p = reinterpret_cast<const f32x4*>(a.p)[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float mk = m[k], vk = v[k];
    adam_clip_moments(a, coef, g[k], mk, vk);
    m[k] = mk; v[k] = vk;
  }
  *mp = m;
  *vp = v;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u = lamb_direction(a, bc1, wd, p[k], m[k], v[k]);
    sum_p += (double)__fmul_rn(p[k], p[k]);
    sum_u += (double)__fmul_rn(u, u);
  }
}

// scratch[(s * gridDim.x + block) * 2 + {0, 1}] = the workgroup's sums of p^2 and u^2 over segment s, written only where
// lamb_contributes (a condition on the block, the same in all its lanes): a thread's items in ascending order, the butterfly over
// the wave, the four waves in order.  red is used in turns (`turn` counts this workgroup's reductions), so one barrier per
// reduction separates thread 0's reads from the next writes to the same half.
__global__ __launch_bounds__(256) void lamb_moments_kernel(AdamParams a, LambSegments t, float bc1, double* __restrict__ scratch) {
  __shared__ double red[2][4][2];
  const float coef = adam_clip_coef(a);
  const bool tail = blockIdx.x == 0 && (a.n & 3);
  int turn = 0;
  long q0 = 0;
  for (int s = 0; s < t.n_seg; ++s) {
    const long q1 = t.end[s] >> 2;
    const float wd = t.wd[s];
    const long first = q0 + (long)lamb_piece(t, s, blockIdx.x, gridDim.x) * 256;
    const bool last = s == t.n_seg - 1;
    if (first < q1 || (last && tail)) {
      double sum_p = 0.0, sum_u = 0.0;
      for (long q = first + threadIdx.x; q < q1; q += (long)gridDim.x * 256) lamb_moments_at<f32x4>(a, coef, bc1, wd, q, sum_p, sum_u);
      if (last && tail && (long)threadIdx.x < (a.n & 3)) lamb_moments_at<float>(a, coef, bc1, wd, (a.n & ~3L) + threadIdx.x, sum_p, sum_u);
      sum_p = wave_sum_f64(sum_p);
      sum_u = wave_sum_f64(sum_u);
      if ((threadIdx.x & 63) == 0) {
        red[turn][threadIdx.x >> 6][0] = sum_p;
        red[turn][threadIdx.x >> 6][1] = sum_u;
      }
      __syncthreads();
      if (threadIdx.x < 2)
        scratch[((long)s * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            ((red[turn][0][threadIdx.x] + red[turn][1][threadIdx.x]) + red[turn][2][threadIdx.x]) + red[turn][3][threadIdx.x];
      turn ^= 1;
    }
    q0 = q1;
  }
}

// Workgroup s: the partials of segment s in workgroup order -- thread t takes the workgroups t, t + 256, ... in ascending order,
// then the butterfly and the four waves as above -- and norms[2 s] = sqrt P, norms[2 s + 1] = sqrt U, ratio[s] = sqrt(P / U) where
// the segment adapts (bit s of `adapt`) and both sums are positive, else 1.  `blocks`: the grid of lamb_moments_kernel.
__global__ __launch_bounds__(256) void lamb_norms_kernel(LambSegments t, long n, int blocks, unsigned long long adapt,
                                                         const double* __restrict__ scratch, float* __restrict__ norms,
                                                         float* __restrict__ ratio) {
  __shared__ double red[4][2];
  const int s = blockIdx.x;
  double sum_p = 0.0, sum_u = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256)
    if (lamb_contributes(t, s, b, blocks, n)) {
      sum_p += scratch[((long)s * blocks + b) * 2];
      sum_u += scratch[((long)s * blocks + b) * 2 + 1];
    }
  sum_p = wave_sum_f64(sum_p);
  sum_u = wave_sum_f64(sum_u);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = sum_p;
    red[threadIdx.x >> 6][1] = sum_u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double P = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], U = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    norms[2 * s] = (float)sqrt(P);
    norms[2 * s + 1] = (float)sqrt(U);
    ratio[s] = ((adapt >> s) & 1) && P > 0.0 && U > 0.0 ? (float)sqrt(P / U) : 1.0f;
  }
}

// Load p, m, v (and the average) of item i, take p -= step u with u = lamb_direction, store p (and the average: ema_elem).
template <bool EMA, class T>
__device__ __forceinline__ void lamb_apply_at(const AdamParams& a, float bc1, float wd, float step, float* ema, float d, float omd, long i);
template <bool EMA>
__device__ __forceinline__ float lamb_apply_elem(const AdamParams& a, float bc1, float wd, float step, float d, float omd, float p,
                                                 float m, float v, float& e) {
  p = p - step * lamb_direction(a, bc1, wd, p, m, v);
  if (EMA) e = ema_elem(d, omd, e, p);
  return p;
}
template <bool EMA, class T>
__device__ __forceinline__ void lamb_apply_at(const AdamParams& a, float bc1, float wd, float step, float* ema, float d, float omd, long i) {
  T* pp = reinterpret_cast<T*>(a.p) + i;
  T* ep = reinterpret_cast<T*>(ema) + i;
  T p = *pp, e = {};
  const T m = reinterpret_cast<const T*>(a.m)[i], v = reinterpret_cast<const T*>(a.v)[i];
  if (EMA) e = *ep;
  if constexpr (sizeof(T) == sizeof(float)) {
    p = lamb_apply_elem<EMA>(a, bc1, wd, step, d, omd, p, m, v, e);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float ek = e[k];
      p[k] = lamb_apply_elem<EMA>(a, bc1, wd, step, d, omd, p[k], m[k], v[k], ek);
      e[k] = ek;
    }
  }
  *pp = p;
  if (EMA) *ep = e;
}

// ratio[s] is read once per segment, with the loop counter: a scalar load, as the table's entries are
template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(AdamParams a, LambSegments t, float bc1, const float* __restrict__ ratio,
                                                         float* ema, float d, float omd) {
  float wd = 0.0f, step = 0.0f;
  long q0 = 0;
  for (int s = 0; s < t.n_seg; ++s) {
    const long q1 = t.end[s] >> 2;
    wd = t.wd[s];
    step = __fmul_rn(t.lr[s], ratio[s]);
    for (long q = q0 + (long)lamb_piece(t, s, blockIdx.x, gridDim.x) * 256 + threadIdx.x; q < q1; q += (long)gridDim.x * 256)
      lamb_apply_at<EMA, f32x4>(a, bc1, wd, step, ema, d, omd, q);
    q0 = q1;
  }
  if (blockIdx.x == 0 && (long)threadIdx.x < (a.n & 3))  // (in the last segment: wd and step still are that segment's)
    lamb_apply_at<EMA, float>(a, bc1, wd, step, ema, d, omd, (a.n & ~3L) + threadIdx.x);
}

// a <-> b, two disjoint 16-byte aligned buffers of n floats: 16-byte lanes, the n & 3 last elements by block 0
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
  const long n4 = n >> 2;
  f32x4* a4 = reinterpret_cast<f32x4*>(a);
  f32x4* b4 = reinterpret_cast<f32x4*>(b);
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
    const f32x4 x = a4[q], y = b4[q];
    a4[q] = y;
    b4[q] = x;
  }
  if (blockIdx.x == 0 && (long)threadIdx.x < (n & 3)) {
    const long q = (n4 << 2) + threadIdx.x;
    const float x = a[q], y = b[q];
    a[q] = y;
    b[q] = x;
  }
}

}  // namespace

// every block ends in one float atomic on the same word (~11 ns each, serialised): 128 blocks, not 1024
template <class Terms>
static int sumsq_launch(Terms t, long n, float* sumsq, ss_stream_t stream) {
  hipLaunchKernelGGL(sumsq_kernel<Terms>, dim3(ss_flat_grid(n >> 2, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), t, n, sumsq);
  return ss_launch_status();
}

extern "C" int ss_sumsq_f32(const float* x, long n, float* sumsq, ss_stream_t stream) {
  SS_REQUIRE(x && sumsq && n > 0, SS_ERR_ARG);
  SS_REQUIRE(ss_aligned16(x), SS_ERR_ARG);
  return sumsq_launch(PlainTerms{x}, n, sumsq, stream);
}

extern "C" int ss_sumsq_absw_f32(const float* w, const float* g, long n, float* sumsq, ss_stream_t stream) {
  SS_REQUIRE(w && g && sumsq && n > 0, SS_ERR_ARG);
  SS_REQUIRE(ss_aligned16(w, g), SS_ERR_ARG);
  return sumsq_launch(AbsWeightTerms{w, g}, n, sumsq, stream);
}

static float adam_step_size(float lr, float beta1, int step) {
  const double bc1 = 1.0 - pow((double)beta1, step);
  return (float)((double)lr / bc1);
}

static void adam_params(AdamParams& a, float* p, const float* g, float* m, float* v, long n, const float* sumsq, float grad_scale,
                        float max_norm, float lr, float beta1, float beta2, float eps, int step) {
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.sumsq = sumsq;
  a.grad_scale = grad_scale; a.max_norm = max_norm;
  const double bc2 = 1.0 - pow((double)beta2, step);
  a.step_size = adam_step_size(lr, beta1, step);
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
}

static bool disjoint_f32(const float* a, const float* b, long n) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * 4;
  return x + bytes <= y || y + bytes <= x;
}

// What the three Adam entry points all refuse.  wide: the kernel works in 16-byte lanes.  ema null: no weight average, its decay is
// not looked at (ss_adam_clip_ema asks for the pointer itself).
static int adam_check(const float* p, const float* g, const float* m, const float* v, const float* sumsq, long n, int step, bool wide,
                      const float* ema, float ema_decay) {
  SS_REQUIRE(p && g && m && v && sumsq && n > 0 && step >= 1, SS_ERR_ARG);
  SS_REQUIRE(!wide || ss_aligned16(p, g, m, v, ema), SS_ERR_ARG);
  SS_REQUIRE(!ema || (ema_decay >= 0.0f && ema_decay < 1.0f), SS_ERR_ARG);  // (a NaN fails both)
  SS_REQUIRE(!ema || (ema != p && disjoint_f32(ema, p, n)), SS_ERR_ARG);
  return SS_OK;
}

extern "C" int ss_adam_clip(float* p, const float* g, float* m, float* v, long n, const float* sumsq,
                            float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                            ss_stream_t stream) {
  if (const int bad = adam_check(p, g, m, v, sumsq, n, step, false, nullptr, 0.0f)) return bad;
  AdamParams a;
  adam_params(a, p, g, m, v, n, sumsq, grad_scale, max_norm, lr, beta1, beta2, eps, step);
  hipLaunchKernelGGL(adam_clip_kernel, dim3(ss_flat_grid(n, 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return ss_launch_status();
}

extern "C" int ss_adam_clip_ema(float* p, const float* g, float* m, float* v, float* ema, long n, const float* sumsq,
                                float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                                float ema_decay, ss_stream_t stream) {
  SS_REQUIRE(ema, SS_ERR_ARG);
  if (const int bad = adam_check(p, g, m, v, sumsq, n, step, true, ema, ema_decay)) return bad;
  AdamParams a;
  adam_params(a, p, g, m, v, n, sumsq, grad_scale, max_norm, lr, beta1, beta2, eps, step);
  hipLaunchKernelGGL(adam_clip_ema_kernel, dim3(ss_flat_grid(n >> 2, 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), a, ema,
                     ema_decay, 1.0f - ema_decay);
  return ss_launch_status();
}

extern "C" int ss_adamw_clip_groups(float* p, const float* g, float* m, float* v, float* ema, long n, const float* sumsq,
                                    float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, int step,
                                    float ema_decay, const long* seg_end, const int* seg_group, int n_seg,
                                    const float* group_lr_scale, const float* group_weight_decay, int n_groups,
                                    ss_stream_t stream) {
  if (const int bad = adam_check(p, g, m, v, sumsq, n, step, true, ema, ema_decay)) return bad;
  SS_REQUIRE(seg_end && seg_group && group_lr_scale && group_weight_decay, SS_ERR_ARG);
  SS_REQUIRE(n_seg >= 1 && n_seg <= ADAMW_MAX_SEGMENTS && n_groups >= 1 && n_groups <= ADAMW_MAX_GROUPS, SS_ERR_ARG);
  for (int G = 0; G < n_groups; ++G)  // (a NaN fails >=, an infinity isfinite)
    SS_REQUIRE(group_lr_scale[G] >= 0.0f && isfinite(group_lr_scale[G]) && group_weight_decay[G] >= 0.0f &&
                   isfinite(group_weight_decay[G]), SS_ERR_ARG);
  AdamParams a;
  adam_params(a, p, g, m, v, n, sumsq, grad_scale, max_norm, lr, beta1, beta2, eps, step);
  AdamwSegments t;
  const int blocks = ss_flat_grid(n >> 2, 2048);
  long lo = 0, pieces = 0;  // pieces: 256-quad pieces of the segments in front
  for (int s = 0; s < ADAMW_MAX_SEGMENTS; ++s) {
    if (s >= n_seg) {  // (unused entries: defined values, never read)
      t.end[s] = n; t.step_size[s] = 0.0f; t.decay[s] = 1.0f; t.first_block[s] = 0;
      continue;
    }
    const long hi = seg_end[s];
    const int G = seg_group[s];
    SS_REQUIRE(hi > lo && hi <= n && (s == n_seg - 1 ? hi == n : (hi & 3) == 0) && G >= 0 && G < n_groups, SS_ERR_ARG);
    const float lr_g = (float)((double)lr * (double)group_lr_scale[G]);
    t.end[s] = hi;
    t.step_size[s] = adam_step_size(lr_g, beta1, step);
    t.decay[s] = (float)(1.0 - (double)lr_g * (double)group_weight_decay[G]);
    t.first_block[s] = (int)(pieces % blocks);
    pieces += ((hi >> 2) - (lo >> 2) + 255) / 256;
    lo = hi;
  }
  t.n_seg = n_seg;
  if (ema)
    hipLaunchKernelGGL(adamw_groups_kernel<true>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a, t, ema,
                       ema_decay, 1.0f - ema_decay);
  else
    hipLaunchKernelGGL(adamw_groups_kernel<false>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a, t, ema,
                       0.0f, 1.0f);
  return ss_launch_status();
}

// The table of the two LAMB entry points from the host arrays, checked as ss_adamw_clip_groups checks its own.  blocks: the grid the
// pieces are dealt round (both launches of ss_lamb_moments use one grid; ss_lamb_apply's is the same function of n).
static int lamb_grid(long n) { return ss_flat_grid(n >> 2, 2048); }

static int lamb_table(LambSegments& t, unsigned long long& adapt, long n, float lr, const long* seg_end, const int* seg_group, int n_seg,
                      const float* group_lr_scale, const float* group_weight_decay, int n_groups, const int* seg_adapt) {
  SS_REQUIRE(seg_end && seg_group && group_lr_scale && group_weight_decay && seg_adapt, SS_ERR_ARG);
  SS_REQUIRE(n_seg >= 1 && n_seg <= ADAMW_MAX_SEGMENTS && n_groups >= 1 && n_groups <= ADAMW_MAX_GROUPS, SS_ERR_ARG);
  SS_REQUIRE(lr >= 0.0f && isfinite(lr), SS_ERR_ARG);
  for (int G = 0; G < n_groups; ++G)  // (a NaN fails >=, an infinity isfinite)
    SS_REQUIRE(group_lr_scale[G] >= 0.0f && isfinite(group_lr_scale[G]) && group_weight_decay[G] >= 0.0f &&
                   isfinite(group_weight_decay[G]), SS_ERR_ARG);
  const int blocks = lamb_grid(n);
  long lo = 0, pieces = 0;
  adapt = 0;
  for (int s = 0; s < ADAMW_MAX_SEGMENTS; ++s) {
    if (s >= n_seg) {  // (unused entries: defined values, never read)
      t.end[s] = n; t.wd[s] = 0.0f; t.lr[s] = 0.0f; t.first_block[s] = 0;
      continue;
    }
    const long hi = seg_end[s];
    const int G = seg_group[s];
    SS_REQUIRE(hi > lo && hi <= n && (s == n_seg - 1 ? hi == n : (hi & 3) == 0) && G >= 0 && G < n_groups, SS_ERR_ARG);
    t.end[s] = hi;
    t.wd[s] = group_weight_decay[G];
    t.lr[s] = (float)((double)lr * (double)group_lr_scale[G]);
    t.first_block[s] = (int)(pieces % blocks);
    if (seg_adapt[s]) adapt |= 1ull << s;
    pieces += ((hi >> 2) - (lo >> 2) + 255) / 256;
    lo = hi;
  }
  t.n_seg = n_seg;
  return SS_OK;
}

static float lamb_bc1(float beta1, int step) { return (float)(1.0 / (1.0 - pow((double)beta1, step))); }

extern "C" int ss_lamb_scratch_bytes(long n, int n_seg, long* bytes) {
  SS_REQUIRE(bytes && n > 0 && n_seg >= 1 && n_seg <= ADAMW_MAX_SEGMENTS, SS_ERR_ARG);
  *bytes = (long)n_seg * lamb_grid(n) * 2 * (long)sizeof(double);
  return SS_OK;
}

extern "C" int ss_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* sumsq, float grad_scale,
                               float max_norm, float beta1, float beta2, float eps, int step, const long* seg_end,
                               const int* seg_group, int n_seg, const float* group_lr_scale, const float* group_weight_decay,
                               int n_groups, const int* seg_adapt, double* scratch, float* norms, float* ratio, ss_stream_t stream) {
  if (const int bad = adam_check(p, g, m, v, sumsq, n, step, true, nullptr, 0.0f)) return bad;
  SS_REQUIRE(scratch && norms && ratio && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0, SS_ERR_ARG);
  LambSegments t;
  unsigned long long adapt;
  if (const int bad = lamb_table(t, adapt, n, 0.0f, seg_end, seg_group, n_seg, group_lr_scale, group_weight_decay, n_groups, seg_adapt))
    return bad;
  AdamParams a;
  adam_params(a, const_cast<float*>(p), g, m, v, n, sumsq, grad_scale, max_norm, 0.0f, beta1, beta2, eps, step);
  const int blocks = lamb_grid(n);
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a, t, lamb_bc1(beta1, step),
                     scratch);
  hipLaunchKernelGGL(lamb_norms_kernel, dim3(n_seg), dim3(256), 0, static_cast<hipStream_t>(stream), t, n, blocks, adapt, scratch, norms,
                     ratio);
  return ss_launch_status();
}

extern "C" int ss_lamb_apply(float* p, const float* m, const float* v, float* ema, long n, float beta1, float beta2, float eps, int step,
                             float ema_decay, float lr, const long* seg_end, const int* seg_group, int n_seg,
                             const float* group_lr_scale, const float* group_weight_decay, int n_groups, const int* seg_adapt,
                             const float* ratio, ss_stream_t stream) {
  // (adam_check's rules, with the ratios in the place of the gradient and its sum of squares: pointers it only tests for NULL)
  if (const int bad = adam_check(p, ratio, m, v, ratio, n, step, false, ema, ema_decay)) return bad;
  SS_REQUIRE(ss_aligned16(p, m, v, ema), SS_ERR_ARG);
  LambSegments t;
  unsigned long long adapt;
  if (const int bad = lamb_table(t, adapt, n, lr, seg_end, seg_group, n_seg, group_lr_scale, group_weight_decay, n_groups, seg_adapt))
    return bad;
  AdamParams a;
  adam_params(a, p, nullptr, const_cast<float*>(m), const_cast<float*>(v), n, nullptr, 1.0f, 1.0f, 0.0f, beta1, beta2, eps, step);
  const float bc1 = lamb_bc1(beta1, step);
  const dim3 grid(lamb_grid(n));
  if (ema)
    hipLaunchKernelGGL(lamb_apply_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, t, bc1, ratio, ema, ema_decay,
                       1.0f - ema_decay);
  else
    hipLaunchKernelGGL(lamb_apply_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, t, bc1, ratio, ema, 0.0f, 1.0f);
  return ss_launch_status();
}

// What the two SAM entry points both refuse: backup is scratch of its own beside the weights and their gradient.
static int sam_check(const float* p, const float* backup, const float* g, const float* sumsq, long n) {
  SS_REQUIRE(p && backup && g && sumsq && n > 0, SS_ERR_ARG);
  SS_REQUIRE(ss_aligned16(p, backup, g), SS_ERR_ARG);
  SS_REQUIRE(disjoint_f32(backup, p, n) && disjoint_f32(backup, g, n), SS_ERR_ARG);
  return SS_OK;
}

extern "C" int ss_sam_perturb(float* p, float* g, float* backup, long n, const float* sumsq, float grad_scale, float rho,
                              int adaptive, float* zero_f, int n_zero_f, int* zero_i, int n_zero_i, ss_stream_t stream) {
  if (const int bad = sam_check(p, backup, g, sumsq, n)) return bad;
  SS_REQUIRE(rho > 0.0f && isfinite(rho), SS_ERR_ARG);  // (a NaN fails >)
  SS_REQUIRE(n_zero_f >= 0 && n_zero_f <= SAM_MAX_SCALARS && n_zero_i >= 0 && n_zero_i <= SAM_MAX_SCALARS, SS_ERR_ARG);
  SS_REQUIRE((zero_f || n_zero_f == 0) && (zero_i || n_zero_i == 0), SS_ERR_ARG);
  // every workgroup reads the sumsq word while block 0 clears: it is none of the cleared ones
  SS_REQUIRE(!(sumsq >= zero_f && sumsq < zero_f + n_zero_f), SS_ERR_ARG);
  SamParams a{p, g, backup, n, sumsq, grad_scale, rho, zero_f, zero_i, n_zero_f, n_zero_i};
  const dim3 grid(ss_flat_grid(n >> 2, 2048));
  if (adaptive)
    hipLaunchKernelGGL(sam_perturb_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(sam_perturb_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return ss_launch_status();
}

extern "C" int ss_sam_restore_sumsq(float* p, const float* backup, const float* g, long n, float* sumsq, ss_stream_t stream) {
  if (const int bad = sam_check(p, backup, g, sumsq, n)) return bad;
  return sumsq_launch(RestoreTerms{p, backup, g}, n, sumsq, stream);
}

extern "C" int ss_swap_f32(float* a, float* b, long n, ss_stream_t stream) {
  SS_REQUIRE(a && b && n > 0, SS_ERR_ARG);
  SS_REQUIRE(disjoint_f32(a, b, n), SS_ERR_ARG);
  SS_REQUIRE(ss_aligned16(a, b), SS_ERR_ARG);
  hipLaunchKernelGGL(swap_kernel, dim3(ss_flat_grid(n >> 2, 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, n);
  return ss_launch_status();
}

