// The arithmetic of one GRU cell and the row layout of what a step saves, shared by the four forms of the masked BiGRU
// recurrence: gru.hip (one CU per slice, f32), gru_split.h (multi-CU, f32), gru_bf16.hip (one launch per step, bf16) and
// gru_bf16_pers.h (persistent multi-CU, bf16).  Device code only; a lane holds four consecutive hidden units of one clip.
//
// What the stage timers of the two multi-CU families taught about a step's loads; the kernels refer to these by name:
//  * UNCONDITIONAL LOADS.  A step's inputs are loaded whatever the clip length says (a lane past its clip's end, or without a
//    previous state, reads a row of a valid clip and the step tests `valid` / `hp_ok` where it USES the values).  Behind
//    `if (t < len)` the registers were cleared first, and a write to the destination of an older load makes hipcc wait for that
//    load by COUNT: it cannot count the younger stores issued under divergent branches, so it waited for the step's
//    write-through granule stores as well.
//  * A STEP AHEAD.  The inputs of step s + 1 are independent of the recurrence and are requested during step s, behind the
//    sweep (forward) resp. into the registers the gate gradients have just finished with (backward).  Loads return in order:
//    requested at the top of their own step, or behind the publish, the sweep's L2 hits queued behind their HBM misses.
//  * THE DROPOUT SCALE STAYS BESIDE THE RAW LOAD of d_out and is applied where the gradient is used, a step later:
//    multiplying at the load made the wave sit through the latency of the load it had just issued, in front of every sweep
//    of a layer with dropout.
#pragma once

// The cell's formulas are macros, used per hidden unit inside the caller's unrolled loop, and not inline functions: these
// kernels are latency chains whose schedule follows the order in which the compiler meets every operation, and a function
// -- its arguments evaluated ahead of its body, its results passed through references or a returned struct -- came out of
// hipcc with another instruction order or register assignment in most of the kernels.  Expanded in place the text is the
// kernels' own.  Arguments are float expressions (results: lvalues), each evaluated where the formula uses it; GRU_GATES
// and GRU_GATE_GRADS are statement sequences and stand in a braced block of their own.
//
// r = sigma(pr), z = sigma(pz), n = tanh(gn + r q), q = W_hn h + b_hn; pr / pz are the pre-activation sums in the order the
// caller adds them (the step kernel (gi + gh) + b, the others gi + (b + MFMA chain)).  Then h' = (1 - z) n + z h.
#define GRU_GATES(r, z, n, pr, pz, gn, q) \
  (r) = sigmoid_f(pr);                    \
  (z) = sigmoid_f(pz);                    \
  (n) = tanh_f((gn) + (r) * (q))
#define GRU_BLEND(z, n, hp) ((1.0f - (z)) * (n) + (z) * (hp))

// BPTT through the cell.  d = gradient w.r.t. h' (the caller adds the output's gradient, scaled where it was dropped out,
// and the recurrence's); hprev is zero where there is no previous state.  dar, daz, dan = gradients of the r, z, n
// pre-activations (= d gi), dqn = d q (the hh side of n), dcarry = the part of d that reaches h without passing W_hh.
#define GRU_GATE_GRADS(dar, daz, dan, dqn, dcarry, d, r, z, n, q, hprev) \
  const float d_ = (d);                                                  \
  const float dn_ = d_ * (1.0f - (z));                                   \
  const float dz_ = d_ * ((hprev) - (n));                                \
  (dan) = dn_ * (1.0f - (n) * (n));                                      \
  (dar) = (dan) * (q) * (r) * (1.0f - (r));                              \
  (daz) = dz_ * (z) * (1.0f - (z));                                      \
  (dqn) = (dan) * (r);                                                   \
  (dcarry) = d_ * (z)

namespace {

// The [rows][ld] layout of `save` (r, z, n, q), d_g (d a_r, d a_z, d a_n, d q) and their packed-bf16 copies: this lane's
// vector V (f32x4 of float, uint2 of four packed bf16) of rows 0 .. 3 at p, p + ld, p + 2 ld, p + 3 ld.
template <typename T, typename V>
__device__ __forceinline__ void load_rows4(const T* p, int ld, V& a, V& b, V& c, V& d) {
  a = *reinterpret_cast<const V*>(p);
  b = *reinterpret_cast<const V*>(p + ld);
  c = *reinterpret_cast<const V*>(p + 2 * ld);
  d = *reinterpret_cast<const V*>(p + 3 * ld);
}
template <typename T, typename V>
__device__ __forceinline__ void store_rows3(T* p, int ld, const V& a, const V& b, const V& c) {
  *reinterpret_cast<V*>(p) = a;
  *reinterpret_cast<V*>(p + ld) = b;
  *reinterpret_cast<V*>(p + 2 * ld) = c;
}
template <typename T, typename V>
__device__ __forceinline__ void store_rows4(T* p, int ld, const V& a, const V& b, const V& c, const V& d) {
  store_rows3(p, ld, a, b, c);
  *reinterpret_cast<V*>(p + 3 * ld) = d;
}

// Per-lane running sums of the four gate gradients of hidden units j0..j0+3 (lane row = 16 clips); flush() adds the rows up on
// the DPP crossbar and lets one lane per row (i == 0) add them to the bias gradients (each [3H], all null = not wanted):
// d b_ih += sum over (clip, t) of (d a_r, d a_z, d a_n), d b_hh += the same with d q in the n block.  They ride on the BPTT: a
// pass over d_g afterwards costs as much HBM traffic as the weight-gradient GEMM that follows it.  Every lane of the wave
// must call flush().
struct GruBiasAcc {
  f32x4 r = {0.f, 0.f, 0.f, 0.f}, z = r, n = r, q = r;
  __device__ __forceinline__ void add(const f32x4& dar, const f32x4& daz, const f32x4& dan, const f32x4& dqn) {
    r += dar; z += daz; n += dan; q += dqn;
  }
  __device__ __forceinline__ void flush(float* const (&g_bih)[2], float* const (&g_bhh)[2], int dir, int H, int j0, int i) {
    if (!g_bih[dir]) return;
    float* gi = g_bih[dir];
    float* gh = g_bhh[dir];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float sr = row_sum(r[e]), sz = row_sum(z[e]), sn = row_sum(n[e]), sq = row_sum(q[e]);
      if (i == 0) {
        atomicAdd(&gi[j0 + e], sr);
        atomicAdd(&gh[j0 + e], sr);
        atomicAdd(&gi[H + j0 + e], sz);
        atomicAdd(&gh[H + j0 + e], sz);
        atomicAdd(&gi[2 * H + j0 + e], sn);
        atomicAdd(&gh[2 * H + j0 + e], sq);
      }
    }
  }
};

}  // namespace
