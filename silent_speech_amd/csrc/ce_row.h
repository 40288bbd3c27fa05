// CrossEntropyLoss(weight=, label_smoothing=) of ONE logit row (train_model_official.py:405 and the class-weighted form of
// :406-414): the loss, d(loss)/d(logits) and the arg-max, shared by ce_ls_kernel (pool_head.hip), eval_accum_kernel (eval.hip)
// and the CE block of tail_fwd_kernel (tail.hip) and by their class-weighted and mixup entry points.
//
// Row with label y, log-softmax lp, p = exp(lp), smoothing eps, C classes, class weights w:
//   loss      = (1 - eps) * (-w[y] * lp[y]) + (eps / C) * (-sum_c w[c] * lp[c])                      (un-normalised)   ce_label_loss
//   d logit_c = [ p_c * A - tgt_c ] / denom,  tgt_c = (c == y) * (1 - eps) * w[y] + (eps / C) * w[c]                   ce_tgt
//               A = w[y] + eps * (sum_k w[k] / C - w[y])                                                               ce_a
// (A is (1 - eps) * w[y] + (eps / C) * sum_k w[k], written so that w == 1 gives exactly 1).
// Each of the three is written once, below, as a function of one label; the row functions call it for y and, under MIX, for yb.
//
// WEIGHTED = false is the arithmetic the three kernels have always done -- the same operations in the same order, so their
// results keep their bits -- and never touches w (A is the constant 1).  WEIGHTED = true with every w[c] == 1.0f gives the same
// bits again: each weight enters as a factor of a product whose other factor is the unweighted term (x * 1 and fma(x, 1, s)
// round like x and s + x), sum_k w[k] = C exactly, A = 1 exactly.
//
// MIX = true is the two-label loss of a mixup batch (ss_ce_ls_mix_fwd_bwd, ss_tail_fwd_mix): labels y and yb, one factor lam,
//   loss      = lam * loss(y) + (1 - lam) * loss(yb),
//   d logit_c = [ p_c * A_mix - tgt_mix_c ] / denom,  tgt_mix = lam * tgt(y) + (1 - lam) * tgt(yb),  A_mix the same blend of the As
// (unweighted: A = 1 for both labels, so A_mix = 1 and is not blended).  MIX = false is every operation the row has always had, in
// its order; MIX = true with lam == 1 gives those bits again (1 * x + 0 * z is x, fused or not, for finite z).
//
// KD = true adds a teacher's soft targets (ss_ce_ls_kd_fwd_bwd, ss_tail_fwd_kd): teacher logits t, temperature tau > 0, weight
// alpha in [0, 1]; q = softmax(z / tau), pt = softmax(t / tau), lq and lpt their logs,
//   loss      = (1 - alpha) * hard / hard_norm        + alpha * tau^2 * KL(pt || q) / denom,   KL = sum_c pt_c * (lpt_c - lq_c)
//   d logit_c = (1 - alpha) * hard_grad_c / hard_norm + alpha * tau * (q_c - pt_c) / denom.
// `hard` is everything above (smoothing, weights, both labels) over its own normaliser (denom, or *den with weights); the soft
// term is never class-weighted and always over CeKd::denom, the global clip count (kl_div's "batchmean" under data parallelism),
// so a weighted launch carries that count as well.  The KL is taken from the two LOG-softmaxes, never from the log of a
// probability: a pt_c that underflows to 0 adds 0 * finite = 0.  Both softmaxes go through ONE pair of helpers (ce_lsm_tau /
// ce_lsm_tau_wave and ce_lp_tau), called once for z and once for t, so t == z gives equal bits, q - pt = 0 and KL = 0 exactly.
// The row has no label in the soft term, so it composes with WEIGHTED and MIX; the label rule is unchanged and a row that does
// not count gets nothing, soft term included.  The teacher logits must be finite: the caller vouches for it, as the plain path
// does for its labels.  KD = false is every operation the row has always had, in its order (kd is not read); KD = true with
// alpha == 0 gives those bits again, gradient row and loss alike: each output is (1 - alpha) * x + alpha * k with x the old
// value, and 1 * x + 0 * k is x, fused or not, for finite k (ce_kd_blend).
//
// Two forms, because the callers spread a row differently: ce_row (one thread walks the row) and ce_row_wave (the 64 lanes of a
// wave share it, classes lane, lane + 64, ...).  They differ in the order of their C-term sums, as the kernels always have.
//
// A launch's loss is one CeLoss, what it means for row b one CeRow (ce_row_of); ce_dispatch picks <WEIGHTED, MIX, KD> on the host.
#pragma once
#include <type_traits>

#include "ss_common.h"

// The loss of a launch.  cw / den (both or neither): class weights, and the device float *den divides instead of `denom`;
// y_b / lam (both or neither): the two-label loss, the factor read from the device.  y == NULL: no loss (tail).
struct CeLoss { const int64_t *y, *y_b; const float *lam, *cw, *den; float denom, ls; };
// Row b of a CeLoss: does it count, its labels as indices, the mixing factor and the normaliser.
struct CeRow { bool counts; int yy, yb; float lam, denom; };

// The soft targets of a launch (KD): t (B, ld_t) teacher logits, the blend alpha, the temperature tau and the soft term's
// normaliser, the global clip count.  Apart from CeLoss, so that a kernel can take it where its other instantiations never look.
struct CeKd { const float* t; int ld_t; float alpha, tau, denom; };

// Host: what both _kd entry points require of their soft targets (NaN fails every comparison)
static inline bool ce_kd_ok(const float* t, int ld_t, int C, float alpha, float tau, float denom) {
  return t && ld_t >= C && alpha >= 0.f && alpha <= 1.f && tau > 0.f && tau <= 3.4e38f && denom > 0.f;
}

__device__ __forceinline__ bool ce_label_ok(int64_t label, int C) { return label >= 0 && label < (int64_t)C; }

template <bool WEIGHTED>
__device__ __forceinline__ float ce_denom(const CeLoss& l) { if constexpr (WEIGHTED) return l.den[0]; else return l.denom; }

// THE label rule.  plain (neither weights nor mixup): the label is not looked at -- the caller vouches for 0 <= y < C, as it
// always has;  WEIGHTED: the row counts iff 0 <= y < C;  MIX (weighted or not): iff 0 <= y < C and 0 <= y_b < C.
// A row that does not count gets a zero gradient row and adds nothing to the loss or the hit count (its labels come back as 0:
// not to be used).  `denom` = ce_denom of the loss: *den with weights, its `denom` without; lam is *lam under MIX, 1 otherwise.
// (eval_accum_kernel applies ce_label_ok to every row, weighted or not, and raises its flag: it has no caller to vouch.)
template <bool WEIGHTED, bool MIX>
__device__ __forceinline__ CeRow ce_row_of(const int64_t* __restrict__ y, const int64_t* __restrict__ y_b,
                                           const float* __restrict__ lam, float denom, int b, int C) {
  CeRow r = {true, 0, 0, 1.0f, denom};
  if constexpr (MIX) {
    r.counts = ce_label_ok(y[b], C) && ce_label_ok(y_b[b], C);
    r.yb = r.counts ? (int)y_b[b] : 0;
    r.lam = lam[0];
  } else if constexpr (WEIGHTED) {
    r.counts = ce_label_ok(y[b], C);
  }
  r.yy = r.counts ? (int)y[b] : 0;
  return r;
}

// ---- the three formulas, each for ONE label `l` with weight wl = w[l] (unweighted: w is not read, wl is ignored);
// lse - logit_l = -lp[l], slp = sum_c w[c] * lp[c], sw = sum_k w[k]
template <bool WEIGHTED>
__device__ __forceinline__ float ce_tgt(int c, int l, float wl, const float* __restrict__ w, float eps, int C) {
  if constexpr (WEIGHTED) return (c == l ? (1.0f - eps) * wl : 0.f) + (eps / C) * w[c];
  else return (c == l ? (1.0f - eps) : 0.f) + eps / C;
}
template <bool WEIGHTED>
__device__ __forceinline__ float ce_label_loss(float lse, float logit_l, float wl, float slp, float eps, int C) {
  if constexpr (WEIGHTED) return (1.0f - eps) * (wl * (lse - logit_l)) + eps * (-slp / C);
  else return (1.0f - eps) * (lse - logit_l) + eps * (-slp / C);
}
template <bool WEIGHTED>
__device__ __forceinline__ float ce_a(float wl, float sw, float eps, int C) {
  if constexpr (WEIGHTED) return wl + eps * (sw / C - wl);
  else return 1.0f;
}

// ---- softmax at temperature (KD): the ONE code path of both the student's and the teacher's row.
// ce_lsm_tau[_wave] -> the row's maximum *m_out and log(sum_c exp((x_c - m) / tau)); ce_lp_tau: log softmax(x / tau)_c from them.
__device__ __forceinline__ float ce_lsm_tau(const float* __restrict__ x, int C, float tau, float* m_out) {
  float m = x[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf((x[c] - m) / tau);
  *m_out = m;
  return logf(se);
}
__device__ __forceinline__ float ce_lsm_tau_wave(const float* x, int C, int lane, float tau, float* m_out) {
  float m = -3.4e38f;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf((x[c] - m) / tau);
  *m_out = m;
  return logf(wave_sum(se));
}
__device__ __forceinline__ float ce_lp_tau(float x, float m, float tau, float ls) { return (x - m) / tau - ls; }
// class c of the soft term: its KL summand is added to *kl, its gradient tau * (q_c - pt_c) / denom returned
__device__ __forceinline__ float ce_kd_class(float z, float mz, float lsz, float t, float mt, float lst, const CeKd& kd, float* kl) {
  const float lq = ce_lp_tau(z, mz, kd.tau, lsz), lpt = ce_lp_tau(t, mt, kd.tau, lst);
  const float q = expf(lq), pt = expf(lpt);
  *kl += pt * (lpt - lq);
  return kd.tau * (q - pt) / kd.denom;
}
// (1 - alpha) * hard + alpha * soft: with alpha == 0 the bits of `hard` (header)
__device__ __forceinline__ float ce_kd_blend(float hard, float soft, float alpha) { return (1.0f - alpha) * hard + alpha * soft; }
// what a row adds to the launch's loss sum: loss / its normaliser, under KD blended with the soft term tau^2 * KL / kd.denom
template <bool KD>
__device__ __forceinline__ float ce_row_loss(float loss, float denom, float kl, const CeKd& kd) {
  if constexpr (KD) return ce_kd_blend(loss / denom, kd.tau * kd.tau * kl / kd.denom, kd.alpha);
  else return loss / denom;
}

// One thread per row.  lr = the row's C logits, r = ce_row_of a row that counts (without MIX r.yb and r.lam are not read).
// d_row (may be NULL): the gradient row / r.denom; *am_out: the lowest index among equal maxima (torch.argmax).  Returns the loss, undivided.
// KD: tr = the row's teacher logits; d_row gets the blended gradient and *kl_out the row's KL (ce_row_loss blends the loss).
template <bool WEIGHTED, bool MIX = false, bool KD = false>
__device__ __forceinline__ float ce_row(const float* __restrict__ lr, int C, float eps, const float* __restrict__ w,
                                        const CeRow& r, float* __restrict__ d_row, int* am_out, const CeKd& kd = CeKd{},
                                        const float* __restrict__ tr = nullptr, float* kl_out = nullptr) {
  const int yy = r.yy, yb = r.yb;
  const float lam = r.lam, oml = 1.0f - r.lam;  // (MIX only)
  float m = lr[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (lr[c] > m) { m = lr[c]; am = c; }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(lr[c] - m);
  const float lse = m + logf(se);
  float slp = 0.f, sw = 0.f, wy = 1.f, wyb = 1.f;
  if constexpr (WEIGHTED) {
    wy = w[yy];
    for (int c = 0; c < C; ++c) {
      slp += w[c] * (lr[c] - lse);
      sw += w[c];
    }
  } else {
    for (int c = 0; c < C; ++c) slp += lr[c] - lse;
  }
  if constexpr (WEIGHTED && MIX) wyb = w[yb];
  float loss = ce_label_loss<WEIGHTED>(lse, lr[yy], wy, slp, eps, C);
  if constexpr (MIX) loss = lam * loss + oml * ce_label_loss<WEIGHTED>(lse, lr[yb], wyb, slp, eps, C);
  float mz = 0.f, lsz = 0.f, mt = 0.f, lst = 0.f, kl = 0.f;  // (KD only)
  if constexpr (KD) {
    lsz = ce_lsm_tau(lr, C, kd.tau, &mz);
    lst = ce_lsm_tau(tr, C, kd.tau, &mt);
  }
  if (d_row) {
    float a = ce_a<WEIGHTED>(wy, sw, eps, C);
    if constexpr (WEIGHTED && MIX) a = lam * a + oml * ce_a<WEIGHTED>(wyb, sw, eps, C);
    for (int c = 0; c < C; ++c) {
      const float pr = expf(lr[c] - lse);
      float tgt = ce_tgt<WEIGHTED>(c, yy, wy, w, eps, C);
      if constexpr (MIX) tgt = lam * tgt + oml * ce_tgt<WEIGHTED>(c, yb, wyb, w, eps, C);
      if constexpr (KD) d_row[c] = ce_kd_blend((pr * a - tgt) / r.denom, ce_kd_class(lr[c], mz, lsz, tr[c], mt, lst, kd, &kl), kd.alpha);
      else d_row[c] = (pr * a - tgt) / r.denom;
    }
  } else if constexpr (KD) {
    for (int c = 0; c < C; ++c) ce_kd_class(lr[c], mz, lsz, tr[c], mt, lst, kd, &kl);
  }
  if constexpr (KD) *kl_out = kl;
  *am_out = am;
  return loss;
}

// One wave per row; every lane of the wave calls it.  lg = the row's C logits (LDS or global), lane = 0..63, r as in ce_row.
// d_row (not NULL) gets the gradient row / r.denom.  Returns the row's loss, not divided, and the arg-max in *am_out (every lane).
// KD: tr = the row's teacher logits; d_row gets the blended gradient and *kl_out (every lane) the row's KL.
template <bool WEIGHTED, bool MIX = false, bool KD = false>
__device__ __forceinline__ float ce_row_wave(const float* lg, int C, int lane, float eps, const float* __restrict__ w,
                                             const CeRow& r, float* __restrict__ d_row, int* am_out, const CeKd& kd = CeKd{},
                                             const float* __restrict__ tr = nullptr, float* kl_out = nullptr) {
  const int yy = r.yy, yb = r.yb;
  const float lam = r.lam, oml = 1.0f - r.lam;  // (MIX only)
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
  float se = 0.f, sl = 0.f, sw = 0.f, wy = 1.f, wyb = 1.f;
  for (int c = lane; c < C; c += 64) se += expf(lg[c] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  if constexpr (WEIGHTED) {
    for (int c = lane; c < C; c += 64) {
      sl += w[c] * (lg[c] - lse);
      sw += w[c];
    }
    sl = wave_sum(sl);
    sw = wave_sum(sw);
    wy = w[yy];
    if constexpr (MIX) wyb = w[yb];
  } else {
    for (int c = lane; c < C; c += 64) sl += lg[c] - lse;
    sl = wave_sum(sl);
  }
  float a = ce_a<WEIGHTED>(wy, sw, eps, C);
  if constexpr (WEIGHTED && MIX) a = lam * a + oml * ce_a<WEIGHTED>(wyb, sw, eps, C);
  float mz = 0.f, lsz = 0.f, mt = 0.f, lst = 0.f, kl = 0.f;  // (KD only)
  if constexpr (KD) {
    lsz = ce_lsm_tau_wave(lg, C, lane, kd.tau, &mz);
    lst = ce_lsm_tau_wave(tr, C, lane, kd.tau, &mt);
  }
  for (int c = lane; c < C; c += 64) {
    const float pr = expf(lg[c] - lse);
    float tgt = ce_tgt<WEIGHTED>(c, yy, wy, w, eps, C);
    if constexpr (MIX) tgt = lam * tgt + oml * ce_tgt<WEIGHTED>(c, yb, wyb, w, eps, C);
    if constexpr (KD) d_row[c] = ce_kd_blend((pr * a - tgt) / r.denom, ce_kd_class(lg[c], mz, lsz, tr[c], mt, lst, kd, &kl), kd.alpha);
    else d_row[c] = (pr * a - tgt) / r.denom;
  }
  if constexpr (KD) *kl_out = wave_sum(kl);
  float loss = ce_label_loss<WEIGHTED>(lse, lg[yy], wy, sl, eps, C);
  if constexpr (MIX) loss = lam * loss + oml * ce_label_loss<WEIGHTED>(lse, lg[yb], wyb, sl, eps, C);
  *am_out = am;
  return loss;
}

// Host: f(std::bool_constant<WEIGHTED>, std::bool_constant<MIX>, std::bool_constant<KD>) for a loss with class weights
// (cw != NULL), second labels (y_b != NULL) and / or teacher logits (t != NULL): the one if-ladder over the instantiations of
// tail_fwd_kernel and ce_ls_kernel.  (Evaluation is the hard loss: eval.hip has no soft targets.)
template <class F>
static inline void ce_dispatch(const void* cw, const void* y_b, const void* t, F&& f) {
  auto kd = [&](auto w, auto m) {
    if (t) f(w, m, std::true_type{});
    else f(w, m, std::false_type{});
  };
  if (cw && y_b) kd(std::true_type{}, std::true_type{});
  else if (y_b) kd(std::false_type{}, std::true_type{});
  else if (cw) kd(std::true_type{}, std::false_type{});
  else kd(std::false_type{}, std::false_type{});
}
