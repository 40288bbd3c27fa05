// Validation state kept on the device (train_model_official.py:449-475, 79-91): per batch ONE launch adds the clips'
// losses, the hit count, the confusion matrix and the position at which every (true, predicted) cell first occurred.
// Every accumulator reduces over ranks with one collective (sum, sum, min), and nothing is read back per batch.
#include "ss_common.h"
#include "ce_row.h"

namespace {

// one thread per clip (C is a handful of words).  The per-clip arithmetic is ce_row (ce_row.h), the function ce_ls_kernel
// (pool_head.hip) calls, with denom = 1 -- same order of operations, expf / logf, lowest index among equal maxima -- so a
// batch of one wave gives the bits ss_ce_ls_fwd_bwd gives.  What differs: a label outside [0, C) is never an index -- every row
// passes ce_label_ok, the range check of ce_row_of, weighted or not -- and such a row raises err_flag.
// WEIGHTED: the class-weighted loss, and wsum += sum of w[y] over the rows that count.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void eval_accum_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                         int B, int C, float eps, int first_row,
                                                         const float* __restrict__ w, float* __restrict__ wsum,
                                                         float* __restrict__ loss_sum, int* __restrict__ correct,
                                                         int* __restrict__ confusion, int* __restrict__ first_seen,
                                                         int* __restrict__ y_true_out, int* __restrict__ y_pred_out,
                                                         int* __restrict__ err_flag) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  float loss = 0.f, wy = 0.f;
  if (b < B) {
    const int64_t label = y[b];
    int yy = -1, am = -1;
    if (ce_label_ok(label, C)) {
      yy = (int)label;
      loss = ce_row<WEIGHTED>(logits + (long)b * C, C, eps, w, CeRow{true, yy, 0, 1.0f, 1.0f}, nullptr, &am);
      if constexpr (WEIGHTED) wy = w[yy];
      const long cell = (long)yy * C + am;
      atomicAdd(&confusion[cell], 1);
      atomicMin(&first_seen[cell], first_row + b);
      if (am == yy) atomicAdd(correct, 1);
    } else {
      *err_flag = 1;  // the row adds nothing anywhere
    }
    if (y_true_out) y_true_out[b] = yy;
    if (y_pred_out) y_pred_out[b] = am;
  }
  loss = wave_sum(loss);  // every lane of the workgroup arrives here
  if constexpr (WEIGHTED) wy = wave_sum(wy);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(loss_sum, loss);
    if constexpr (WEIGHTED) atomicAdd(wsum, wy);
  }
}

}  // namespace

// both entry points: what they both check, and the launch (w == NULL: the unweighted loss, wsum is not touched)
static int eval_accum_launch(const float* logits, const int64_t* y, int B, int C, float label_smoothing, int first_row,
                             const float* w, float* loss_sum, float* wsum, int32_t* correct, int32_t* confusion, int32_t* first_seen,
                             int32_t* y_true_out, int32_t* y_pred_out, int32_t* err_flag, ss_stream_t stream) {
  SS_REQUIRE(logits && y && loss_sum && correct && confusion && first_seen && err_flag, SS_ERR_ARG);
  SS_REQUIRE(B > 0 && C > 0 && first_row >= 0, SS_ERR_ARG);
  SS_REQUIRE((long)first_row + (long)B <= 2147483647L, SS_ERR_ARG);  // first_row + b stays an int32
  const int blocks = (int)(((long)B + 255) / 256);
  hipLaunchKernelGGL(w ? eval_accum_kernel<true> : eval_accum_kernel<false>, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), logits, y, B, C, label_smoothing, first_row, w, wsum, loss_sum, correct,
                     confusion, first_seen, y_true_out, y_pred_out, err_flag);
  return ss_launch_status();
}

extern "C" int ss_eval_accum(const float* logits, const int64_t* y, int B, int C, float label_smoothing, int first_row,
                             float* loss_sum, int32_t* correct, int32_t* confusion, int32_t* first_seen,
                             int32_t* y_true_out, int32_t* y_pred_out, int32_t* err_flag, ss_stream_t stream) {
  return eval_accum_launch(logits, y, B, C, label_smoothing, first_row, nullptr, loss_sum, nullptr, correct, confusion, first_seen,
                           y_true_out, y_pred_out, err_flag, stream);
}

extern "C" int ss_eval_accum_w(const float* logits, const int64_t* y, int B, int C, float label_smoothing, int first_row,
                               const float* w, float* loss_sum, float* wsum, int32_t* correct, int32_t* confusion,
                               int32_t* first_seen, int32_t* y_true_out, int32_t* y_pred_out, int32_t* err_flag,
                               ss_stream_t stream) {
  SS_REQUIRE(w && wsum, SS_ERR_ARG);
  return eval_accum_launch(logits, y, B, C, label_smoothing, first_row, w, loss_sum, wsum, correct, confusion, first_seen,
                           y_true_out, y_pred_out, err_flag, stream);
}
