/* ss_hotpath.h -- C ABI of the MI355X (gfx950) Silent-Speech per-clip hot path.
 *
 * The reference (davdwan21/Silent-Speech) has no FFI: its path sits behind a Python nn.Module
 * (train_model_official.py:253-310), NumPy helpers (record_landmarks_official.py:52-118,
 * live_infer_official.py:141-187) and torch's optimiser/loss objects
 * (train_model_official.py:403-405, 433-439).  This header is the boundary a maintainer would
 * bind with ctypes: plain device pointers and sizes, no torch types.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless a comment says otherwise; buffers are borrowed for
 *    the duration of the call (asynchronously: until the work enqueued on `stream` has finished);
 *  - no entry point allocates, frees or synchronises; workspaces are passed in, so every call is
 *    capturable into a hipGraph;
 *  - `stream` is a hipStream_t (0 = the default stream); calls are re-entrant per stream;
 *  - return value: 0 (SS_OK) or a negative ss_status; the Python shim raises RuntimeError on != 0;
 *  - all floating-point buffers are fp32 row-major unless stated; gate order everywhere is
 *    torch's r | z | n.
 */
#ifndef SS_HOTPATH_H
#define SS_HOTPATH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ss_stream_t; /* hipStream_t */

enum ss_status {
  SS_OK = 0,
  SS_ERR_ARG = -1,         /* null pointer / non-positive size / inconsistent flags */
  SS_ERR_LAUNCH = -2,      /* hipGetLastError() after the launch was not hipSuccess */
  SS_ERR_UNSUPPORTED = -3  /* shape outside what the kernels are built for (e.g. hidden size) */
};

/* ABI version, bumped on any signature change. */
int ss_abi_version(void);
const char* ss_status_string(int status);

/* ---- a1: per-frame landmark feature fuse -------------------------------------------------
 * replaces extract_feature + mouth_width_px (record_landmarks_official.py:52-100;
 * live_infer_official.py:141-169).
 * lm      (B,T,K,2) MediaPipe-normalised x,y of the K selected landmarks
 * reset   (B,T) uint8 or NULL: non-zero = the velocity state prev_xy is None at that frame
 *         (t == 0 always resets)
 * a_*     positions of landmarks 61, 291, 13, 14 inside the K-list
 * variant 0 = recorder arithmetic (mouth width in float64), 1 = live (float32 points)
 * X       (B,T, ldx>=2K+4): [x0,y0,...,vel,open_px,width_px,aspect]
 * center  (B,T,2) float32 pixel centre; fourth (B,T) float64: width+1e-6 (recorder) or width (live) */
int ss_feature_fuse(const float* lm, const uint8_t* reset, int B, int T, int K, int w, int h, int a_left,
                    int a_right, int a_up, int a_lo, int variant, float* X, int ldx, float* center,
                    double* fourth, ss_stream_t stream);

/* The live chain's front for n DISTINCT streams, one frame each (live_infer_official.py:264-296): the distance gate
 * band_lo <= mouth_w <= band_hi (MOUTH_W_MIN_PX / MAX_PX, :23-24, :272) decides whether a frame is KEPT; a kept frame gets
 * extract_feature with the stream's velocity state, a dropped frame of a recording stream clears that state (:295-296), so the
 * first kept frame after re-entry has vel = 0.  State, resident in HBM, zero-initialised by the caller: prev_lm (S,K,2) = raw
 * landmarks of the stream's previous kept frame, has_prev (S) u8.  recording (n) u8 or NULL (= all recording): 0 leaves the
 * stream untouched (``if recording`` false).  Outputs per frame i: X row (zeros when dropped), center, fourth (as
 * ss_feature_fuse), kept[i].  stream_ids must be distinct and in [0, n_streams) -- the caller checks. */
int ss_feature_fuse_stream(const float* lm, const int32_t* stream_ids, const uint8_t* recording, int n, int n_streams, int K,
                           int w, int h, int a_left, int a_right, int a_up, int a_lo, int variant, double band_lo,
                           double band_hi, float* prev_lm, uint8_t* has_prev, float* X, int ldx, float* center,
                           double* fourth, uint8_t* kept, ss_stream_t stream);

/* ---- a4 + a5 for ANY ROI size (csrc/roi_cnn_generic.hip): the building blocks of the layer-by-layer form the host sequences for
 * frame sizes outside the fused kernels' set (ss_roi_cnn_stash_size returns SS_ERR_UNSUPPORTED for them): every 3x3 convolution is
 * ss_im2col3x3 + ss_gemm_f32_batched against nn.Conv2d's weight as it stands ((Cout, C, 3, 3) = [n][k], k = c*9 + ky*3 + kx).
 *   ss_roi_norm    R (N, HW) u8 -> xn (N, HW) f32 = (u/255 - mu)/sd (train_model_official.py:286-291; standardize 0: u/255);
 *                  stats (N, 2) = mu, sd or NULL
 *   ss_im2col3x3   src (N, C, H, W) planar -> col (N H W, ld_col >= 9 C), zero padding at the borders and in columns [9 C, ld_col)
 *   ss_relu_pool2  y (N H W, C) pixel-major pre-activation -> a (N, C, H/2, W/2) = maxpool(relu(y)), idx = winner of the 2x2 window
 *                  (0..3 row-major, the first on ties)
 *   ss_relu_mean   y (N P, C) -> feat (N, C) = mean over the P pixels of relu(y); mask (N P, C) = y > 0 (NULL: not written)
 *   ss_mask_scale  dy (N P, C) = mask ? dfeat[n][c] / P : 0
 *   ss_col2im3x3   dcol (N H W, ld_col) -> d (N, C, H, W): the transposed convolution's gather
 *   ss_pool2_bwd   da, a, idx (N, C, H2, W2) -> dy (N 2H2 2W2, C) pixel-major: the winner gets da where a > 0, zeros elsewhere */
int ss_roi_norm(const uint8_t* R, int N, int HW, int standardize, float* xn, float* stats, ss_stream_t stream);
int ss_im2col3x3(const float* src, int N, int C, int H, int W, float* col, int ld_col, ss_stream_t stream);
int ss_relu_pool2(const float* y, int N, int C, int H, int W, float* a, uint8_t* idx, ss_stream_t stream);
int ss_relu_mean(const float* y, int N, int P, int C, float* feat, uint8_t* mask, ss_stream_t stream);
int ss_mask_scale(const uint8_t* mask, const float* dfeat, int N, int P, int C, float* dy, ss_stream_t stream);
int ss_col2im3x3(const float* dcol, int ld_col, int N, int C, int H, int W, float* d, ss_stream_t stream);
int ss_pool2_bwd(const float* da, const float* a, const uint8_t* idx, int N, int C, int H2, int W2, float* dy, ss_stream_t stream);

/* ---- a2: ROI crop rectangle ---------------------------------------------------------------
 * replaces the index arithmetic of crop_roi (record_landmarks_official.py:106-114, variant 0) and
 * crop_roi_gray (live_infer_official.py:172-181, variant 1).  Bit-exact integers.
 * box (n,5) int32: x1, x2, y1, y2, valid */
int ss_roi_crop_idx(const float* center, const double* scale, int n, int w, int h, int variant, int32_t* box,
                    ss_stream_t stream);

/* ---- a2: crop -> BGR2GRAY -> resize behind the crop box --------------------------
 * replaces cv2.cvtColor + cv2.resize in crop_roi (record_landmarks_official.py:116-118, INTER_LINEAR: interp 0) and
 * crop_roi_gray (live_infer_official.py:184-186, INTER_AREA: interp 1).  frames_bgr (N,h,w,3) u8, box (N,5) from
 * ss_roi_crop_idx, out (N,roi_h,roi_w) u8 (zeros where the box is invalid).  OpenCV's 8-bit algorithms restated;
 * parity with OpenCV itself is unpinned: +-1 grey level is the contract. */
int ss_crop_gray_resize(const uint8_t* frames_bgr, int N, int h, int w, const int32_t* box, int roi_h, int roi_w,
                        int interp, uint8_t* out, ss_stream_t stream);

/* ---- a4+a5(+a6): ROI normalise + TinyROICNN, fused ------------------------------------------
 * replaces train_model_official.py:286-291 and TinyROICNN.forward (:212-229); with
 * standardize = 0 the live variant (live_infer_official.py:126-127).
 * R    (N,H,W) uint8 raw 0..255;  H, W multiples of 4 (two 2x2 pools)
 * w1 (8,1,3,3) b1 (8) w2 (16,8,3,3) b2 (16) w3 (24,16,3,3) b3 (24) wfc (E,24) bfc (E), E <= 64
 * out  row n written at out + n*ld_out, E floats (pass Z + x_dim with ld_out = x_dim+E to fuse
 *      the torch.cat of train_model_official.py:297) */
int ss_roi_cnn_fwd(const uint8_t* R, int N, int H, int W, int standardize, const float* w1, const float* b1,
                   const float* w2, const float* b2, const float* w3, const float* b3, const float* wfc,
                   const float* bfc, int E, float* out, int ld_out, ss_stream_t stream);

/* Workgroups the two persistent ROI-CNN kernels launch (default 256 = one per CU; 0 restores the default).
 * A caller that runs a second stream beside them (micro-batch pipelining) leaves CUs free this way. */
int ss_roi_cnn_set_max_workgroups(int n);

/* per-frame sizes of the six stash arrays for an (H, W) the kernels are built for, sizes[6] (host memory) =
 * { floats of the pooled-1 map, floats of the pooled-2 map, bytes of the pool-1 argmax map (padded planes), bytes of the
 *   pool-2 argmax map, bytes of the conv3 sign mask, floats of an st_feat row } */
#define SS_ROI_CNN_STASH_SIZES 6
int ss_roi_cnn_stash_size(int H, int W, int* sizes);

/* Same forward, additionally writing what the backward needs (the six st_* pointers are either
 * all NULL -- then this is ss_roi_cnn_fwd -- or all valid):
 * st_a1 (N, a1_floats) f32: the pooled conv1 map in the kernels' zero-haloed LDS layout (8 planes of
 *   (H/2+2) rows x (W/2+2) floats, plane stride padded; sizes from ss_roi_cnn_stash_size) so that the backward
 *   streams it back with linear 16-byte copies; st_i1 (N, i1_bytes) u8: its 2x2 argmax (0..3, row-major window),
 *   8 planes of Geom::I1S = H/2*W/2 bytes;
 * st_a2 (N, a2_floats) f32 and st_i2 (N,H/4,W/4,16) u8 (pixel-major): the same for conv2;
 * st_m3 (N,H/4*W/4,32) u8, pixel-major, channels 24..31 zero: conv3 output > 0; st_feat (N,52): globally averaged conv3 features, then the
 * per-channel counts of positive conv3 outputs, then the mean and the standard deviation of the frame (the backward kernel reuses them).
 * stash_sizes (host memory, 6 ints; may be NULL when the st_* are): the per-frame sizes the caller allocated the six arrays
 *   with (what ss_roi_cnn_stash_size returned).  The forward and the backward kernel each compare ALL of them with the
 *   layout THEY were compiled with and return SS_ERR_ARG on a mismatch instead of writing / reading out of bounds (round 1
 *   lost a GPU process to two objects built against different versions of that layout: DESIGN.md section 9). */
int ss_roi_cnn_fwd_stash(const uint8_t* R, int N, int H, int W, int standardize, const float* w1, const float* b1,
                         const float* w2, const float* b2, const float* w3, const float* b3, const float* wfc,
                         const float* bfc, int E, float* out, int ld_out, float* st_a1, uint8_t* st_i1,
                         float* st_a2, uint8_t* st_i2, uint8_t* st_m3, float* st_feat, const int* stash_sizes,
                         ss_stream_t stream);

/* autograd of the above w.r.t. the eight parameter tensors (the uint8 input has no gradient),
 * i.e. what loss.backward() (train_model_official.py:437) leaves in roi_cnn.*.grad.
 * d_out row n read at d_out + n*ld_dout (E floats).  Gradients are ACCUMULATED (+=) into g_*.
 * Needs the stash of ss_roi_cnn_fwd_stash for the same R and weights. */
int ss_roi_cnn_bwd(const uint8_t* R, int N, int H, int W, int standardize, const float* w1, const float* b1,
                   const float* w2, const float* b2, const float* w3, const float* b3, const float* wfc,
                   const float* bfc, int E, const float* st_a1, const uint8_t* st_i1, const float* st_a2,
                   const uint8_t* st_i2, const uint8_t* st_m3, const float* st_feat, const int* stash_sizes,
                   const float* d_out, int ld_dout, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3,
                   float* g_wfc, float* g_bfc, ss_stream_t stream);

/* ---- padded batches: only the frames that belong to a clip ---------------------------------
 * The reference pads every clip to T frames and runs TinyROICNN over all B*T of them (train_model_official.py:286-297) although
 * pack_padded_sequence (:300) drops rows t >= lengths[b] before the recurrence: their embeddings never reach the logits and
 * their gradient is exactly zero.  ss_roi_active_frames lists the rows that count -- frames[0] = how many, frames[1 ...] = the
 * row numbers b*T + t with t < min(max(lengths[b], 0), T), ascending; frames needs 1 + B*T ints of device memory -- and, when
 * emb is given, clears emb[row*ld_emb + 0 .. emb_cols) of every other row (pass Z + x_dim: the input-projection GEMM still
 * reads those rows).  ss_roi_cnn_fwd_frames / ss_roi_cnn_bwd_frames are ss_roi_cnn_fwd_stash / ss_roi_cnn_bwd walking only the
 * listed frames (frames == NULL: all N); `out` rows and stash slots stay indexed by the frame number, so the two launches of a
 * step must be given the same list.  Logits and gradients are those of the full walk. */
int ss_roi_active_frames(const int32_t* lengths, int B, int T, int* frames, float* emb, int ld_emb, int emb_cols,
                         ss_stream_t stream);
int ss_roi_cnn_fwd_frames(const uint8_t* R, int N, int H, int W, int standardize, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* w3, const float* b3, const float* wfc,
                          const float* bfc, int E, float* out, int ld_out, float* st_a1, uint8_t* st_i1,
                          float* st_a2, uint8_t* st_i2, uint8_t* st_m3, float* st_feat, const int* stash_sizes,
                          const int* frames, ss_stream_t stream);
int ss_roi_cnn_bwd_frames(const uint8_t* R, int N, int H, int W, int standardize, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* w3, const float* b3, const float* wfc,
                          const float* bfc, int E, const float* st_a1, const uint8_t* st_i1, const float* st_a2,
                          const uint8_t* st_i2, const uint8_t* st_m3, const float* st_feat, const int* stash_sizes,
                          const float* d_out, int ld_dout, float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* g_w3,
                          float* g_b3, float* g_wfc, float* g_bfc, const int* frames, ss_stream_t stream);

/* ---- dense contraction used by a7/a9 and their gradients -----------------------------------
 * C[M,N] (+)= opA[M,K] * opB[K,N] (+ bias[N]) (then ReLU), exact-f32 MFMA.
 * a_kcontig = 1: A is stored [M][K] (lda = row stride); 0: stored [K][M].
 * b_kcontig = 1: B is stored [N][K] (torch Linear weight layout); 0: stored [K][N].
 * *_group/_gstride/_off remap the storage ROW index r of that operand to
 *   (r / group) * gstride + (r % group) + off   (identity: group = INT32_MAX, off = 0);
 *   used to pair dG[b][t] with h[b][t-1] without materialising a shifted copy.
 * a_colsum (may be NULL; needs a_kcontig = 0): a_colsum[m] += sum_k A[k][m] -- the bias gradient of a
 *   Linear layer rides on its weight-gradient GEMM instead of a separate reduction pass.
 * flags bit0: accumulate into C; bit1: ReLU epilogue; bit2: accumulate with float atomics even when K is not
 * split (several streams add into one C).  splits > 1 slices K over blockIdx.z and adds with float atomics
 * (atomics require bit0, C pre-initialised, no ReLU).
 * flags bit4 (ss_gemm_f32_batched only): the `batch` problems are SUMMED into one C (stride_c ignored) -- the K loop of a
 * workgroup runs through all (A, B) pairs, so e.g. d layer_in = dG_fwd W_fwd + dG_rev W_rev needs neither atomics nor a cleared C.
 * flags bit3 (alone; no bias): C is a split-K workspace of ss_gemm_splitk_ws_floats() floats (16-byte aligned) instead of
 * the result: every workgroup leaves its raw accumulators there with plain stores and ss_gemm_splitk_reduce adds the
 * slices into the real C afterwards -- the weight-gradient GEMMs (M x N tiny, K = B*T) spend as long in float atomics
 * as in their K loop otherwise. */
int ss_gemm_f32(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, int lda, int a_group,
                int a_gstride, int a_off, const float* B, int ldb, int b_group, int b_gstride, int b_off,
                float* C, int ldc, const float* bias, float* a_colsum, int flags, int splits, ss_stream_t stream);

/* `batch` independent problems of identical shape in one launch (the two GRU directions): problem b uses
 * A + b*stride_a, B + b*stride_b, C + b*stride_c, bias + b*stride_bias, a_colsum + b*stride_colsum (element strides). */
int ss_gemm_f32_batched(int a_kcontig, int b_kcontig, int M, int N, int K, const float* A, int lda, int a_group,
                        int a_gstride, int a_off, const float* B, int ldb, int b_group, int b_gstride, int b_off,
                        float* C, int ldc, const float* bias, float* a_colsum, int flags, int splits, int batch,
                        long stride_a, long stride_b, long stride_c, long stride_bias, long stride_colsum,
                        ss_stream_t stream);

/* Second half of a split-K GEMM run with flags bit3: C[b][m][n] += sum over the K slices left in ws.  M, N, K, splits and
 * batch are those of the GEMM call; stride_c = element stride between the problems' C. */
int ss_gemm_splitk_ws_floats(int M, int N, int K, int splits, int batch, long* floats);
int ss_gemm_splitk_reduce(const float* ws, int M, int N, int K, int splits, int batch, float* C, int ldc, long stride_c,
                          ss_stream_t stream);

/* What a training step does before its first real kernel, in one launch: grads[0:n_grads] = 0 (the flat gradient bucket of
 * optimizer.zero_grad, train_model_official.py:433), scalars[0:n_scalars] = 0 and correct[0] = 0 (loss / sum of squares /
 * hit counter; correct may be NULL), lengths32[b] = lengths64[b] (NULL: skipped), Z[r][0:cols] = X[r][0:cols] for `rows`
 * rows (the landmark half of torch.cat((X, roi_emb)), train_model_official.py:297; X NULL: skipped); frames (may be NULL; needs
 * lengths64, X and rows = B*T): what ss_roi_active_frames does, from the int64 lengths, clearing Z[row][cols .. cols + emb_cols). */
int ss_train_prologue(float* grads, long n_grads, float* scalars, int n_scalars, int32_t* correct,
                      const int64_t* lengths64, int32_t* lengths32, int B, const float* X, int ld_x, float* Z, int ld_z,
                      int rows, int cols, int* frames, int emb_cols, ss_stream_t stream);

/* Several split-K problems C_j (ldc_j, stride_c_j between the batch members) += op(A_j) op(B_j) in ONE GEMM launch plus ONE
 * reduce launch (the three weight-gradient GEMMs of a GRU layer; every launch boundary on a stream costs the tail of one
 * kernel and the ramp of the next).  Fields as the arguments of ss_gemm_f32_batched; n <= 4; all problems of one operand
 * layout.  ws: ss_gemm_splitk_group_ws_floats() floats, 16-byte aligned, contents irrelevant. */
typedef struct ss_gemm_problem {
  int a_kcontig, b_kcontig, M, N, K;
  const float* A;
  int lda, a_group, a_gstride, a_off;
  const float* B;
  int ldb, b_group, b_gstride, b_off;
  float* C;
  int ldc, splits, batch;
  long stride_a, stride_b, stride_c;
} ss_gemm_problem;
int ss_gemm_splitk_group_ws_floats(const ss_gemm_problem* problems, int n, long* floats);
/* ws_floats = the floats the caller allocated at ws: the entry points recompute the layout and return SS_ERR_ARG when it does not fit
 * (a caller that sized ws for another group would otherwise be written past its end, silently). */
int ss_gemm_f32_splitk_group(const ss_gemm_problem* problems, int n, float* ws, long ws_floats, int flags, ss_stream_t stream);
/* flags bit 0: the launch has the chip to itself -> k-major groups run as 192 x 192 output tiles, one 512-thread workgroup per CU,
 * K slices chosen by the library so that the group fills the chip in one round (`splits` ignored): dG and the layer input are
 * fetched 2 - 3 x instead of 5 - 6 x and the launch takes 12 - 18 % less time alone on the chip.  Beside a latency-bound kernel on
 * another stream (the lower layer's BPTT) the 128 x 64 form with three workgroups per CU is the better neighbour: leave the bit 0. */
/* The same for bf16 operands (config 5; csrc/gemm_bf16.hip): A and B point at bf16 data (k-major, a_kcontig = b_kcontig = 0; lda /
 * ldb / strides in bf16 elements, multiples of 8; K a multiple of 64; n <= 8), C[b] += A[b]^T B[b] in f32.  A group with at least
 * half a chip of 256 x 128 output tiles runs one workgroup per tile over all of K (neighbouring tiles share operand panels in L2);
 * a smaller one has its K tiles dealt evenly over the CUs ("stream-K"), every workgroup leaves raw accumulators in `ws`
 * (ss_gemm_bf16_splitk_group_ws_floats() floats, 16-byte aligned, contents irrelevant) and a second launch folds them into C.
 * `splits` is ignored. */
int ss_gemm_bf16_splitk_group_ws_floats(const ss_gemm_problem* problems, int n, long* floats);
int ss_gemm_bf16_splitk_group(const ss_gemm_problem* problems, int n, float* ws, long ws_floats, ss_stream_t stream);

/* d layer_in of a GRU layer, both directions as one contraction:
 *   C[M][N] = A0[M][K] B0[K][N] + A1[M][K] B1[K][N],  A1 = A + stride_a, B1 = B + stride_b (element strides)
 * A: [row][k] with lda >= K (the gate gradients dG of one direction, lda = 4H, K = 3H); B: [k][col] with ldb, the wanted columns
 * are b_col0 .. b_col0 + N (W_ih as nn.GRU keeps it; b_col0 = x_dim asks for the ROI-embedding columns of layer 0 only); C with
 * ldc >= N.  Every element of C[0..M)[0..N) is written once with a plain store -- C needs no clearing, nothing outside it is
 * written, nothing outside the operands is read -- and the sum runs through A0 B0 with k ascending, then through A1 B1, in one
 * accumulator: the same operands give the same bits.  64 x 192 tiles (N > 32) or 32 x 32 tiles on the LDS-DMA ring; operands
 * that are not 16-byte aligned in every address, leading dimension and stride, or N not a multiple of 4, are staged through
 * registers instead (slow, same result).  SS_ERR_ARG: a null pointer, a size <= 0, lda < K, ldb < b_col0 + N, ldc < N. */
int ss_gru_dx_f32(int M, int N, int K, const float* A, int lda, long stride_a, const float* B, int ldb, int b_col0,
                  long stride_b, float* C, int ldc, ss_stream_t stream);

/* a[0..na) = 0 and b[0..nb) = 0 in one launch (either may be empty; 16-byte aligned): destinations that are summed into with float
 * atomics (the bf16 engine's d layer_in GEMMs) are cleared by this, off the critical path, instead of two library fills */
int ss_zero_f32x2(float* a, long na, float* b, long nb, ss_stream_t stream);

/* column sums: out[n] += sum_r A[r*lda + n]  (bias gradients) */
int ss_colsum_f32(const float* A, int rows, int cols, int lda, float* out, ss_stream_t stream);

/* ---- a3: batch assembly on the device ----------------------------------------------
 * replaces NPZWordDataset.__getitem__ + collate_fn (train_model_official.py:122-204) for clips that are
 * resident in HBM as one ragged frame store: additive feature noise (:143-145), interior frame drop (:146-152,
 * expressed through the map), zero padding / trimming to max_t (:93-118), stacking (:174-204).
 * frame_map (rows = B*max_t) int32: row of the store that lands in each destination row, -1 = zero padding.
 * f32: dst (rows, D) = gathered rows + noise on the rows whose noise_map entry is >= 0 (NULL map: none):
 *      noise != NULL -> noise[noise_map[r]] (host-drawn, bit-exact with the reference's np.random.normal);
 *      noise == NULL and noise_std > 0 -> noise_std * N(0,1) from the Philox stream (seed, element index).
 * u8 : dst (rows, frame_bytes), frame_bytes a multiple of 16 (ROI frames).
 * (ss_batch_gather_f32, _at and _aug are instantiations of one kernel, ss_batch_plan and ss_batch_plan_aug of another.) */
int ss_batch_gather_f32(const float* src, int D, const int32_t* frame_map, long rows, const float* noise,
                        const int32_t* noise_map, float noise_std, uint64_t seed, float* dst, ss_stream_t stream);
/* ss_batch_gather_f32 with Philox noise for a batch that is a run of rows of a larger one (a data-parallel rank's shard of the
 * global batch): element q of dst draws what element noise_first + q of the larger batch draws under the same seed, so the
 * shards of all ranks, concatenated, are the batch one process gathers, bit for bit.  noise_first = (first row of the shard
 * inside the larger batch) * D * max_t; any value, not only multiples of 4.  noise_map as above (required). */
int ss_batch_gather_f32_at(const float* src, int D, const int32_t* frame_map, long rows, const int32_t* noise_map, float noise_std,
                           uint64_t seed, uint64_t noise_first, float* dst, ss_stream_t stream);
int ss_batch_gather_u8(const uint8_t* src, int frame_bytes, const int32_t* frame_map, long rows, uint8_t* dst,
                       ss_stream_t stream);
/* The plan of an epoch and of a batch made on the device (no map, length or label crosses PCIe).  Both draw Philox4x32-10 blocks:
 * counter = (draw index low, high, domain tag, sub-draw number), key = seed; the feature-noise stream of ss_batch_gather_f32 uses
 * tag 0x6e6f6973, these 0x73616d70 (sampler) and 0x706c616e (planner).  Decisions are integer arithmetic on the 32-bit outputs
 * r0..r3: mulhi(r, n) = (uint64)r * n >> 32 is a uniform integer below n, thr(p) = (uint32)(p * 2^32) computed in double.
 * ss_epoch_sample: WeightedRandomSampler(1 / count(label), replacement=True) (train_model_official.py:382-397) = a uniform class
 *   among those that have clips, then a uniform member.  members (n_members) = clip ids grouped by class, class_start
 *   (n_classes + 1) = where each class begins.  Draw first + k: cls = mulhi(r0, n_classes),
 *   indices[k] = members[class_start[cls] + mulhi(r1, size(cls))], k < count.  (`first` lets a rank draw its shard of an epoch.)
 * ss_batch_plan: what NPZWordDataset.__getitem__ decides per clip (train...:143-172), one wave per batch row.  Tables per clip:
 *   x_off / x_len (rows of the feature store), r_off / r_len (rows of the ROI store, r_off < 0: the clip has none; both NULL: the
 *   store has no ROI frames, rmap may be NULL), y.  Row b = clip indices[b] with T = x_len frames, draw index first_row + b:
 *     sub-draw 0: noisy = augment && r0 < thr(noise_prob);  drop = augment && T > 12 && r1 < thr(drop_prob);
 *                 k = 1 + mulhi(r2, drop_max) frames dropped, the first one p0 = 1 + mulhi(r3, T - 2);
 *     sub-draw 1: (k == 2) p1 = 1 + mulhi(r0, T - 3), p1 += (p1 >= p0): every pair of distinct interior frames equally likely.
 *   t_eff = min(T - k, max_t), and min(.., r_len) for a clip with ROI frames; for t < t_eff: xmap[b][t] = x_off + s, where
 *   s = t stepped over the dropped frames in ascending order; nmap[b][t] = noisy ? 0 : -1; rmap[b][t] = r_off + t (ROI frames
 *   are not dropped); all three -1 for t >= t_eff; lens[b] = t_eff; y_out[b] = y[indices[b]].  drop_max > 2: SS_ERR_UNSUPPORTED.
 *   An index outside [0, n_clips) is not dereferenced: the row is an empty clip (lens 0, maps -1, label 0) and *err_flag
 *   (one device word the caller owns and clears) is set to 1. */
int ss_epoch_sample(const int32_t* members, int n_members, const int32_t* class_start, int n_classes, uint64_t first, long count,
                    uint64_t seed, int32_t* indices, ss_stream_t stream);
int ss_batch_plan(const int32_t* indices, int B, const int32_t* x_off, const int32_t* x_len, const int32_t* r_off,
                  const int32_t* r_len, const int64_t* y, int n_clips, int max_t, int augment, uint64_t first_row, uint64_t seed,
                  double noise_prob, double drop_prob, int drop_max, int32_t* xmap, int32_t* nmap, int32_t* rmap, int64_t* lens,
                  int64_t* y_out, int32_t* err_flag, ss_stream_t stream);
/* The opt-in augmentation policy of the device-planned path: a time warp of the whole clip (features and ROI frames together),
 * a scale factor on the features, an integer shift of the ROI frames with edge replication.  ss_batch_plan is untouched; with
 * the three probabilities 0 ss_batch_plan_aug writes the same maps, lengths and labels, bit for bit.
 * ss_batch_plan_aug: ss_batch_plan's arguments and rules (sub-draws 0 and 1 as there), plus, from sub-draw 2 (w0..w3) and
 *   sub-draw 3 (s0..s3) of the same row counter:
 *     warp : T > 10 && w0 < thr(warp_prob): f = warp_lo_pm + mulhi(w1, warp_hi_pm - warp_lo_pm + 1) (permille),
 *            L = max(5, T * f / 1000); else L = T.  Warped position j reads source frame Wp(j) = j * (T - 1) / (L - 1) (integer
 *            division; j when L == T): np.linspace(0, T - 1, L).astype(int) without its float rounding.
 *     drop : the rule of ss_batch_plan on the warped clip: L > 12, positions in [1, L - 2]; features only.
 *     maps : xmap[b][t] = x_off + Wp(t stepped over the dropped positions), rmap[b][t] = r_off + Wp(t);
 *            n_r = L if r_len >= T, else (r_len * (L - 1) + T - 2) / (T - 1) (warped positions whose source frame the ROI track
 *            has; 0 for r_len = 0); t_eff = min(L - k, max_t, n_r for a clip with ROI frames).
 *     scale: w2 < thr(scale_prob): u = (float)(w3 >> 8) * 2^-24, row_scale[b] = fl(scale_lo + fl(scale_span * u)); else 1.0f.
 *     shift: clip has ROI frames && s0 < thr(shift_prob): row_shift[b] = (mulhi(s1, 2 mx + 1) - mx, mulhi(s2, 2 my + 1) - my),
 *            mx = shift_max_x, my = shift_max_y; else (0, 0).
 *   row_scale (B) f32, row_shift (B, 2) int32 (dx, dy).  An invalid index writes scale 1 and shift (0, 0).  SS_ERR_ARG: a
 *   probability outside [0, 1], not 0 < warp_lo_pm <= warp_hi_pm <= 4000, scale_lo <= 0, scale_span < 0, shift_max_* < 0.
 * ss_batch_gather_f32_aug: ss_batch_gather_f32_at (noise_first = 0: the stream of ss_batch_gather_f32) with every element of dst
 *   row r multiplied, after the noise, by row_scale[r / rows_per_clip] (one rounded product).  rows % rows_per_clip == 0.
 * ss_batch_gather_u8_shift: dst[r][y][x] = src[frame_map[r]][clamp(y - dy, 0, H-1)][clamp(x - dx, 0, W-1)], (dx, dy) =
 *   row_shift[r / rows_per_clip]; zeros where frame_map[r] < 0.  H * W % 16 == 0; W % 16 == 0 is the streaming path, other widths
 *   go byte by byte.  shift_max_x / shift_max_y: the bounds the table was planned with, shift_max_x >= W or shift_max_y >= H is
 *   SS_ERR_ARG; whatever the table holds, no byte outside the mapped frame is read. */
int ss_batch_plan_aug(const int32_t* indices, int B, const int32_t* x_off, const int32_t* x_len, const int32_t* r_off,
                      const int32_t* r_len, const int64_t* y, int n_clips, int max_t, int augment, uint64_t first_row, uint64_t seed,
                      double noise_prob, double drop_prob, int drop_max, double warp_prob, int warp_lo_pm, int warp_hi_pm,
                      double scale_prob, float scale_lo, float scale_span, double shift_prob, int shift_max_x, int shift_max_y,
                      int32_t* xmap, int32_t* nmap, int32_t* rmap, int64_t* lens, int64_t* y_out, float* row_scale,
                      int32_t* row_shift, int32_t* err_flag, ss_stream_t stream);
int ss_batch_gather_f32_aug(const float* src, int D, const int32_t* frame_map, long rows, const int32_t* noise_map, float noise_std,
                            uint64_t seed, uint64_t noise_first, const float* row_scale, int rows_per_clip, float* dst,
                            ss_stream_t stream);
int ss_batch_gather_u8_shift(const uint8_t* src, int H, int W, const int32_t* frame_map, long rows, const int32_t* row_shift,
                             int rows_per_clip, int shift_max_x, int shift_max_y, uint8_t* dst, ss_stream_t stream);
/* Rows of a training batch for a model whose ROI CNN is frozen: the embeddings of the store's frames are constants of the run
 * (emb (n_frames, E) f32, made once), so the batch carries E floats per frame instead of the pixels.  Row r of dst (rows rows,
 * ld_dst >= D + E floats apart; columns behind D + E are not written):
 *   [0, D)     bit for bit what ss_batch_gather_f32_aug writes to row r of a dense (rows, D) destination for the same feat, xmap,
 *              noise_map, noise_std, seed, noise_first, row_scale and rows_per_clip -- element (r, c) draws element
 *              noise_first + r * D + c of the noise stream (dense in D, not in ld_dst); row_scale NULL: no scale, i.e. what
 *              ss_batch_gather_f32_at writes (rows_per_clip is then ignored); noise_map NULL: no noise; xmap[r] < 0: zeros.
 *   [D, D + E) emb[rmap[r]] where rmap[r] >= 0, else emb_fill (E floats: the embedding of an all-zero frame, which a clip without
 *              ROI frames gets), or zeros when emb_fill is NULL.  rmap NULL: every row takes the fill (emb may then be NULL).
 * D, E and ld_dst multiples of 4 and feat, emb, emb_fill, dst 16-byte aligned: 16 bytes per lane; anything else goes element by
 * element.  SS_ERR_ARG, nothing written: D <= 0, E <= 0, ld_dst < D + E, rows <= 0, noise_std < 0, row_scale with
 * rows % rows_per_clip != 0, rmap without emb, a base pointer that is not 4-byte aligned. */
int ss_batch_gather_z(const float* feat, int D, const int32_t* xmap, const float* emb, int E, const int32_t* rmap,
                      const float* emb_fill, long rows, const int32_t* noise_map, float noise_std, uint64_t seed,
                      uint64_t noise_first, const float* row_scale, int rows_per_clip, float* dst, int ld_dst, ss_stream_t stream);
/* The masking augmentations of the policy: one masked run of frames, one zeroed band of feature columns, one filled rectangle of
 * the ROI frames, each per clip.  Two launches beside the ones above, which do not change: the masks are planned into the maps a
 * planner has written, the band and the rectangle are written over what the gathers have written.
 * ss_batch_plan_mask: behind ss_batch_plan or ss_batch_plan_aug on the same stream; one wave per batch row.  xmap, nmap, rmap
 *   (may be NULL) (B, max_t) are edited in place, lens (B) is read.  Row b draws the planner's own counter (draw index
 *   first_row + b, tag "plan", key = seed), sub-draws 4 (m0..m3), 5 (c0..c3) and 6 (q0..q3); sub-draws 0 - 3 keep their use.
 *   n = lens[b]; has_roi = rmap && n > 0 && rmap[b][0] >= 0.
 *     time  : augment && n >= 8 && m0 < thr(time_mask_prob): cap = min(time_mask_max, n / 4), tw = 1 + mulhi(m1, cap),
 *             t0 = 1 + mulhi(m2, n - tw): the run [t0, t0 + tw) lies in [1, n), frame 0 is never masked, lens never changes.
 *             time_mask_streams 0 (both), 1 (features: xmap and nmap), 2 (roi: rmap) selects the maps the run is written into;
 *             time_mask_fill 0 (zero): their entries become -1, the gathers write zero rows (ss_batch_gather_z: emb_fill);
 *             1 (hold): xmap[t] = xmap[t0 - 1], rmap[t] = rmap[t0 - 1], nmap untouched -- a repeated row takes fresh noise.
 *     band  : augment && c0 < thr(feat_mask_prob): cw = 1 + mulhi(c1, min(feat_mask_max, D)), col0 = mulhi(c2, D - cw + 1).
 *     cutout: augment && has_roi && c3 < thr(cutout_prob): rw = 1 + mulhi(q0, min(cut_max_w, W)),
 *             rh = 1 + mulhi(q1, min(cut_max_h, H)), x0 = mulhi(q2, W - rw + 1), y0 = mulhi(q3, H - rh + 1).
 *   A maximum of 0 switches its mask off (the cutout: either of its two).  row_mask (B, 8) int32 = {t0, tw, col0, cw, x0, y0, rw,
 *   rh}; an inactive mask writes width 0 and position 0, an empty row (n = 0, the planner's invalid-index rows among them) eight
 *   zeros and edits nothing.  SS_ERR_ARG, nothing written: a probability outside [0, 1], a negative maximum, streams outside
 *   0..2, fill outside 0..1, cutout_fill outside [0, 255] (only checked here), a cutout that is on with rmap NULL or H, W <= 0.
 * ss_batch_mask_apply: behind the gathers, in place.  Row r of the batch belongs to clip r / rows_per_clip:
 *     X[r][col0, col0 + cw) = 0.0f; X rows are ld_x >= D floats apart, so the call serves the dense X (ld_x = D) and the Z of
 *     ss_batch_gather_z (ld_x = D + E) alike;  R[r][y0, y0 + rh)[x0, x0 + rw) = fill where rmap[r] >= 0 (zero-padding frames and
 *     the frames of clips without ROI stay zero).  X or R may be NULL (its half is skipped).  Nothing else is read or written:
 *   the launch's traffic is the masked bytes and the two tables.  Whatever row_mask holds, positions and widths are clamped into
 *   the row and the frame first.  SS_ERR_ARG: both X and R NULL, rows % rows_per_clip != 0, fill outside [0, 255], ld_x < D,
 *   R without rmap. */
int ss_batch_plan_mask(int32_t* xmap, int32_t* nmap, int32_t* rmap, const int64_t* lens, int B, int max_t, int D, int H, int W,
                       int augment, uint64_t first_row, uint64_t seed, double time_mask_prob, int time_mask_max,
                       int time_mask_streams, int time_mask_fill, double feat_mask_prob, int feat_mask_max, double cutout_prob,
                       int cut_max_w, int cut_max_h, int cutout_fill, int32_t* row_mask, ss_stream_t stream);
int ss_batch_mask_apply(float* X, int ld_x, int D, uint8_t* R, int H, int W, const int32_t* rmap, const int32_t* row_mask,
                        long rows, int rows_per_clip, int fill, ss_stream_t stream);

/* Mixup of a planned batch (AugmentPolicy: mixup_prob, mixup_alpha; inactive/train_reduced.py:36-53 mixes the collated batch): one
 * factor lam = k / 256 per batch, k an integer in [0, 256], and one partner row per row.  Two launches behind everything above:
 * ss_batch_plan_mixup: one workgroup; lens (B) and y (B) int64 as a planner wrote them.  Draws of the planners' scheme under the
 *   domain tag "mixp" (0x6d697870), so they meet no other stream: counter (batch_first_row, "mixp", 0) gives u0, u1; the batch is
 *   mixed iff augment && u0 < thr(mixup_prob), and then k = table[mulhi(u1, N)] -- table (N) device uint16 with entries in
 *   [0, 256] (quantiles of Beta(alpha, alpha) times 256; larger entries count as 256), N a power of two.  Counter
 *   (batch_first_row + b, "mixp", 1) gives row b its 32-bit key; perm[b] = the rank of (key_b, b) among the rows (a stable
 *   argsort: a uniform permutation).  Not mixed: perm = identity, k = 256.  Written, all on the device: perm (B) int32,
 *   y_b (B) int64 = y[perm], lens_m (B) int64 = max(lens, lens[perm]) (the shorter clip adds its zero padding), k_out (1) int32,
 *   lam_out (1) float = k / 256.  SS_ERR_ARG, nothing written: B outside [1, 1024], N not a power of two, mixup_prob outside [0, 1].
 * ss_batch_mixup: the blended batch, out of place (rows are read through perm), one launch, two HBM streams:
 *     Xm[b] = fmaf(lam, X[b], (1 - lam) * X[perm[b]])                 X, Xm (B, T, D) f32, rows ld_x >= D floats apart in both
 *     Rm[b] = (k R[b] + (256 - k) R[perm[b]] + 128) >> 8 per byte     R, Rm (B, T, frame_bytes) u8, frame_bytes % 16 == 0
 *   with k (1) int32 read from the DEVICE.  X / Xm or R / Rm may be NULL as a pair.  A clip with perm[b] == b, and every clip
 *   when k == 256, is copied byte for byte.  Any D (16 bytes per lane where D and ld_x are multiples of 4 and X, Xm 16-byte
 *   aligned).  SS_ERR_ARG: both pairs NULL, half a pair, X == Xm or R == Rm, ld_x < D, R or Rm not 16-byte aligned;
 *   SS_ERR_UNSUPPORTED: frame_bytes % 16 != 0. */
int ss_batch_plan_mixup(const int64_t* lens, const int64_t* y, int B, int augment, uint64_t batch_first_row, uint64_t seed,
                        double mixup_prob, const uint16_t* table, int N, int32_t* perm, int64_t* y_b, int64_t* lens_m,
                        int32_t* k_out, float* lam_out, ss_stream_t stream);
int ss_batch_mixup(const float* X, int ld_x, int D, float* Xm, const uint8_t* R, uint8_t* Rm, int frame_bytes,
                   const int32_t* perm, const int32_t* k, int B, int T, ss_stream_t stream);

/* ---- sliding-window serving of many streams ---------------------------------------
 * per stream a ring of the last max_t frames (features (S,max_t,D) f32, optional ROI (S,max_t,frame_bytes) u8), a head
 * and a count: the deque(maxlen=max_t) of inactive/live_feed.py:155.  A push appends one frame for each of n DISTINCT
 * streams (feats (n,D), rois (n,frame_bytes)) and bumps frames_seen; the window map lists, oldest first, the rows of the
 * rings of n selected streams (-1 = zero padding; live_feed.py:203-207) for ss_batch_gather_f32/u8, lengths = frames held.
 * ss_mouth_openness: the openness signal itself, float64 like the reference's Python floats.  lm (n,K,2) f32 normalised
 *   (x,y) landmarks; mode 0: |y[i_bot] - y[i_top]| / (dist2d(lm[i_eye_l], lm[i_eye_r]) + 1e-6)
 *   (important_landmarks.py:64-67, 131-133; within one ulp of its ``** 0.5``); mode 1: max(y) - min(y) over the K
 *   landmarks (inactive/live_test_5.py:92-94; the i_* arguments are ignored); mode 2: |lm[i_top] - lm[i_bot]| / (|lm[i_eye_r] -
 *   lm[i_eye_l]| + 1e-6) in float32, every operation rounded (inactive/live_feed.py:69-78 with i_top/i_bot = 13/14 and the
 *   mouth corners 61/291 in the two "eye" slots).  All three are pinned by the reference's own outputs (tests/golden/serving.npz).
 * ss_mouth_gate: EMA (alpha) of the openness and its open/close hysteresis, carried in float64
 *   (important_landmarks.py:136-144: ``mouth_ema`` is a Python float).
 * ss_clip_gate: openness-gated clip segmentation of n DISTINCT streams (inactive/live_test_5.py:146-152, 233-272):
 *   state (S,4) int32 = {speaking, above_ct, below_ct, clip_len}, zero-initialised.  Per pushed frame:
 *   openv > open_thresh bumps above_ct and clears below_ct, else the reverse; idle streams start a clip (clip_len = 0)
 *   after start_n consecutive frames above -- the starting frame itself is not kept; speaking streams append the frame
 *   (feats row -> clip_x (S,max_clip,D), rois -> clip_r (S,max_clip,frame_bytes)) and stop after end_n consecutive
 *   frames below or at max_clip frames.  append_row (n): row written, -1 if none; emit_len (n): length of the clip that
 *   just ended if >= min_clip (the reference classifies clips of >= 6 frames), else 0.  face_present (n) u8 may be
 *   NULL; 0 resets the stream (the "NO FACE" branch, :293-301). */
int ss_ring_push(float* ring_x, uint8_t* ring_r, int n_streams, int max_t, int D, int frame_bytes,
                 const int32_t* stream_ids, int n, const float* feats, const uint8_t* rois, int32_t* head, int32_t* count,
                 int32_t* frames_seen, ss_stream_t stream);
/* a camera frame in which no face was found, for n DISTINCT streams: frames_seen runs on (live_feed.py:173 counts every camera
 * frame, and the prediction rule :201 tests that count), the ring keeps what it holds (:179-185 ``continue``) */
int ss_ring_tick(const int32_t* stream_ids, int n, int32_t* frames_seen, ss_stream_t stream);
int ss_ring_window_map(const int32_t* stream_ids, int n, int max_t, const int32_t* head, const int32_t* count,
                       int32_t* frame_map, int64_t* lengths, ss_stream_t stream);
int ss_mouth_openness(const float* lm, int n, int K, int mode, int i_top, int i_bot, int i_eye_l, int i_eye_r,
                      double* openness, ss_stream_t stream);
int ss_mouth_gate(const int32_t* stream_ids, int n, const double* openness, double alpha, double open_thr,
                  double close_thr, double* ema, uint8_t* state_open, ss_stream_t stream);
int ss_clip_gate(const int32_t* stream_ids, int n, const double* openv, const uint8_t* face_present, double open_thresh,
                 int start_n, int end_n, int max_clip, int min_clip, int32_t* state, int D, int frame_bytes,
                 const float* feats, const uint8_t* rois, float* clip_x, uint8_t* clip_r, int32_t* append_row,
                 int32_t* emit_len, ss_stream_t stream);

/* ---- BASELINE config 5 (100 words, 96x96 ROI, CNN 16/32/64/96, BiGRU H = 512, bf16 MFMA) ----------------------
 * The reference defines no such model ("build-defined"); it is the same module
 * (train_model_official.py:209-229, 253-310) with wider layers, run on v_mfma_f32_16x16x32_bf16: operands rounded to
 * bf16 on their way into LDS / registers, f32 accumulation, f32 master weights, activations between the GRU kernels f32.
 *
 * ss_gemm_bf16_batched: C[M,N] (+)= opA * opB (+ bias), the conventions of ss_gemm_f32_batched (f32 operands in HBM,
 *   a_kcontig / b_kcontig, storage-row remap, batch strides in elements); flags bit0 accumulate, bit2 float atomics;
 *   splits > 1 slices K and needs bit0 (atomics into a C the caller initialised).  Contiguous dimensions % 4 == 0.
 *   flags bit3: A and B already ARE bf16 in HBM (uint16 bit patterns; lda / ldb / strides in bf16 elements, multiples of 8,
 *   leading dimensions zero-padded to a multiple of 8 where the extent is not one: ss_cvt_bf16_rows): no conversion pass,
 *   half the operand bytes, 64-deep k tiles. */
int ss_gemm_bf16_batched(int a_kcontig, int b_kcontig, int M, int N, int K, const void* A, int lda, int a_group,
                         int a_gstride, int a_off, const void* B, int ldb, int b_group, int b_gstride, int b_off,
                         float* C, int ldc, const float* bias, int flags, int splits, int batch, long stride_a,
                         long stride_b, long stride_c, long stride_bias, ss_stream_t stream);

/* GRU recurrence for wide hidden states (H % 128 == 0), both directions, same masking semantics and buffer layouts as
 * ss_gru_fwd / ss_gru_bwd (gi (2,N,3H), out (N,2H), save / d_g (2,N,4,H)).
 * ss_gru_bf16_prep: W_hh of both directions -> whh_bf16 (2,3H,H) and its transpose whh_t_bf16 (2,H,3H), once per
 *   optimiser step; with wih_bf16 (may be NULL) also W_ih (3H,K) of both directions -> (2,3H,Kp) bf16, Kp = K rounded up
 *   to 8, zero-padded: the operand of the layer's input-projection / d layer_in GEMMs (ss_gemm_bf16_batched, bit 3).  ws: ss_gru_bf16_ws_bytes(B, H) bytes (state / gate-gradient hand-over between step launches).
 * Two forms behind one entry point.  With sync_ws (ss_gru_bf16_sync_bytes(B, T, H) bytes, > 0 for H = 128 ... 512;
 *   ZEROED ONCE by the caller, kept consistent by the kernels afterwards) a layer is ONE persistent launch per clip chunk:
 *   a (16-clip slice, direction) is spread over H/64 workgroups that keep their rows of W_hh in registers for all T steps
 *   and exchange the state (forward) / partial d h_prev (backward) through tagged 8-byte granules (csrc/gru_bf16_pers.h).
 *   sync_ws = NULL, or a shape outside that range: one launch per time step.  sync_bytes = the bytes the caller allocated at
 *   sync_ws: the layout is a function of (B, T, H) -- and not monotone in B -- so the entry points recompute it and return
 *   SS_ERR_ARG when an area sized for another batch is too small for this one.
 *   sync_ws words: [0] launch generation, [1] arrivals, [2] bounded waits that gave up (a lost partner: the workgroups
 *   concerned emit NaN from then on; the owner reads this word where it synchronises), [3] same-XCD fast-path count,
 *   [5] fault injection for tests (1 + index of a workgroup that plays dead; 0 = off).
 * By-products (each may be NULL): out_bf16 (N,2H) = bf16 copy of out; out_drop_bf16 (N,2H) = bf16 of dropout(out) with
 *   ss_dropout's Philox stream at (seed, offset) over the (N,2H) index space -- nn.GRU's inter-layer dropout, ready as
 *   the next layer's MFMA operand (drop_p = 0: a plain copy); d_g_bf16 (2,N,4,H) = bf16 copy of d_g (with it, the
 *   persistent form also accepts d_g = NULL: 126 MB per launch less to write at config 5); g_b* (all four or
 *   none): d b_ih += column sums of (d r, d z, d n), d b_hh += column sums of (d r, d z, d hn) (what ss_gru_bias_grad
 *   computes from d_g).  ss_gru_bf16_bwd: drop_p / seed / offset = the same mask re-drawn on d_out (see ss_gru_bwd).
 * ss_cvt_bf16_rows: y[r][c] = bf16(x[r][c] * mask), c < cols; y[r][cols .. ld_y) = 0 (GEMM operands are read in whole
 *   8-element chunks); cols, ld_x, ld_y % 4 == 0; the mask indexes the SOURCE element r * ld_x + c. */
int ss_gru_bf16_prep(const float* w_hh_f, const float* w_hh_r, int H, uint16_t* whh_bf16, uint16_t* whh_t_bf16,
                     const float* w_ih_f, const float* w_ih_r, int K, uint16_t* wih_bf16, ss_stream_t stream);
int ss_gru_bf16_ws_bytes(int B, int H, long* bytes);
int ss_gru_bf16_sync_bytes(int B, int T, int H, long* bytes);
int ss_gru_bf16_fwd(const float* gi, const uint16_t* whh_bf16, const float* b_hh_f, const float* b_hh_r,
                    const int32_t* lengths, int B, int T, int H, float* out, float* save, uint16_t* out_bf16,
                    uint16_t* out_drop_bf16, float drop_p, uint64_t seed, uint64_t offset, void* ws, void* sync_ws,
                    long sync_bytes, ss_stream_t stream);
int ss_gru_bf16_bwd(const float* d_out, const float* out, const float* save, const uint16_t* whh_t_bf16,
                    const int32_t* lengths, int B, int T, int H, float* d_g, uint16_t* d_g_bf16, float drop_p,
                    uint64_t seed, uint64_t offset, float* g_bih_f, float* g_bhh_f, float* g_bih_r, float* g_bhh_r,
                    void* ws, void* sync_ws, long sync_bytes, ss_stream_t stream);
int ss_cvt_bf16_rows(const float* x, int ld_x, uint16_t* y, int ld_y, long rows, int cols, float drop_p, uint64_t seed,
                     uint64_t offset, ss_stream_t stream);

/* bf16 ROI-CNN of config 5: 96x96 uint8 frame -> normalise -> [conv3x3 + ReLU + maxpool2] x 3 (1->16->32->64) ->
 * conv3x3 64->96 + ReLU -> global average -> Linear(96 -> E): TinyROICNN (train_model_official.py:209-229) with a fourth
 * block.  One persistent kernel per layer; between the layers the pooled maps are NHWC bf16 (N,H,W,C) in HBM with one
 * argmax byte per pooled element (0..3 = position in the 2x2 window, 4 = maximum not positive: no gradient).
 *   ss_c5_conv1_fwd      R (N,96,96) u8 -> a1 (N,48,48,16) bf16, i1 (N,48,48,16) u8, st (N,2) f32 mean/std (may be NULL)
 *   ss_c5_conv_fwd       layer 2: a1 -> a2 (N,24,24,32), i2;  layer 3: a2 -> a3 (N,12,12,64), i3
 *   ss_c5_conv_last_fwd  a3 -> z rows (E floats at z + n*ld_z); training also mask (N,144,96) u8 and feat (N,96) f32
 * Backward (gradients ACCUMULATE into g_*; d a maps are UNMASKED, the argmax byte of the layer below applies its ReLU):
 *   ss_c5_conv_last_wgrad  d z (N,E at ld_dz) -> g_w4, g_b4, g_wfc, g_bfc;   ss_c5_conv_last_dgrad -> da3 (N,12,12,64)
 *   ss_c5_conv_wgrad / ss_c5_conv_dgrad  layer 3: (a2, da3, i3) -> g_w3, g_b3 / da2;  layer 2: (a1, da2, i2) -> g_w2, g_b2 / da1
 *   ss_c5_conv1_wgrad      (R, st, da1, i1 | w1, b1) -> g_w1, g_b1 */
int ss_c5_conv1_fwd(const uint8_t* R, int N, int standardize, const float* w1, const float* b1, uint16_t* a1, uint8_t* i1,
                    float* st, ss_stream_t stream);
int ss_c5_conv_fwd(int layer, const uint16_t* in, int N, const float* w, const float* b, uint16_t* out, uint8_t* idx,
                   ss_stream_t stream);
int ss_c5_conv_last_fwd(const uint16_t* in, int N, const float* w, const float* b, const float* wfc, const float* bfc, int E,
                        float* z, int ld_z, uint8_t* mask, float* feat, ss_stream_t stream);
int ss_c5_conv_wgrad(int layer, const uint16_t* a_in, const uint16_t* da_out, const uint8_t* idx, int N, float* g_w, float* g_b,
                     ss_stream_t stream);
int ss_c5_conv_dgrad(int layer, const uint16_t* da_out, const uint8_t* idx, int N, const float* w, uint16_t* da_in,
                     ss_stream_t stream);
int ss_c5_conv_last_wgrad(const uint16_t* a_in, const float* dz, int ld_dz, int E, const float* wfc, const uint8_t* mask,
                          const float* feat, int N, float* g_w, float* g_b, float* g_wfc, float* g_bfc, ss_stream_t stream);
int ss_c5_conv_last_dgrad(const float* dz, int ld_dz, int E, const float* wfc, const uint8_t* mask, int N, const float* w,
                          uint16_t* da_in, ss_stream_t stream);
int ss_c5_conv1_wgrad(const uint8_t* R, int N, int standardize, const float* st, const uint16_t* da1, const uint8_t* i1,
                      const float* w1, const float* b1, float* g_w1, float* g_b1, ss_stream_t stream);
/* ss_c5_conv_dgrad(2) and ss_c5_conv1_wgrad (recompute form) in ONE kernel: the gradient w.r.t. the pooled conv1 map (73.7 KB per
 * frame, the largest gradient of the net) is born band by band in LDS and consumed there: 1.13 GB per step at config 5 that no
 * longer crosses HBM.  da1 may be NULL (the product path); non-NULL: the map is also stored (N,48,48,16), for tests. */
int ss_c5_conv2_dgrad_conv1_wgrad(const uint16_t* da2, const uint8_t* i2, int N, const float* w2, const uint8_t* R, const float* st,
                                  int standardize, const float* w1, const float* b1, uint16_t* da1, float* g_w1, float* g_b1,
                                  ss_stream_t stream);
/* The fused forms the engine uses (the pooled conv1 map -- 74 KB per frame + 37 KB of argmax bytes, the largest tensor of the
 * net -- never reaches HBM):
 *   ss_c5_conv12_fwd      R -> a2 (N,24,24,32), i2, st: conv1 lands in conv2's LDS image
 *   ss_c5_conv2_wgrad_rc  layer 2's weight gradient with a1 recomputed per band from R and st (conv1: w1, b1)
 *   ss_c5_conv1_wgrad     with i1 == NULL recomputes conv1's pool winners from R (needs w1, b1) */
int ss_c5_conv12_fwd(const uint8_t* R, int N, int standardize, const float* w1, const float* b1, const float* w2, const float* b2,
                     uint16_t* a2, uint8_t* i2, float* st, ss_stream_t stream);
/* Layer 4 with its Linear and the Linear's gradients as the caller's GEMMs over all frames (three small f32 GEMMs instead of a
 * per-frame walk over W_fc inside the persistent kernels):
 *   ss_c5_conv_last_fwd_feat  a3 -> feat (N,96) f32 (+ mask (N,144,96) u8 when training); z = feat . W_fc^T + b_fc is the caller's
 *   ss_c5_conv_last_wgrad_df / _dgrad_df  take dfeat (N,96) f32 = d z . W_fc (unscaled: the kernels divide by 144);
 *                             g_wfc += d z^T . feat and g_bfc += column sums of d z are the caller's */
int ss_c5_conv_last_fwd_feat(const uint16_t* in, int N, const float* w, const float* b, uint8_t* mask, float* feat, ss_stream_t stream);
int ss_c5_conv_last_wgrad_df(const uint16_t* a_in, const float* dfeat, const uint8_t* mask, int N, float* g_w, float* g_b,
                             float* part, long part_floats, ss_stream_t stream);
/* Weight gradients with the workgroups' partial sums through a scratch buffer instead of float atomics onto g_w:
 * part = (min(N, CUs)) x (COUT * CIN * 9) floats, 16-byte aligned, contents irrelevant; NULL or too small: the atomics form.
 * (256 workgroups adding 55 k floats each onto the same 55 k addresses was half of the last layer's launch.) */
int ss_c5_conv_wgrad_ws(int layer, const uint16_t* a_in, const uint16_t* da_out, const uint8_t* idx, int N, float* g_w, float* g_b,
                        float* part, long part_floats, ss_stream_t stream);
int ss_c5_conv2_wgrad_rc_ws(const uint8_t* R, const float* st, int standardize, const float* w1, const float* b1,
                            const uint16_t* da_out, const uint8_t* idx, int N, float* g_w, float* g_b, float* part, long part_floats,
                            ss_stream_t stream);
int ss_c5_conv_last_dgrad_df(const float* dfeat, const uint8_t* mask, int N, const float* w, uint16_t* da_in, ss_stream_t stream);
/* The same two with conv1's pool winners i1 (N,48,48,16) u8 left in HBM by the forward kernel and read back by the fused backward
 * kernel instead of being recomputed from the frame (37 KB per frame each way; i1 = NULL: the forms above). */
int ss_c5_conv12_fwd_i1(const uint8_t* R, int N, int standardize, const float* w1, const float* b1, const float* w2, const float* b2,
                        uint16_t* a2, uint8_t* i2, float* st, uint8_t* i1, ss_stream_t stream);
int ss_c5_conv2_dgrad_conv1_wgrad_i1(const uint16_t* da2, const uint8_t* i2, int N, const float* w2, const uint8_t* R, const float* st,
                                     int standardize, const float* w1, const float* b1, uint16_t* da1, float* g_w1, float* g_b1,
                                     const uint8_t* i1, ss_stream_t stream);
int ss_c5_conv2_wgrad_rc(const uint8_t* R, const float* st, int standardize, const float* w1, const float* b1,
                         const uint16_t* da_out, const uint8_t* idx, int N, float* g_w, float* g_b, ss_stream_t stream);

/* ---- a7: one bidirectional GRU layer, recurrence only ---------------------------------------
 * replaces pack_padded_sequence -> nn.GRU -> pad_packed_sequence (train_model_official.py:301-305).
 * gi      (2, B*T, 3H): W_ih x + b_ih per direction (forward, reverse), from ss_gemm_f32
 * lengths (B) int32, 1 <= len <= T
 * out     (B,T,2H): forward states in [0,H), reverse in [H,2H); zeros for t >= len
 * save    (2, B*T, 4, H) or NULL: r, z, n, W_hn h + b_hn for the backward pass
 * sync_ws NULL, or ss_gru_sync_bytes() bytes of device memory the caller zeroed ONCE and then leaves alone: with it,
 *         a batch small enough to leave most CUs idle runs each (16-clip slice, direction) on several CUs that
 *         exchange the state through `out` every step (same results, lower latency).  Launches that may run
 *         concurrently (different streams) need different sync_ws; launches on one stream can share one.
 * H in {64, 192} */
int ss_gru_fwd(const float* gi, const float* w_hh_f, const float* w_hh_r, const float* b_hh_f,
               const float* b_hh_r, const int32_t* lengths, int B, int T, int H, float* out, float* save,
               void* sync_ws, ss_stream_t stream);
/* The same with nn.GRU's inter-layer dropout as a by-product: out_drop (B,T,2H) = out x the keep-scales of ss_dropout's Philox
 * stream at (drop_seed, drop_offset) -- what the next layer's input projection multiplies (train_model_official.py:261-267,
 * dropout=0.2 between the layers).  out_drop != NULL needs the multi-CU form (sync_ws given, ss_gru_sync_bytes(B,T,H) != 0);
 * otherwise SS_ERR_UNSUPPORTED and the caller runs ss_dropout on `out`. */
int ss_gru_fwd_drop(const float* gi, const float* w_hh_f, const float* w_hh_r, const float* b_hh_f, const float* b_hh_r,
                    const int32_t* lengths, int B, int T, int H, float* out, float* save, float* out_drop, float drop_p,
                    uint64_t drop_seed, uint64_t drop_offset, void* sync_ws, ss_stream_t stream);

/* bytes of sync_ws the multi-CU recurrence needs for this shape; 0 = the shape always takes the one-CU-per-slice
 * kernels (pass NULL). */
int ss_gru_sync_bytes(int B, int T, int H, long* bytes);

/* BPTT.  d_out (B,T,2H) gradient of the layer output; d_g (2, B*T, 4, H) receives
 * d(gi_r), d(gi_z), d(gi_n) and d(W_hn h + b_hn) = d(gi_n) * r; rows with t >= len are zero.
 * drop_p > 0: d_out is the gradient w.r.t. the DROPPED-OUT output (nn.GRU's inter-layer dropout); the mask is the
 * ss_dropout stream (drop_seed, drop_offset) over the (B*T, 2H) tensor and is applied while d_out is read.
 * g_bih_f, g_bhh_f, g_bih_r, g_bhh_r (each 3H floats; all NULL = not wanted): the bias gradients of the layer are summed up
 * while the recurrence runs and ADDED here (what ss_gru_bias_grad computes from d_g in a separate pass). */
int ss_gru_bwd(const float* d_out, const float* out, const float* save, const float* w_hh_f,
               const float* w_hh_r, const int32_t* lengths, int B, int T, int H, float* d_g,
               float drop_p, uint64_t drop_seed, uint64_t drop_offset, float* g_bih_f, float* g_bhh_f, float* g_bih_r,
               float* g_bhh_r, void* sync_ws, ss_stream_t stream);

/* bias gradients of one GRU layer from d_g: g_bih_* (3H) += colsum(d_g[dir][:, 0:3H]),
 * g_bhh_* (3H) += colsum(d_g[dir][:, 0:2H] | d_g[dir][:, 3H:4H]).  N = B*T rows per direction. */
int ss_gru_bias_grad(const float* d_g, int N, int H, float* g_bih_f, float* g_bhh_f, float* g_bih_r, float* g_bhh_r,
                     ss_stream_t stream);

/* ---- a8: AttnPool (train_model_official.py:231-248) ------------------------------------------
 * h (B,T,D), score weight (D) + bias (1); masked (-1e9) softmax over t, weighted sum.
 * attn (B,T) softmax weights (saved for backward), pooled (B,D). */
int ss_attn_pool_fwd(const float* h, const int32_t* lengths, const float* w_score, const float* b_score, int B,
                     int T, int D, float* attn, float* pooled, ss_stream_t stream);
/* d_h (B,T,D) is written (not accumulated); g_w (D), g_b (1) are accumulated. */
int ss_attn_pool_bwd(const float* h, const int32_t* lengths, const float* w_score, const float* attn,
                     const float* d_pooled, int B, int T, int D, float* d_h, float* g_w, float* g_b,
                     ss_stream_t stream);

/* ---- a9: head = LayerNorm -> Linear -> ReLU -> Dropout -> Linear (train_model_official.py:271-277)
 * The two Linear layers go through ss_gemm_f32; these are the LayerNorm halves.
 * xhat (B,D) normalised rows and rstd (B) are saved for the backward. */
int ss_layernorm_fwd(const float* x, const float* gamma, const float* beta, int B, int D, float eps, float* y,
                     float* xhat, float* rstd, ss_stream_t stream);
int ss_layernorm_bwd(const float* d_y, const float* xhat, const float* rstd, const float* gamma, int B, int D,
                     float* d_x, float* g_gamma, float* g_beta, ss_stream_t stream);
/* y = x * mask(philox(seed, offset)) / (1-p), or the same mask applied to a gradient; p = 0 is a no-op.
 * relu_of (may be NULL): additionally zero where relu_of <= 0 (ReLU backward fused). */
int ss_dropout(const float* x, float* y, long n, float p, uint64_t seed, uint64_t offset, const float* relu_of,
               ss_stream_t stream);

/* ---- a8+a9(+CE) fused: the whole classifier tail of one clip per workgroup ----------------------
 * AttnPool -> LayerNorm -> Linear(D,MID) -> ReLU -> Dropout(drop_p) -> Linear(MID,C), and, when y != NULL,
 * CrossEntropyLoss(label_smoothing)/denom with d(loss)/d(logits) (train_model_official.py:231-248, 271-277, 405).
 * Stash outputs (attn (B,T), xhat (B,D), rstd (B), ln (B,D) = LayerNorm output, mid (B,MID) = post-ReLU,
 * mid_d (B,MID) = after dropout) may each be NULL for inference.  Dropout draws the ss_dropout stream (seed, offset)
 * at element index b*MID + o.
 * Supported: any T, D, MID, C >= 1 (tested: T 1..15 221, D 1..2 050, MID 1..1 025, C 1..1 025; 1 <= lengths[b] <= T) as long as
 * the clip's rows fit the workgroup's 60 KiB of LDS: T + 2 D + MID + C <= 15 360 floats here, MID + D + 2 T + C <= 15 360 in
 * ss_tail_bwd; beyond that SS_ERR_UNSUPPORTED.  h behind a clip's length is never read. */
int ss_tail_fwd(const float* h, const int32_t* lengths, const float* w_score, const float* b_score, const float* gamma,
                const float* beta, const float* w1, const float* b1, const float* w4, const float* b4, const int64_t* y,
                int B, int T, int D, int MID, int C, float ln_eps, float drop_p, uint64_t seed, uint64_t offset,
                float label_smoothing, float denom, float* attn, float* xhat, float* rstd, float* ln, float* mid,
                float* mid_d, float* logits, float* d_logits, float* loss_sum, int32_t* correct, ss_stream_t stream);
/* ss_tail_fwd with the class-weighted loss CrossEntropyLoss(weight=cw, label_smoothing) (train_model_official.py:406-414):
 * cw (C) class weights, den (1) a DEVICE float read by the kernel = sum of cw[y] over the normalising set (the global batch:
 * ss_class_weight_sum) in place of the host `denom`; y, cw and den must not be NULL.  Per row
 *   l = (1-ls) * (-cw[y] lp[y]) + (ls/C) * (-sum_c cw[c] lp[c]),    loss_sum += l / *den,
 *   d_logits[c] = [ (1-ls) cw[y] (p_c - [c==y]) + (ls/C) (p_c sum_k cw[k] - cw[c]) ] / *den.
 * A row whose label is outside [0, C) gets a zero d_logits row and adds nothing.  With every cw[c] == 1 and *den == denom the
 * logits, d_logits and the loss are bit for bit those of ss_tail_fwd.  ss_tail_bwd serves both. */
int ss_tail_fwd_w(const float* h, const int32_t* lengths, const float* w_score, const float* b_score, const float* gamma,
                  const float* beta, const float* w1, const float* b1, const float* w4, const float* b4, const int64_t* y,
                  int B, int T, int D, int MID, int C, float ln_eps, float drop_p, uint64_t seed, uint64_t offset,
                  float label_smoothing, const float* cw, const float* den, float* attn, float* xhat, float* rstd, float* ln,
                  float* mid, float* mid_d, float* logits, float* d_logits, float* loss_sum, int32_t* correct,
                  ss_stream_t stream);
/* ss_tail_fwd / ss_tail_fwd_w with the two-label loss of a mixup batch: y_b (B) the partners' labels, lam (1) a DEVICE float in
 * [0, 1] (ss_batch_plan_mixup writes both).  cw and den both NULL: the unweighted loss divided by `denom`; both given: the
 * class-weighted one divided by *den (`denom` unused) -- sum_i cw[y_b[i]] is the sum over the same labels as sum_i cw[y[i]], so
 * the one normaliser serves both terms.  Per row
 *   l = lam * l(y) + (1 - lam) * l(y_b),    d_logits[c] = [ p_c A_mix - (lam tgt(y)_c + (1 - lam) tgt(y_b)_c) ] / normaliser,
 * l, tgt and A as above and A_mix the same blend of the two As (1 without weights).  correct counts argmax == y.  A row with
 * either label outside [0, C) gets a zero d_logits row and adds nothing.  *lam == 1: the bits of ss_tail_fwd / ss_tail_fwd_w.
 * ss_tail_bwd serves this one too. */
int ss_tail_fwd_mix(const float* h, const int32_t* lengths, const float* w_score, const float* b_score, const float* gamma,
                    const float* beta, const float* w1, const float* b1, const float* w4, const float* b4, const int64_t* y,
                    const int64_t* y_b, const float* lam, int B, int T, int D, int MID, int C, float ln_eps, float drop_p,
                    uint64_t seed, uint64_t offset, float label_smoothing, float denom, const float* cw, const float* den,
                    float* attn, float* xhat, float* rstd, float* ln, float* mid, float* mid_d, float* logits, float* d_logits,
                    float* loss_sum, int32_t* correct, ss_stream_t stream);
/* Any of the three losses above blended with a teacher's soft targets (knowledge distillation): t_logits (B, ld_t) f32 teacher
 * logits (rows ld_t >= C apart; they must be finite: the caller vouches for it), kd_alpha in [0, 1], kd_tau > 0 and finite.
 * y_b / lam and cw / den are each both given or both NULL, as under ss_tail_fwd_mix.  Per row, with q = softmax(z / tau) of the
 * row's own logits z and pt = softmax(t / tau):
 *   l           = (1 - alpha) * hard / hard_norm        + alpha * tau^2 * sum_c pt_c (log pt_c - log q_c) / denom,
 *   d_logits[c] = (1 - alpha) * hard_grad_c / hard_norm + alpha * tau * (q_c - pt_c) / denom,
 * `hard` the loss the other arguments describe over its own normaliser (denom, or *den with weights).  The soft term is not
 * class-weighted and is ALWAYS divided by `denom` (the global clip count: kl_div's "batchmean"), so `denom` > 0 is required
 * with weights too.  The label rule is that of the hard loss; a row that does not count adds nothing, soft term included;
 * correct counts argmax == y.  kd_alpha == 0: the bits of ss_tail_fwd / _w / _mix, d_logits and loss alike.  t_logits equal to
 * the row's own logits: the soft term and its gradient are exactly 0.  The logits and stashes are those of ss_tail_fwd.
 * ss_tail_bwd serves this one too. */
int ss_tail_fwd_kd(const float* h, const int32_t* lengths, const float* w_score, const float* b_score, const float* gamma,
                   const float* beta, const float* w1, const float* b1, const float* w4, const float* b4, const int64_t* y,
                   const int64_t* y_b, const float* lam, int B, int T, int D, int MID, int C, float ln_eps, float drop_p,
                   uint64_t seed, uint64_t offset, float label_smoothing, float denom, const float* cw, const float* den,
                   float* attn, float* xhat, float* rstd, float* ln, float* mid, float* mid_d, float* logits, float* d_logits,
                   float* loss_sum, int32_t* correct, const float* t_logits, int ld_t, float kd_alpha, float kd_tau,
                   ss_stream_t stream);
/* Backward of the tail from d_logits (B,C) down to d_h (B,T,D) (written) and d_mid (B,MID) (written: the input of the
 * first Linear's weight-gradient GEMM); g_gamma, g_beta (D), g_wscore (D), g_bscore (1) are accumulated -- unless
 * col_part (B,3,D) is given: then every clip STORES its terms of g_gamma | g_beta | g_wscore there and the caller adds the
 * column sums (ss_colsum_f32, lda = 3 D) to the three gradients; 256 clips' float atomics on the same D addresses serialise.  The two
 * Linear weight/bias gradients are ss_gemm_f32 calls on (d_logits, mid_d) and (d_mid, ln).  d_h behind a clip's length and
 * d_mid where the unit is dead or dropped are +0.0.  LDS: MID + D + 2 T + C <= 15 360 floats, else SS_ERR_UNSUPPORTED. */
int ss_tail_bwd(const float* h, const int32_t* lengths, const float* w_score, const float* gamma, const float* w1,
                const float* w4, const float* attn, const float* xhat, const float* rstd, const float* mid,
                const float* d_logits, int B, int T, int D, int MID, int C, float drop_p, uint64_t seed,
                uint64_t offset, float* d_mid, float* d_h, float* g_gamma, float* g_beta, float* g_wscore,
                float* g_bscore, float* col_part, ss_stream_t stream);

/* ---- a10: loss, clip, Adam -------------------------------------------------------------------
 * CrossEntropyLoss(label_smoothing) mean-reduced over `denom` clips (the GLOBAL batch under data
 * parallelism), forward and d(loss)/d(logits) in one pass (train_model_official.py:405, 434-437).
 * loss_sum (1) is accumulated: sum over this call's clips of the per-clip loss / denom.
 * correct (1) int32 accumulated: argmax == y count (train_model_official.py:442). */
int ss_ce_ls_fwd_bwd(const float* logits, const int64_t* y, int B, int C, float label_smoothing, float denom,
                     float* d_logits, float* loss_sum, int32_t* correct, ss_stream_t stream);

/* The class-weighted form (CrossEntropyLoss(weight=w, label_smoothing), train_model_official.py:406-414) with the
 * normaliser on the device: w (C) class weights, den (1) a device float = sum of w[y] over the normalising set (the rows of
 * ALL ranks' batch; ss_class_weight_sum writes it) in place of `denom`.  Per-row loss and gradient as under ss_tail_fwd_w;
 * loss_sum += sum of l / *den, correct as above; d_logits, loss_sum and correct may each be NULL.  A row whose label is
 * outside [0, C) gets a zero gradient row and adds nothing.  Every w[c] == 1 and *den == denom: the bits of ss_ce_ls_fwd_bwd. */
int ss_ce_ls_w_fwd_bwd(const float* logits, const int64_t* y, int B, int C, float label_smoothing, const float* w,
                       const float* den, float* d_logits, float* loss_sum, int32_t* correct, ss_stream_t stream);
/* The two-label loss of a mixup batch, lam * CE(logits, y) + (1 - lam) * CE(logits, y_b): y_b (B) int64, lam (1) a DEVICE float.
 * w and den both NULL: the unweighted loss over `denom`; both given: the weighted one over *den (see ss_tail_fwd_mix).  d_logits,
 * loss_sum and correct (argmax == y) may each be NULL.  A row with either label outside [0, C) gets a zero gradient row and adds
 * nothing.  *lam == 1: the bits of ss_ce_ls_fwd_bwd / ss_ce_ls_w_fwd_bwd. */
int ss_ce_ls_mix_fwd_bwd(const float* logits, const int64_t* y, const int64_t* y_b, const float* lam, int B, int C,
                         float label_smoothing, float denom, const float* w, const float* den, float* d_logits, float* loss_sum,
                         int32_t* correct, ss_stream_t stream);
/* The stand-alone form of ss_tail_fwd_kd's loss on given logits (B, C): y_b / lam and w / den each both given or both NULL;
 * t_logits (B, ld_t), kd_alpha, kd_tau and the always-required `denom` as there.  d_logits, loss_sum and correct may each be
 * NULL.  kd_alpha == 0: the bits of ss_ce_ls_fwd_bwd / _w_ / _mix_. */
int ss_ce_ls_kd_fwd_bwd(const float* logits, const int64_t* y, const int64_t* y_b, const float* lam, int B, int C,
                        float label_smoothing, float denom, const float* w, const float* den, float* d_logits, float* loss_sum,
                        int32_t* correct, const float* t_logits, int ld_t, float kd_alpha, float kd_tau, ss_stream_t stream);
/* out[0] = sum of w[y_i] over the n int64 labels y (device), written (not accumulated).  One workgroup, a fixed reduction
 * order: the result is a pure function of (the labels in order, w), so ranks that hold the same labels get the same bits.
 * A label outside [0, C) adds nothing. */
int ss_class_weight_sum(const int64_t* y, long n, const float* w, int C, float* out, ss_stream_t stream);

/* Validation kept on the device (train_model_official.py:449-475 and the confusion list of :79-91): one launch per
 * validation batch, nothing read back.  Per clip the arithmetic of ss_ce_ls_fwd_bwd with denom = 1 (same order of
 * operations, lowest index among equal maxima), accumulated into state that reduces over ranks with one collective:
 *   loss_sum (1) f32    += sum of the per-clip losses (per-wave partial sums, one float atomic per wave)
 *   correct (1) i32     += #(argmax == y)
 *   confusion (C,C) i32 [true][pred] += 1 for every row, hits included
 *   first_seen (C,C) i32 = min(first_seen, first_row + b) over the rows of the cell; the caller fills it with INT32_MAX.
 *                         first_row = position of row 0 in the evaluated set (ties of the confusion list break by it)
 *   y_true_out / y_pred_out (B) i32, each may be NULL: the label and the argmax of every row
 * A label outside [0, C) is never used as an index: the row adds nothing anywhere, both outputs get -1 and *err_flag
 * (one device word the caller owns and clears) is set to 1.  first_row < 0 or first_row + B past INT32_MAX: SS_ERR_ARG. */
int ss_eval_accum(const float* logits, const int64_t* y, int B, int C, float label_smoothing, int first_row,
                  float* loss_sum, int32_t* correct, int32_t* confusion, int32_t* first_seen, int32_t* y_true_out,
                  int32_t* y_pred_out, int32_t* err_flag, ss_stream_t stream);

/* ss_eval_accum under class weights w (C): loss_sum (1) += sum of the per-clip weighted losses l (un-normalised),
 * wsum (1) += sum of w[y] over the same clips; the weighted mean loss of a set is loss_sum / wsum, and both sums add over
 * batches and over ranks.  Everything else, rows with a label outside [0, C) (they add to neither sum) and the flag
 * included, is ss_eval_accum. */
int ss_eval_accum_w(const float* logits, const int64_t* y, int B, int C, float label_smoothing, int first_row, const float* w,
                    float* loss_sum, float* wsum, int32_t* correct, int32_t* confusion, int32_t* first_seen,
                    int32_t* y_true_out, int32_t* y_pred_out, int32_t* err_flag, ss_stream_t stream);

/* a12: softmax over the classes + the k most probable of every clip, largest first
 * (topk_from_logits, live_infer_official.py:223-226: softmax -> argsort descending -> first k).
 * probs (B,k) f32, idx (B,k) int32 (class ids; -1 / 0 when k > C). */
int ss_softmax_topk(const float* logits, int B, int C, int k, float* probs, int32_t* idx, ss_stream_t stream);

/* ss_softmax_topk at a temperature: the softmax of inv_temp[0] * logits, inv_temp a DEVICE float (u = 1 / T > 0), read by the
 * kernel -- a captured graph is replayed under a new temperature by rewriting the float, without re-capture.  Every exponent is
 * u * (l - max); inv_temp == NULL means u = 1, and with NULL or a stored 1.0f the results are the bits of ss_softmax_topk
 * (1.0f * x is exact).  The indices do not depend on u.  Everything else as ss_softmax_topk. */
int ss_softmax_topk_t(const float* logits, int B, int C, int k, const float* inv_temp, float* probs, int32_t* idx,
                      ss_stream_t stream);

/* Post-hoc temperature scaling, fitted on the device ("Calibrated confidences").  Parametrised by u = 1 / T.  Row with
 * logits z (C floats), label y, m = max z:   e_c = exp(u (z_c - m)), S0 = sum e_c, S1 = sum e_c (z_c - m),
 *   nll = log S0 - u (z_y - m),   g = d nll / du = S1 / S0 - (z_y - m);   sum g is non-decreasing in u.
 * A fit is SS_CALIB_FIT_ITERS (ss_calib_moments, ss_calib_bisect) pairs on one stream, enqueue-only; no float atomics: the same
 * inputs give the same bits on every run.
 * state (8 doubles, device): u, lo, hi, nll, g, nll_at_1, iteration, at_bound.  The caller starts it as
 *   {1, SS_CALIB_U_MIN, SS_CALIB_U_MAX, 0, 0, 0, 0, 0}.
 * ss_calib_moments: reads u = state[0]; logits (N, C) f32, y (N) int64; one wave per row, rows by grid stride over exactly
 *   n_partials workgroups (1..SS_CALIB_MAX_PARTIALS; four rows per workgroup and pass); per-row arithmetic in f32, sums over rows in
 *   f64 in a fixed order; workgroup i WRITES partials[2 i] = its sum of nll, partials[2 i + 1] = its sum of g (partials: 2 *
 *   n_partials doubles).  A label outside [0, C) is never an index: the row counts nowhere and *err_flag (one device word the caller
 *   owns and clears) is set to 1.  C >= 2.
 * ss_calib_bisect: one wave sums the partials in slot order, stores the sums as state's nll and g and advances the schedule:
 *   iteration 0 evaluated u = 1: nll_at_1 = nll, next u = U_MIN;
 *   iteration 1 evaluated U_MIN: g >= 0 -> the answer is U_MIN, at_bound = -1; else next u = U_MAX;
 *   iteration 2 evaluated U_MAX: g <= 0 -> the answer is U_MAX, at_bound = +1; else next u = sqrt(lo hi);
 *   iterations 3 .. 34: g > 0 moves hi to u, otherwise lo; next u = sqrt(lo hi) -- except after the last one, where u stays the
 *   point just evaluated (an end of the final bracket), so that nll and g are those of the u the fit returns.
 *   32 halvings of ln(U_MAX / U_MIN) = ln 400 leave 1.4e-9 of ln u, below the resolution of a float32 temperature.
 *   Once at_bound != 0, or after SS_CALIB_FIT_ITERS iterations, a call leaves the state alone. */
#define SS_CALIB_U_MIN 0.05
#define SS_CALIB_U_MAX 20.0
#define SS_CALIB_FIT_ITERS 35
#define SS_CALIB_MAX_PARTIALS 256
int ss_calib_moments(const float* logits, const int64_t* y, int N, int C, const double* state, double* partials, int n_partials,
                     int32_t* err_flag, ss_stream_t stream);
int ss_calib_bisect(double* state, const double* partials, int n_partials, ss_stream_t stream);

/* Reliability of the confidences at inverse temperature inv_temp[0] (a DEVICE float; NULL: 1).  Per row: the confidence 1 / S0
 * (the probability of the arg-max), the prediction (lowest index among equal maxima) and the rank of the true class = #{c: z_c >
 * z_y, or z_c == z_y and c < y}.  Accumulated with integer atomics only (sums that do not depend on the order and add over ranks):
 *   bin_count (n_bins) i32   [min(n_bins - 1, floor(conf * n_bins))] += 1
 *   bin_hits (n_bins) i32    the same bin += (prediction == y)
 *   bin_conf_fx (n_bins) u64 the same bin += llrint((double)conf * 2^32)
 *   rank_hist (k_max + 1) i32 [min(rank, k_max)] += 1
 * The caller clears them.  Labels outside [0, C): as ss_calib_moments.  n_bins and k_max in 1..64. */
int ss_calib_bins(const float* logits, const int64_t* y, int N, int C, const float* inv_temp, int n_bins, int k_max,
                  int32_t* bin_count, int32_t* bin_hits, uint64_t* bin_conf_fx, int32_t* rank_hist, int32_t* err_flag,
                  ss_stream_t stream);

/* sumsq (1) += sum x^2 over the flat gradient bucket (clip_grad_norm_'s global L2 norm). */
int ss_sumsq_f32(const float* x, long n, float* sumsq, ss_stream_t stream);

/* clip_grad_norm_(max_norm) folded into Adam (torch defaults, no weight decay, no amsgrad)
 * (train_model_official.py:403, 438-439): g' = g * grad_scale * min(1, max_norm / (sqrt(sumsq)*grad_scale + 1e-6)).
 * grad_scale = 1/world after a summing all-reduce.  step >= 1.  p, m, v updated in place. */
int ss_adam_clip(float* p, const float* g, float* m, float* v, long n, const float* sumsq, float grad_scale,
                 float max_norm, float lr, float beta1, float beta2, float eps, int step, ss_stream_t stream);

/* ss_adam_clip with an exponential moving average of the weights in the same pass: after p, m, v are updated exactly as
 * ss_adam_clip updates them (the same bits for the same inputs), ema[q] = ema_decay * ema[q] + (1 - ema_decay) * p[q] with the
 * p[q] just written; 1 - ema_decay is taken once, in f32.  0 <= ema_decay < 1 (0: ema becomes p).  ema (n) must not overlap p;
 * p, g, m, v, ema 16-byte aligned.  SS_ERR_ARG otherwise, and nothing is written. */
int ss_adam_clip_ema(float* p, const float* g, float* m, float* v, float* ema, long n, const float* sumsq, float grad_scale,
                     float max_norm, float lr, float beta1, float beta2, float eps, int step, float ema_decay, ss_stream_t stream);

/* Grouped AdamW: ss_adam_clip / ss_adam_clip_ema (ema != NULL) with torch's decoupled weight decay and a learning-rate scale per
 * parameter group, in the same single pass over the flat bucket.  The bucket is cut into n_seg <= 64 segments, segment s covering
 * elements [seg_end[s-1], seg_end[s]) with seg_end[-1] = 0: strictly increasing, every end but the last a multiple of 4, the last
 * equal to n.  seg_group[s] in [0, n_groups) names the segment's group, n_groups <= 8.  Per element of group G:
 *     lr_G        = float(double(lr) * double(group_lr_scale[G]))
 *     step_size_G = float(double(lr_G) / (1 - beta1^step))              (as ss_adam_clip takes it from lr)
 *     decay_G     = float(1 - double(lr_G) * double(group_weight_decay[G]))
 *     p1 = p * decay_G, rounded to f32 on its own (torch's in-place mul_; the decay is no part of the gradient)
 *     m, v, p  <-  the update of ss_adam_clip on (p1, g, m, v) with step_size_G; ema as ss_adam_clip_ema's
 * The clip coefficient is ss_adam_clip's, from the one sumsq word over the whole range.  So one segment of a group {scale 1,
 * decay 0} writes the bits of ss_adam_clip (ss_adam_clip_ema), and with all decays 0 every segment gets the bits of an
 * ss_adam_clip launch on its sub-range with lr = lr_G and the same sumsq word.  A scale of 0 leaves p at p1; m and v still move.
 * seg_end, seg_group, group_lr_scale and group_weight_decay are HOST arrays -- the first arguments of this interface that are:
 * they are read during the call and reach the kernel by value; nothing is allocated, copied to the device or kept, and the caller
 * may free or change them as soon as the call returns.  Every other pointer is device memory.
 * p, g, m, v, ema 16-byte aligned; ema must not overlap p and then 0 <= ema_decay < 1 (ema == NULL: ema_decay is ignored); scales
 * and decays finite and >= 0; step >= 1.  SS_ERR_ARG otherwise, before any launch: nothing is written. */
int ss_adamw_clip_groups(float* p, const float* g, float* m, float* v, float* ema, long n, const float* sumsq, float grad_scale,
                         float max_norm, float lr, float beta1, float beta2, float eps, int step, float ema_decay,
                         const long* seg_end, const int* seg_group, int n_seg, const float* group_lr_scale,
                         const float* group_weight_decay, int n_groups, ss_stream_t stream);

/* LAMB (You et al., "Large Batch Optimization for Deep Learning", ICLR 2020) on a flat bucket: the Adam direction plus the weight
 * decay, rescaled per segment -- one parameter tensor -- by |w| / |update|.  Bias correction on, the decay inside u (not decoupled
 * as in ss_adamw_clip_groups), no clamp on |w|, no eta, no clipping of the ratio.  The segment arrays are ss_adamw_clip_groups'
 * (HOST arrays, read during the call, handed to the kernels by value, nothing kept), with one more: seg_adapt[n_seg], nonzero where
 * the segment takes its trust ratio, 0 where it takes r = 1 (biases, LayerNorm).  With coef, inv_sqrt_bc2 as ss_adam_clip takes
 * them, bc1 = float(1 / (1 - double(beta1)^step)) and, for segment s of group G, wd_s = group_weight_decay[G] and
 * lr_s = float(double(lr) * double(group_lr_scale[G])):
 *     g'   = g * coef;   m = beta1 m + (1 - beta1) g';   v = beta2 v + (1 - beta2) g' g'       (ss_adam_clip's m and v, bit for bit)
 *     quot = m / (sqrt(v) * inv_sqrt_bc2 + eps)
 *     u    = fmaf(wd_s, p, bc1 * quot)                        (the product bc1 * quot rounded to f32 on its own)
 *     P_s  = sum p^2,  U_s = sum u^2 over the segment         (f32 squares, each widened, summed in float64 in one fixed order)
 *     r_s  = seg_adapt[s] && P_s > 0 && U_s > 0 ? float(sqrt(P_s / U_s)) : 1
 *     p    = p - (lr_s * r_s) * u                              (lr_s * r_s: one f32 product per segment);  ema as ss_adam_clip_ema's
 *
 * ss_lamb_moments: two launches.  The first streams g, m, v, p once, writes m and v, and leaves the float64 sums of p^2 and u^2 of
 * every (segment, workgroup) in scratch (ss_lamb_scratch_bytes(n, n_seg) bytes, 8-byte aligned; it need not be cleared and is
 * scratch again when the call's work is done).  The second adds each segment's partials in workgroup order and writes
 * norms[2 s] = float(sqrt(P_s)), norms[2 s + 1] = float(sqrt(U_s)) and ratio[s] (n_seg floats), all on the device.  No atomics: two
 * calls on the same inputs write the same bits.  p is only read.
 * ss_lamb_apply: one launch.  Recomputes u from the stored m, v and p -- the same expression, the same bits -- reads ratio[s] once
 * per segment and writes p and, when ema != NULL, ema (0 <= ema_decay < 1; ema must not overlap p).  It needs beta2 for
 * inv_sqrt_bc2.  seg_adapt is checked and otherwise unused here (the ratios already hold it): it is taken so that both entry points
 * are handed one and the same table.
 * p, g, m, v, ema 16-byte aligned; scales, decays and lr finite and >= 0; step >= 1; n_seg in 1..64, n_groups in 1..8; every
 * segment end but the last a multiple of 4, the last n.  SS_ERR_ARG otherwise, before any launch: nothing is written. */
int ss_lamb_scratch_bytes(long n, int n_seg, long* bytes);
int ss_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* sumsq, float grad_scale, float max_norm,
                    float beta1, float beta2, float eps, int step, const long* seg_end, const int* seg_group, int n_seg,
                    const float* group_lr_scale, const float* group_weight_decay, int n_groups, const int* seg_adapt, double* scratch,
                    float* norms, float* ratio, ss_stream_t stream);
int ss_lamb_apply(float* p, const float* m, const float* v, float* ema, long n, float beta1, float beta2, float eps, int step,
                  float ema_decay, float lr, const long* seg_end, const int* seg_group, int n_seg, const float* group_lr_scale,
                  const float* group_weight_decay, int n_groups, const int* seg_adapt, const float* ratio, ss_stream_t stream);

/* Sharpness-aware minimisation (Foret et al. 2021; adaptive: ASAM, Kwon et al. 2021) on a flat bucket, as the widely used torch
 * SAM optimiser computes it (adaptive=True, no eta): three streams around the second forward and backward of a step.
 *
 * sumsq (1) += sum (|w_i| g_i)^2: the square of ASAM's scale-invariant norm.  The walk, the workgroup count and the order of
 * adds are ss_sumsq_f32's; each product |w| g is rounded to f32 before it is squared.  w, g 16-byte aligned. */
int ss_sumsq_absw_f32(const float* w, const float* g, long n, float* sumsq, ss_stream_t stream);

/* The ascent step, one pass over n elements:  backup_i = p_i;  p_i = p_i + e_i;  g_i = +0, with
 *     scale = rho * grad_scale / (sqrt(sumsq[0]) * grad_scale + 1e-12)      (f32, from the device word: no host read)
 *     e_i   = scale * g_i               (adaptive == 0;  sumsq = sum g^2,        ss_sumsq_f32)
 *     e_i   = scale * g_i * p_i^2       (adaptive != 0;  sumsq = sum (|p| g)^2,  ss_sumsq_absw_f32)
 * grad_scale as ss_adam_clip takes it.  The launch also stores +0 to zero_f[0, n_zero_f) and 0 to zero_i[0, n_zero_i) (at most
 * 256 each; a pointer may be NULL with a count of 0): the loss sum and hit count the second pass adds onto.
 * p, g, backup 16-byte aligned; backup must overlap neither p nor g; sumsq must not be one of the cleared floats; rho finite and
 * > 0.  SS_ERR_ARG otherwise, before any launch: nothing is written. */
int ss_sam_perturb(float* p, float* g, float* backup, long n, const float* sumsq, float grad_scale, float rho, int adaptive,
                   float* zero_f, int n_zero_f, int32_t* zero_i, int n_zero_i, ss_stream_t stream);

/* Behind the second backward: p_i = backup_i bit for bit, and sumsq (1) += sum g_i^2 with the walk and the adds of ss_sumsq_f32
 * (the same bits as ss_sumsq_f32 on g).  Alignment and overlap rules of ss_sam_perturb; SS_ERR_ARG otherwise, nothing written. */
int ss_sam_restore_sumsq(float* p, const float* backup, const float* g, long n, float* sumsq, ss_stream_t stream);

/* exchanges the contents of two f32 buffers of n elements in place (the weights and their average, Trainer.ema_weights).
 * Both 16-byte aligned; ranges that overlap are SS_ERR_ARG. */
int ss_swap_f32(float* a, float* b, long n, ss_stream_t stream);

/* strided row copy dst[r*ld_dst + c] = src[r*ld_src + c], c < cols (places X into Z, train_model_official.py:297) */
int ss_copy_rows_f32(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, ss_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SS_HOTPATH_H */
