// What the f32 ROI-CNN forward (roi_cnn.hip) and backward (roi_cnn_bwd.hip) share: the compile-time LDS geometry, the weight
// sizes, the geometry dispatch, and one copy of each device routine both kernels use.  The kernels are instantiated per
// frame size so every plane / row stride is an immediate in the ds_read/ds_write offsets and every pixel -> (y, x)
// split is a multiply-shift; SS_CNN_SHAPES lists the sizes built (the reference ships 48x96, BASELINE.json's
// synthetic configs use 64x64).  No routine here holds a barrier or a wait: those stay
// in the kernels, next to the comment that says what they protect.  What the compiler made of each routine, and the
// ones it refused, are in docs/LAB_NOTES.md section 14.
#pragma once
#include "ss_common.h"

// X(H, W) for every instantiated frame size
#define SS_CNN_SHAPES(X) X(64, 64) X(48, 96) X(32, 32)

namespace {

// element counts of the weight tensors and of the operand images made from them
constexpr int W1_N = 8 * 9;         // conv1 [8][1][3][3]
constexpr int W2_ROW = 8 * 9;       // conv2, one output channel: [8][3][3]
constexpr int W2_N = 16 * W2_ROW;   // conv2 [16][8][3][3]
constexpr int W3_ROW = 16 * 9;      // conv3, one output channel: [16][3][3]
constexpr int W3_N = 24 * W3_ROW;   // conv3 [24][16][3][3]
constexpr int W3_LO = 16 * W3_ROW;  // its output channels 0..15: the ds_read_b128 part of the backward's W3 operand image
constexpr int W2T_N = 192 * 16;     // the backward's S4 operand image of W2: K = 4 rows x 3 columns x 16 channels, 16 columns

constexpr int plane_stride(int n) {  // smallest >= n that is == 18 (mod 32): conflict-free MFMA operand reads
  return n + (18 - n % 32 + 32) % 32;  // both when lanes walk pixels (stride 1) and when they walk planes
}

// one row of the st_feat stash: 24 averaged conv3 features, 24 counts of positive conv3 outputs, the frame's mean and
// standard deviation (the backward kernel would otherwise redo the pixel statistics and their f64 arithmetic per frame), pad
constexpr int ST_FEAT = 52;

template <int H_, int W_>
struct Geom {
  static constexpr int H = H_, W = W_, H2 = H_ / 2, W2 = W_ / 2, H4 = H_ / 4, W4 = W_ / 4;
  static constexpr int HW = H * W, HW2 = H2 * W2, P = H4 * W4;
  static constexpr int XS = W + 2;                              // haloed normalised image, row stride
  static constexpr int S1 = W2 + 2, P1 = plane_stride((H2 + 2) * S1);  // haloed pooled-1 map
  static constexpr int S2 = W4 + 2, P2 = plane_stride((H4 + 2) * S2);  // haloed pooled-2 map
  // pool-1 argmax bytes, plane stride per channel: 16 bytes of padding put the eight planes four LDS banks apart (the backward's S5
  // reads one byte per plane) and keep them 16-byte aligned, so the stash IS the backward kernel's LDS image and arrives by
  // linear LDS-DMA (round 3: the planes went through registers to be laid out one bank apart)
  static constexpr int I1S = HW2 + 16;
  static_assert(H % 4 == 0 && W % 32 == 0 && H2 % 2 == 0 && P % 32 == 0 && HW2 % 32 == 0, "unsupported ROI size");
};

// Per-frame sizes of the six stash arrays as THIS translation unit lays them out: a1 / a2 floats, pool-1 argmax bytes,
// pool-2 argmax bytes, conv3 sign-mask bytes, floats of an st_feat row.  The caller allocates from ss_roi_cnn_stash_size and
// hands the same six numbers to the forward and the backward entry point; each compares them with its own Geom.
constexpr int SS_CNN_STASH_SIZES = 6;
template <class G>
inline void stash_sizes_of(int* s) {
  s[0] = 8 * G::P1; s[1] = 16 * G::P2; s[2] = 8 * G::I1S; s[3] = G::P * 16; s[4] = G::P * 32; s[5] = ST_FEAT;
}
template <class G>
inline bool stash_sizes_match(const int* s) {
  int mine[SS_CNN_STASH_SIZES];
  stash_sizes_of<G>(mine);
  for (int k = 0; k < SS_CNN_STASH_SIZES; ++k)
    if (s[k] != mine[k]) return false;
  return true;
}

// ---- device routines both kernels use

// Grey-level table entry: the normalised value of the uint8 level whose fl(level / 255) is level_f (one IEEE divide per
// grey level and frame instead of one per pixel); stat = {mean, std}
__device__ __forceinline__ float xn_of_level(float level_f, int standardize, const float* stat) {
  return standardize ? (level_f - stat[0]) / stat[1] : level_f;
}

// Walk of a frame list (ss_roi_active_frames): frames[0] = how many frames to walk, frames[1 ...] their numbers, both
// clamped to the N frames the buffers hold.  Whether there is a list is the kernel's business.
__device__ __forceinline__ int listed_count(const int* frames, int N) { return min(frames[0], N); }
__device__ __forceinline__ int listed_frame(const int* frames, int N, int it) {
  return (int)min((unsigned)frames[1 + it], (unsigned)(N - 1));
}

// Pool argmax byte 2 * (row bit) + (column bit) of every lane from the two lane masks: two vector instructions
__device__ __forceinline__ int pool_index_byte(unsigned long long t1, unsigned long long b0) {
  int hi, bi;
  unsigned long long carry_out;
  asm("v_cndmask_b32_e64 %0, 0, 2, %1" : "=v"(hi) : "s"(t1));
  asm("v_addc_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(bi), "=s"(carry_out) : "v"(hi), "s"(b0));
  return bi;
}

// 1 KB piece `piece` of a linear copy of `bytes` bytes from src to LDS float offset lds_float_off: one wave instruction,
// 16 bytes per lane, lanes past the end idle.  The issuing wave waits (ss_dma_wait) before the barrier that publishes it.
__device__ __forceinline__ void dma_pieces(const char* src, int bytes, int lds_float_off, int piece, int lane) {
  const int off = piece * 1024 + lane * 16;
  if (off < bytes) ss_dma16(src + off, (unsigned)(lds_float_off * 4 + piece * 1024));
}

// f(Geom<H, W>{}) for the built shape (H, W); every entry point that takes a frame size goes through here
template <class F>
inline int for_geom(int H, int W, F&& f) {
#define SS_GEOM_CASE(HH, WW) \
  if (H == HH && W == WW) return f(Geom<HH, WW>{});
  SS_CNN_SHAPES(SS_GEOM_CASE)
#undef SS_GEOM_CASE
  return SS_ERR_UNSUPPORTED;
}

}  // namespace
