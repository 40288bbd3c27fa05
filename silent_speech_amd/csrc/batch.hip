// Batch assembly on the device: clips stay resident in HBM as one ragged frame store, a training batch is a
// gather of frame rows into the padded (B, max_t, ...) tensors the model takes.
//
// Replaces what NPZWordDataset.__getitem__ and collate_fn do per clip on the host
// (/root/reference/train_model_official.py:122-204): additive feature noise (:143-145), interior frame drop
// (:146-152, expressed as a frame map), zero padding / trimming to max_t (:93-118), stacking (:174-204).  Which
// frames go where is a (B, max_t) int32 map, -1 = padding; the bytes never leave the GPU.
// The gathers are pure HBM streams: 16 bytes per lane, one row per wave group.  The map comes from the host
// (rng "reference" / "device") or from the planning kernels below them: the epoch's class-balanced sample order
// (:382-397) and the augmentation draws + maps of a batch, both on the Philox stream, nothing crossing PCIe.
//
// Ten kernels behind the thirteen entry points:
//   batch_gather_f32_kernel<HOST_NOISE, SCALE>  ss_batch_gather_f32 (<true, false> with a noise table, else <false, false>),
//                                               ss_batch_gather_f32_at (<false, false>), ss_batch_gather_f32_aug (<false, true>)
//   batch_gather_z_kernel<W>                    ss_batch_gather_z (W = 4: 16 bytes per lane; W = 1: any row geometry)
//   batch_gather_u8_kernel                      ss_batch_gather_u8
//   batch_gather_u8_shift_kernel<WIDE>          ss_batch_gather_u8_shift (WIDE: W % 16 == 0)
//   epoch_sample_kernel                         ss_epoch_sample
//   batch_plan_kernel<POLICY>                   ss_batch_plan (<false>), ss_batch_plan_aug (<true>)
//   batch_plan_mask_kernel                      ss_batch_plan_mask (behind either planner: edits its maps in place)
//   batch_mask_apply_kernel                     ss_batch_mask_apply (behind the gathers: writes the masked bytes only)
//   batch_plan_mixup_kernel                     ss_batch_plan_mixup (behind the planners: the batch's factor, partners, second labels)
//   batch_mixup_kernel<W>                       ss_batch_mixup (behind everything else: the blended batch, out of place)
#include "ss_common.h"

namespace {

// Four N(0,1) values of the feature-noise stream: Philox block `ctr` under `seed`, two Box-Muller pairs from four uniforms in
// (0, 1].  Returned by value: the callers select among named components, nothing is indexed at run time.
__device__ __forceinline__ float4 gather_noise4(uint64_t ctr, uint64_t seed) {
  uint32_t rnd[4];
  philox4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0x6e6f6973u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), rnd);
  const float u0 = ((float)rnd[0] + 1.0f) * 2.3283064e-10f, u1 = (float)rnd[1] * 2.3283064e-10f;
  const float u2 = ((float)rnd[2] + 1.0f) * 2.3283064e-10f, u3 = (float)rnd[3] * 2.3283064e-10f;
  const float ra = sqrtf(-2.0f * __logf(u0)), rb = sqrtf(-2.0f * __logf(u2));
  return float4{ra * __cosf(6.2831853f * u1), ra * __sinf(6.2831853f * u1), rb * __cosf(6.2831853f * u3),
                rb * __sinf(6.2831853f * u3)};
}

// The f32 gather, one template for the three entry points:
//   dst[r][:] = ((map[r] >= 0 ? src[map[r]][:] : 0) + noise term) * scale term.
// Noise term, HOST_NOISE (ss_batch_gather_f32 with a noise table): noise[noise_map[r]][:] on every row with noise_map[r] >= 0
//   (host-drawn, the reference's np.random.normal); no Philox in this instantiation.
// Noise term, !HOST_NOISE: noise_std * N(0,1) on the rows with map[r] >= 0 and noise_map[r] >= 0 (a NULL noise_map or
//   noise_std == 0: none).  Element q of dst is element noise_first + q of the stream (seed, element index); four elements
//   share a Philox block.  noise_first is 0 for ss_batch_gather_f32; for a batch that is rows [first, first + rows) of a
//   larger one (a data-parallel rank's shard of the global batch; _at and _aug) it is that batch's element offset, so the shards
//   of all ranks, put together, are the batch a single process gathers, bit for bit.  It need not be a multiple of 4: a 16-byte
//   chunk of dst then takes its four values from two neighbouring blocks (the second one is drawn only then).
// Scale term, SCALE (ss_batch_gather_f32_aug, the augmentation policy's scale jitter): row r of dst belongs to clip
//   r / rows_per_clip, and x_after_noise * row_scale[clip] is one rounded product (__fmul_rn: no contraction with the noise
//   term, so NumPy's fl(x * s) restates it).  Padding rows stay 0.  Without SCALE row_scale is never read.
template <bool HOST_NOISE, bool SCALE>
__global__ __launch_bounds__(256) void batch_gather_f32_kernel(const float* __restrict__ src, int D,
                                                               const int32_t* __restrict__ frame_map, long rows,
                                                               const float* __restrict__ noise,
                                                               const int32_t* __restrict__ noise_map, float noise_std,
                                                               uint64_t seed, uint64_t noise_first,
                                                               const float* __restrict__ row_scale, int rows_per_clip,
                                                               float* __restrict__ dst) {
  const long total = rows * D;
  const bool philox = !HOST_NOISE && noise_map && noise_std > 0.f;
  const int shift = (int)(noise_first & 3);  // the same for every chunk
  for (long q = ((long)blockIdx.x * 256 + threadIdx.x) * 4; q < total; q += (long)gridDim.x * 256 * 4) {
    // D need not be a multiple of 4: walk the four elements of this 16-byte destination chunk
    float v[4], sc[4];
    unsigned noisy = 0;  // bit e: element e takes Philox noise
    long r = q / D;           // one division per 16-byte chunk, then walk
    int d = (int)(q - r * D);
    float s = 1.0f;
    if constexpr (SCALE) s = row_scale[r / rows_per_clip];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = 0.f;
      if (q + e < total) {
        const int m = frame_map[r];
        if (m >= 0) x = src[(long)m * D + d];
        const int nm = noise_map ? noise_map[r] : -1;
        if constexpr (HOST_NOISE) {
          if (nm >= 0) x += noise[(long)nm * D + d];
        } else {
          noisy |= (unsigned)(m >= 0 && nm >= 0) << e;
        }
      }
      v[e] = x;
      sc[e] = s;
      if (++d == D) {
        d = 0;
        ++r;
        if constexpr (SCALE)
          if (r < rows) s = row_scale[r / rows_per_clip];
      }
    }
    if (philox) {
      const uint64_t ctr = (noise_first + (uint64_t)q) >> 2;
      auto add = [&](int e, float n) {
        if (noisy >> e & 1) v[e] += noise_std * n;
      };
      // element e takes value shift + e of the eight that this block and the next one hold; this block's share is added
      // before the next block is drawn, so the two are never live together
      const float4 a = gather_noise4(ctr, seed);
      switch (shift) {
        case 0: add(0, a.x); add(1, a.y); add(2, a.z); add(3, a.w); break;
        case 1: add(0, a.y); add(1, a.z); add(2, a.w); break;
        case 2: add(0, a.z); add(1, a.w); break;
        default: add(0, a.w);
      }
      if (shift) {
        const float4 b = gather_noise4(ctr + 1, seed);
        switch (shift) {
          case 1: add(3, b.x); break;
          case 2: add(2, b.x); add(3, b.y); break;
          default: add(1, b.x); add(2, b.y); add(3, b.z);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q + e < total) dst[q + e] = SCALE ? __fmul_rn(v[e], sc[e]) : v[e];
  }
}

// component k (0..3) of a float4 by selects: nothing is indexed at run time, so nothing goes to scratch
__device__ __forceinline__ float pick4(const float4 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// Rows of a frozen-CNN training batch (ss_batch_gather_z): dst[r] = feature row | embedding row, ld_dst >= D + E floats apart,
// the columns behind D + E left alone.
//   [0, D)      what batch_gather_f32_kernel<false, SCALE> writes to row r of a dense (rows, D) destination, bit for bit: element
//               (r, c) is element n = noise_first + r * D + c of the noise stream -- component n & 3 of Philox block n >> 2, which is
//               what that kernel's chunk walk hands the same element -- added as noise_std * N in the same expression form (one
//               contracted multiply-add), then one rounded product with row_scale[r / rows_per_clip] (row_scale NULL: none).
//   [D, D + E)  emb[rmap[r]] where rmap[r] >= 0, else emb_fill (NULL: zeros); rmap NULL: the fill on every row.
// One lane per W consecutive elements of a row, W = 4 (one 16-byte load and store per lane; D, E, ld_dst multiples of 4 and every
// base 16-byte aligned, so a chunk lies inside one half of the row and its noise inside two neighbouring blocks) or W = 1 (any
// geometry: x_dim = 83 exists in the reference's lineage).
template <int W>
__global__ __launch_bounds__(256) void batch_gather_z_kernel(const float* __restrict__ feat, int D,
                                                             const int32_t* __restrict__ xmap, const float* __restrict__ emb,
                                                             int E, const int32_t* __restrict__ rmap,
                                                             const float* __restrict__ emb_fill, long rows,
                                                             const int32_t* __restrict__ noise_map, float noise_std,
                                                             uint64_t seed, uint64_t noise_first,
                                                             const float* __restrict__ row_scale, int rows_per_clip,
                                                             float* __restrict__ dst, int ld_dst) {
  static_assert(W == 1 || W == 4, "one element or one 16-byte chunk per lane");
  const int units = (D + E) / W;  // per row
  const long total = rows * units;
  const bool philox = noise_map && noise_std > 0.f;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)gridDim.x * 256) {
    const long r = u / units;  // one division per lane and 16-byte chunk, as in the f32 gather
    const int c = (int)(u - r * units) * W;
    float v[W];
    if (c < D) {
      const int m = xmap[r];
      const float* s = feat + (long)(m < 0 ? 0 : m) * D + c;
      if constexpr (W == 4) {
        const float4 x = m >= 0 ? *reinterpret_cast<const float4*>(s) : float4{0.f, 0.f, 0.f, 0.f};
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
      } else {
        v[0] = m >= 0 ? *s : 0.f;
      }
      if (philox && m >= 0 && noise_map[r] >= 0) {
        const uint64_t n0 = noise_first + (uint64_t)(r * D + c);
        const int shift = (int)(n0 & 3);
        const float4 a = gather_noise4(n0 >> 2, seed);
#pragma unroll
        for (int e = 0; e < W; ++e)
          if (shift + e < 4) v[e] += noise_std * pick4(a, shift + e);
        if (shift + W > 4) {  // (W == 4 and noise_first & 3 != 0: the same for every chunk)
          const float4 b = gather_noise4((n0 >> 2) + 1, seed);
#pragma unroll
          for (int e = 0; e < W; ++e)
            if (shift + e >= 4) v[e] += noise_std * pick4(b, shift + e - 4);
        }
      }
      if (row_scale) {
        const float sc = row_scale[r / rows_per_clip];
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = __fmul_rn(v[e], sc);
      }
    } else {
      const int m = rmap ? rmap[r] : -1;
      const float* s = m >= 0 ? emb + (long)m * E + (c - D) : emb_fill ? emb_fill + (c - D) : nullptr;
      if constexpr (W == 4) {
        const float4 x = s ? *reinterpret_cast<const float4*>(s) : float4{0.f, 0.f, 0.f, 0.f};
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
      } else {
        v[0] = s ? *s : 0.f;
      }
    }
    float* d = dst + r * ld_dst + c;
    if constexpr (W == 4)
      *reinterpret_cast<float4*>(d) = float4{v[0], v[1], v[2], v[3]};
    else
      *d = v[0];
  }
}

// dst[r][0:frame_bytes] = map[r] >= 0 ? src[map[r]] : 0; frame_bytes % 16 == 0, one workgroup walks whole rows
__global__ __launch_bounds__(256) void batch_gather_u8_kernel(const uint8_t* __restrict__ src, int chunks /* 16-byte */,
                                                              const int32_t* __restrict__ frame_map, long rows,
                                                              uint8_t* __restrict__ dst) {
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int m = frame_map[r];
    const uint4* s4 = reinterpret_cast<const uint4*>(src) + (long)(m < 0 ? 0 : m) * chunks;
    uint4* d4 = reinterpret_cast<uint4*>(dst) + r * chunks;
    for (int c = threadIdx.x; c < chunks; c += 256) d4[c] = m >= 0 ? s4[c] : uint4{0, 0, 0, 0};
  }
}

// The gather above with a per-clip integer shift of the frame, edges replicated (the augmentation policy's ROI jitter):
//   dst[r][y][x] = src[map[r]][clamp(y - dy, 0, H-1)][clamp(x - dx, 0, W-1)],  (dx, dy) = row_shift[2 * (r / rows_per_clip)].
// Still an HBM stream: one workgroup walks whole frames, one 16-byte store per lane.  WIDE (W % 16 == 0): a destination chunk
// lies inside one image row, its 16 source bytes start at byte x0 - dx of the (clamped) source row.  Where that run lies inside
// the row it is fetched whole (load16_at); only the chunks that reach over the left or right edge go byte by byte, every
// byte address clamped into the row.  !WIDE: every byte on its own (correctness for odd widths, not speed).  No load touches a
// byte outside [src + map[r] * H * W, + H * W): row and column are clamped before any address is formed, and dx, dy
// themselves are clamped to +-W, +-H first (the same result, and no overflow whatever the table holds).
struct __attribute__((packed, aligned(1))) bytes16 { uint32_t w[4]; };  // a 16-byte load the compiler may not assume aligned

// 16 bytes from byte offset `at` of a row, 0 <= at and at + 16 <= row length: ONE global load at the byte address.  (Measured
// against two aligned 16-byte loads + v_alignbyte: never slower, 3 - 7 % faster where clips are shifted)
__device__ __forceinline__ uint4 load16_at(const uint8_t* __restrict__ row, int at) {
  const bytes16 b = *reinterpret_cast<const bytes16*>(row + at);
  return uint4{b.w[0], b.w[1], b.w[2], b.w[3]};
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <bool WIDE>
__global__ __launch_bounds__(256) void batch_gather_u8_shift_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                                    const int32_t* __restrict__ frame_map, long rows,
                                                                    const int32_t* __restrict__ row_shift, int rows_per_clip,
                                                                    uint8_t* __restrict__ dst) {
  const int chunks = (H * W) >> 4;
  const int row_chunks = W >> 4;  // WIDE only
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int m = frame_map[r];
    uint4* d4 = reinterpret_cast<uint4*>(dst) + r * chunks;
    if (m < 0) {
      for (int c = threadIdx.x; c < chunks; c += 256) d4[c] = uint4{0, 0, 0, 0};
      continue;
    }
    const long clip = r / rows_per_clip;
    const int dx = clampi(row_shift[2 * clip], -W, W), dy = clampi(row_shift[2 * clip + 1], -H, H);
    const uint8_t* frame = src + (long)m * H * W;
    for (int c = threadIdx.x; c < chunks; c += 256) {
      uint32_t o[4];
      if constexpr (WIDE) {
        const int y = (int)((uint32_t)c / (uint32_t)row_chunks);
        const int x0 = (c - y * row_chunks) << 4;
        const uint8_t* row = frame + clampi(y - dy, 0, H - 1) * W;
        const int at = x0 - dx;
        if (at >= 0 && at + 16 <= W) {
          d4[c] = load16_at(row, at);
          continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t word = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) word |= (uint32_t)row[clampi(at + 4 * i + j, 0, W - 1)] << (8 * j);
          o[i] = word;
        }
      } else {
        int y = (int)((uint32_t)(c << 4) / (uint32_t)W);
        int x = (c << 4) - y * W;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t word = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            word |= (uint32_t)frame[clampi(y - dy, 0, H - 1) * W + clampi(x - dx, 0, W - 1)] << (8 * j);
            if (++x == W) { x = 0; ++y; }
          }
          o[i] = word;
        }
      }
      d4[c] = uint4{o[0], o[1], o[2], o[3]};
    }
  }
}

// ---- planning on the device.  One Philox4x32-10 block per draw: counter = (draw index low, high, domain tag, sub-draw),
// key = the 64-bit seed.  Every decision is integer arithmetic on the 32-bit outputs, so tests/batch_plan_ref.py restates
// it bit for bit: mulhi(r, n) is a uniform integer below n, a probability is the threshold (uint32)(p * 2^32) computed in
// double on the host (as drop_scale4 does), carried in 64 bits so that p = 1 stays "always".
constexpr uint32_t TAG_SAMPLER = 0x73616d70u;  // "samp"
constexpr uint32_t TAG_PLANNER = 0x706c616eu;  // "plan"

__device__ __forceinline__ uint32_t mulhi_u32(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// WeightedRandomSampler(1 / count(label), replacement=True) (train...:382-397): a uniform class among those present, then a
// uniform member of it
__global__ __launch_bounds__(256) void epoch_sample_kernel(const int32_t* __restrict__ members, int n_members,
                                                           const int32_t* __restrict__ class_start, int n_classes,
                                                           uint64_t first, long count, uint64_t seed,
                                                           int32_t* __restrict__ indices) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const uint64_t j = first + (uint64_t)k;
  uint32_t r[4];
  philox4((uint32_t)j, (uint32_t)(j >> 32), TAG_SAMPLER, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const int cls = (int)mulhi_u32(r[0], (uint32_t)n_classes);
  const int lo = class_start[cls], size = class_start[cls + 1] - lo;
  // a table that is not what the store builds (empty class, offsets past the end) gives -1, which the planner reports
  const long at = (lo >= 0 && size > 0) ? (long)lo + mulhi_u32(r[1], (uint32_t)size) : -1;
  indices[k] = (at >= 0 && at < n_members) ? members[at] : -1;
}

// What ss_batch_plan_aug takes beyond ss_batch_plan: the policy's thresholds and ranges, and where the per-clip scale factor
// and ROI shift go
struct PlanPolicy {
  uint64_t warp_thr;
  int warp_lo_pm, warp_hi_pm;
  uint64_t scale_thr;
  float scale_lo, scale_span;
  uint64_t shift_thr;
  int shift_max_x, shift_max_y;
  float* row_scale;
  int32_t* row_shift;
};

// The plan of a batch, one template for ss_batch_plan (POLICY false) and ss_batch_plan_aug (POLICY true).  One wave per batch
// row, lanes over t (every lane makes the row's few draws itself: cheaper than a broadcast).  Sub-draw 0 decides noise and
// drop, sub-draw 1 the second dropped frame.  POLICY adds the augmentation policy from sub-draws 2 (w) and 3 (s): a time warp
// of the whole clip (features and ROI frames together; the drop then acts on the warped length Lw), a scale factor for the
// features and an integer shift for the ROI frames.  Warped position j of a clip of T frames warped to Lw reads source frame
// Wp(j) = j * (T - 1) / (Lw - 1) (integer division; j when Lw == T).  Without POLICY Lw == T, and neither those two Philox
// blocks nor the warp arithmetic nor the row_scale / row_shift stores exist; with its three probabilities 0 the policy
// instantiation writes the same plan.
template <bool POLICY>
__global__ __launch_bounds__(SS_WAVE) void batch_plan_kernel(
    const int32_t* __restrict__ indices, const int32_t* __restrict__ x_off, const int32_t* __restrict__ x_len,
    const int32_t* __restrict__ r_off, const int32_t* __restrict__ r_len, const int64_t* __restrict__ y, int n_clips,
    int max_t, int augment, uint64_t first_row, uint64_t seed, uint64_t noise_thr, uint64_t drop_thr, int drop_max,
    PlanPolicy pol, int32_t* __restrict__ xmap, int32_t* __restrict__ nmap, int32_t* __restrict__ rmap,
    int64_t* __restrict__ lens, int64_t* __restrict__ y_out, int32_t* __restrict__ err_flag) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int clip = indices[b];
  const bool valid = clip >= 0 && clip < n_clips;  // anything else is never dereferenced: an empty row and the flag
  int xo = 0, ro = -1, t_eff = 0, k = 0, d0 = 0, d1 = 0, T = 0, Lw = 0, dx = 0, dy = 0;
  float scale = 1.0f;
  bool noisy = false;
  if (valid) {
    T = x_len[clip];
    Lw = T;
    xo = x_off[clip];
    const bool has_roi = r_off && r_off[clip] >= 0;
    if (augment) {
      const uint64_t row = first_row + (uint64_t)b;
      const uint32_t r0 = (uint32_t)row, r1 = (uint32_t)(row >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
      uint32_t r[4];
      philox4(r0, r1, TAG_PLANNER, 0u, k0, k1, r);
      noisy = (uint64_t)r[0] < noise_thr;
      if constexpr (POLICY) {
        uint32_t w[4], s[4];
        philox4(r0, r1, TAG_PLANNER, 2u, k0, k1, w);
        philox4(r0, r1, TAG_PLANNER, 3u, k0, k1, s);
        if (T > 10 && (uint64_t)w[0] < pol.warp_thr) {
          const long f = pol.warp_lo_pm + (long)mulhi_u32(w[1], (uint32_t)(pol.warp_hi_pm - pol.warp_lo_pm + 1));
          const long l = (long)T * f / 1000;
          Lw = l < 5 ? 5 : l > 0x7fffffffL ? 0x7fffffff : (int)l;
        }
        if ((uint64_t)w[2] < pol.scale_thr) {
          const float u = (float)(w[3] >> 8) * 5.9604644775390625e-8f;  // 24 bits: exact
          scale = __fadd_rn(pol.scale_lo, __fmul_rn(pol.scale_span, u));
        }
        if (has_roi && (uint64_t)s[0] < pol.shift_thr) {
          dx = (int)mulhi_u32(s[1], (uint32_t)(2 * pol.shift_max_x + 1)) - pol.shift_max_x;
          dy = (int)mulhi_u32(s[2], (uint32_t)(2 * pol.shift_max_y + 1)) - pol.shift_max_y;
        }
      }
      if (Lw > 12 && (uint64_t)r[1] < drop_thr) {  // interior frames only: 0 and Lw-1 stay (train...:148)
        k = 1 + (int)mulhi_u32(r[2], (uint32_t)drop_max);
        d0 = 1 + (int)mulhi_u32(r[3], (uint32_t)(Lw - 2));
        if (k == 2) {  // the second one uniform over the other Lw-3 interior frames: every pair equally likely
          uint32_t q[4];
          philox4(r0, r1, TAG_PLANNER, 1u, k0, k1, q);
          int p1 = 1 + (int)mulhi_u32(q[0], (uint32_t)(Lw - 3));
          p1 += (p1 >= d0);
          d1 = p1 > d0 ? p1 : d0;
          d0 = p1 > d0 ? d0 : p1;
        }
      }
    }
    t_eff = Lw - k < max_t ? Lw - k : max_t;  // clip_pad_trim
    if (t_eff < 0) t_eff = 0;
    if (has_roi) {  // T_use = min(T_eff, n_r, max_t); the ROI frames are NOT dropped
      ro = r_off[clip];
      const int tr = r_len[clip] > 0 ? r_len[clip] : 0;
      int n_r = tr;  // the positions the ROI track has a frame for; of a warped clip: those whose source frame it has
      if constexpr (POLICY) n_r = tr >= T ? Lw : tr == 0 ? 0 : (int)(((long)tr * (Lw - 1) + T - 2) / (T - 1));
      t_eff = t_eff < n_r ? t_eff : n_r;
    }
  }
  const bool warped = POLICY && Lw != T;  // (then T > 10 and Lw >= 5: no division by zero)
  for (int t = lane; t < max_t; t += SS_WAVE) {
    const bool in = t < t_eff;
    int s = t;
    s += (k >= 1 && s >= d0);
    s += (k == 2 && s >= d1);
    int fx = s, fr = t;
    if (warped && in) {
      fx = (int)((long)s * (T - 1) / (Lw - 1));
      fr = (int)((long)t * (T - 1) / (Lw - 1));
    }
    const long at = (long)b * max_t + t;
    xmap[at] = in ? xo + fx : -1;
    nmap[at] = (in && noisy) ? 0 : -1;
    if (rmap) rmap[at] = (in && ro >= 0) ? ro + fr : -1;
  }
  if (lane == 0) {
    lens[b] = t_eff;
    y_out[b] = valid ? y[clip] : 0;
    if constexpr (POLICY) {
      pol.row_scale[b] = scale;
      pol.row_shift[2 * b] = dx;
      pol.row_shift[2 * b + 1] = dy;
    }
    if (!valid) atomicOr(err_flag, 1);  // (a vector atomic; the flag's owner clears it when it reads it)
  }
}

// ---- the masking augmentations (AugmentPolicy: time mask, feature band, ROI cutout).  Two launches beside the kernels above,
// none of which changes: the plan of the masks edits the maps a planner has written, the apply step overwrites the masked
// columns and rectangles of what the gathers have written.
struct MaskPolicy {
  uint64_t time_thr;
  int time_max, streams /* 0 both, 1 features, 2 roi */, hold;
  uint64_t band_thr;
  int band_max;
  uint64_t cut_thr;
  int cut_max_w, cut_max_h;
};

// One wave per batch row, lanes over t, as the planner; row b draws the planner's own counter (first_row + b, "plan", seed),
// sub-draws 4 (m: time mask), 5 (c: feature band, cutout decision) and 6 (q: cutout rectangle).  n = lens[b] is what the
// planner left; the run [t0, t0 + tw) lies in [1, n), so frame 0 stays and lens is only read.  "zero": the entries of the run
// become -1 (features: xmap and nmap); "hold": they become entry t0 - 1, which lies before the run and is written by nobody here
// (nmap stays: a repeated row takes fresh noise).  A maximum of 0 switches its mask off; an inactive mask is width 0 at position
// 0, an empty row eight zeros.  row_mask[b] = {t0, tw, col0, cw, x0, y0, rw, rh}.
__global__ __launch_bounds__(SS_WAVE) void batch_plan_mask_kernel(int32_t* xmap, int32_t* nmap, int32_t* rmap,
                                                                  const int64_t* __restrict__ lens, int max_t, int D, int H, int W,
                                                                  int augment, uint64_t first_row, uint64_t seed, MaskPolicy pol,
                                                                  int32_t* __restrict__ row_mask) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long base = (long)b * max_t;
  const int64_t len = lens[b];
  const int n = len < 0 ? 0 : len > max_t ? max_t : (int)len;
  int t0 = 0, tw = 0, col0 = 0, cw = 0, x0 = 0, y0 = 0, rw = 0, rh = 0;
  if (augment && n > 0) {
    const bool has_roi = rmap && rmap[base] >= 0;  // (entry 0 is never masked)
    const uint64_t row = first_row + (uint64_t)b;
    const uint32_t r0 = (uint32_t)row, r1 = (uint32_t)(row >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (pol.time_thr && pol.time_max >= 1 && n >= 8) {
      uint32_t m[4];
      philox4(r0, r1, TAG_PLANNER, 4u, k0, k1, m);
      if ((uint64_t)m[0] < pol.time_thr) {
        const int cap = pol.time_max < n / 4 ? pol.time_max : n / 4;
        tw = 1 + (int)mulhi_u32(m[1], (uint32_t)cap);
        t0 = 1 + (int)mulhi_u32(m[2], (uint32_t)(n - tw));
      }
    }
    const bool band_on = pol.band_thr && pol.band_max >= 1;
    const bool cut_on = pol.cut_thr && pol.cut_max_w >= 1 && pol.cut_max_h >= 1 && has_roi;
    if (band_on || cut_on) {
      uint32_t c[4];
      philox4(r0, r1, TAG_PLANNER, 5u, k0, k1, c);
      if (band_on && (uint64_t)c[0] < pol.band_thr) {
        cw = 1 + (int)mulhi_u32(c[1], (uint32_t)(pol.band_max < D ? pol.band_max : D));
        col0 = (int)mulhi_u32(c[2], (uint32_t)(D - cw + 1));
      }
      if (cut_on && (uint64_t)c[3] < pol.cut_thr) {
        uint32_t q[4];
        philox4(r0, r1, TAG_PLANNER, 6u, k0, k1, q);
        rw = 1 + (int)mulhi_u32(q[0], (uint32_t)(pol.cut_max_w < W ? pol.cut_max_w : W));
        rh = 1 + (int)mulhi_u32(q[1], (uint32_t)(pol.cut_max_h < H ? pol.cut_max_h : H));
        x0 = (int)mulhi_u32(q[2], (uint32_t)(W - rw + 1));
        y0 = (int)mulhi_u32(q[3], (uint32_t)(H - rh + 1));
      }
    }
    if (tw) {
      const bool feat = pol.streams != 2, roi = pol.streams != 1 && rmap;
      int hx = -1, hr = -1;
      if (pol.hold) {
        if (feat) hx = xmap[base + t0 - 1];
        if (roi) hr = rmap[base + t0 - 1];
      }
      for (int t = t0 + lane; t < t0 + tw; t += SS_WAVE) {
        if (feat) {
          xmap[base + t] = hx;
          if (!pol.hold) nmap[base + t] = -1;
        }
        if (roi) rmap[base + t] = hr;
      }
    }
  }
  if (lane < 8) {
    const int v = lane == 0 ? t0 : lane == 1 ? tw : lane == 2 ? col0 : lane == 3 ? cw : lane == 4 ? x0 : lane == 5 ? y0
                : lane == 6 ? rw : rh;
    row_mask[(long)b * 8 + lane] = v;
  }
}

// The band and the rectangle of row_mask written over what the gathers left, in place: one wave per row r of the batch (clip
// r / rows_per_clip), so the launch reads the two tables and writes the masked bytes -- it is not a pass over X or R.
//   X[r][col0, col0 + cw) = 0.0f (X NULL: skipped);  R[r][y0, y0 + rh)[x0, x0 + rw) = fill where rmap[r] >= 0 (R NULL: skipped).
// Position and width are clamped into the row and the frame before any address is formed, whatever the table holds.  A run of
// the rectangle inside one image row goes as the bytes up to the next 4-byte address, whole dwords, and the bytes left over:
// chunk 0 is the head, chunk k >= 1 the k-th dword behind it; a power-of-two group of lanes takes the chunks of one image row,
// the groups of the wave take the image rows.  No byte outside the rectangle is read or written.
__global__ __launch_bounds__(256) void batch_mask_apply_kernel(float* __restrict__ X, int ld_x, int D, uint8_t* __restrict__ R,
                                                               int H, int W, const int32_t* __restrict__ rmap,
                                                               const int32_t* __restrict__ row_mask, long rows, int rows_per_clip,
                                                               int fill) {
  const int lane = threadIdx.x & (SS_WAVE - 1), wave = threadIdx.x / SS_WAVE;
  const uint32_t fill4 = 0x01010101u * (uint32_t)fill;
  for (long r = (long)blockIdx.x * 4 + wave; r < rows; r += (long)gridDim.x * 4) {
    const int32_t* m = row_mask + 8 * (r / rows_per_clip);
    if (X) {
      const int col0 = clampi(m[2], 0, D), cw = clampi(m[3], 0, D - col0);
      float* x = X + r * ld_x + col0;
      for (int c = lane; c < cw; c += SS_WAVE) x[c] = 0.f;
    }
    if (R) {
      const int x0 = clampi(m[4], 0, W), y0 = clampi(m[5], 0, H);
      const int rw = clampi(m[6], 0, W - x0), rh = clampi(m[7], 0, H - y0);
      if (rw == 0 || rh == 0 || rmap[r] < 0) continue;
      uint8_t* frame = R + r * ((long)H * W);
      const int chunks = (rw + 3) / 4 + 1;
      int shift = 0;  // lanes per image row: the power of two that holds the chunks, at most the wave
      while ((1 << shift) < chunks && shift < 6) ++shift;
      const int sub = 1 << shift, lx = lane & (sub - 1), ly = lane >> shift;
      for (int y = ly; y < rh; y += SS_WAVE >> shift) {
        uint8_t* s = frame + (long)(y0 + y) * W + x0;
        const int head = (int)((4 - (reinterpret_cast<uintptr_t>(s) & 3)) & 3);
        for (int k = lx; k < chunks; k += sub) {
          const int lo = k == 0 ? 0 : head + 4 * (k - 1);
          int hi = k == 0 ? head : lo + 4;
          hi = hi < rw ? hi : rw;
          if (hi - lo == 4) {
            *reinterpret_cast<uint32_t*>(s + lo) = fill4;  // (k >= 1: s + lo is a 4-byte address)
          } else {
            for (int i = lo; i < hi; ++i) s[i] = (uint8_t)fill;
          }
        }
      }
    }
  }
}

// ---- mixup (AugmentPolicy: mixup_prob, mixup_alpha; inactive/train_reduced.py:36-53 mixes the collated batch).  One factor per
// batch, lam = k / 256 with k an integer in [0, 256] from a table of Beta(alpha, alpha) quantiles, one partner row per row.
constexpr uint32_t TAG_MIXUP = 0x6d697870u;  // "mixp"
constexpr int MIXUP_MAX_B = 1024;

// One workgroup plans the batch.  Counter (first_row, "mixp", 0) decides the batch: mixed iff augment && u0 < thr, then
// k = table[mulhi(u1, N)]; counter (first_row + b, "mixp", 1) gives row b one 32-bit key, and perm[b] is the rank of (key_b, b)
// among the rows -- a stable argsort, every thread counting the keys in LDS that order before its own (B <= 1024: at most 4 x 1024
// compares per thread).  Not mixed: the identity, k = 256.  y_b = y[perm], lens_m = max(lens, lens[perm]).
__global__ __launch_bounds__(256) void batch_plan_mixup_kernel(const int64_t* __restrict__ lens, const int64_t* __restrict__ y, int B,
                                                               int augment, uint64_t first_row, uint64_t seed, uint64_t mix_thr,
                                                               const uint16_t* __restrict__ table, int N,
                                                               int32_t* __restrict__ perm, int64_t* __restrict__ y_b,
                                                               int64_t* __restrict__ lens_m, int32_t* __restrict__ k_out,
                                                               float* __restrict__ lam_out) {
  __shared__ uint32_t keys[MIXUP_MAX_B];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t u[4];
  philox4((uint32_t)first_row, (uint32_t)(first_row >> 32), TAG_MIXUP, 0u, k0, k1, u);
  const bool mixed = augment && (uint64_t)u[0] < mix_thr;
  int k = 256;
  if (mixed) {
    k = table[mulhi_u32(u[1], (uint32_t)N)];
    k = k > 256 ? 256 : k;
  }
  for (int b = threadIdx.x; b < B; b += 256) {
    const uint64_t row = first_row + (uint64_t)b;
    uint32_t r[4];
    philox4((uint32_t)row, (uint32_t)(row >> 32), TAG_MIXUP, 1u, k0, k1, r);
    keys[b] = r[0];
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    int p = b;
    if (mixed) {
      const uint32_t mine = keys[b];
      p = 0;
      for (int j = 0; j < B; ++j) {
        const uint32_t other = keys[j];
        p += (other < mine || (other == mine && j < b));
      }
    }
    perm[b] = p;
    y_b[b] = y[p];
    const int64_t la = lens[b], lb = lens[p];
    lens_m[b] = la > lb ? la : lb;
  }
  if (threadIdx.x == 0) {
    k_out[0] = k;
    lam_out[0] = (float)k * 0.00390625f;  // k / 256: exact
  }
}

// bytes a and b blended by k / 256, four at a time: (k a + (256 - k) b + 128) >> 8 per byte.  Even and odd bytes each sit in
// their own 16-bit lane of a dword, where the sum is at most 255 * 256 + 128 < 2^16: no carry leaves a lane.
__device__ __forceinline__ uint32_t mix_bytes4(uint32_t a, uint32_t b, uint32_t k) {
  const uint32_t m = 0x00ff00ffu, half = 0x00800080u, nk = 256u - k;
  const uint32_t even = ((a & m) * k + (b & m) * nk + half) >> 8 & m;
  const uint32_t odd = (((a >> 8) & m) * k + ((b >> 8) & m) * nk + half) & ~m;
  return even | odd;
}

__device__ __forceinline__ float mix_f32(float lam, float oml, float a, float b) { return __fmaf_rn(lam, a, __fmul_rn(oml, b)); }

// The blended batch, out of place (row b reads row perm[b], which an in-place pass may already have overwritten):
//   Xm[b] = fmaf(lam, X[b], (1 - lam) * X[perm[b]]),   Rm[b] = (k R[b] + (256 - k) R[perm[b]] + 128) >> 8 per byte,
// k read from the device, lam = k / 256 and 1 - lam both exact.  A clip whose partner is itself, and every clip when k == 256,
// is copied: the input bytes, whatever they are (a -0.0, a NaN in a partner the factor gives no weight).  One launch, two
// ranges of workgroups, both pure HBM streams of two reads and one write.  [0, r_blocks): the ROI frames, 16 bytes per lane as the
// u8 gathers move them; the T frames of a clip are one run of T * chunks 16-byte chunks, and a lane takes chunk u of the batch,
// clip u / (T * chunks), whatever the frame size (a 32 x 32 frame is 64 chunks: no lane idles on it).  Behind them: the features, one lane per W consecutive
// elements of a row of D -- W = 4 (16 bytes per lane: D and ld_x multiples of 4, bases 16-byte aligned) or W = 1 (any D and
// ld_x: 83 exists); rows are ld_x floats apart in X and in Xm.  An entry of perm outside [0, B) is never an index: the row is
// copied.
template <int W>
__global__ __launch_bounds__(256) void batch_mixup_kernel(const float* __restrict__ X, int ld_x, int D, float* __restrict__ Xm,
                                                          const uint8_t* __restrict__ R, uint8_t* __restrict__ Rm, int chunks,
                                                          const int32_t* __restrict__ perm, const int32_t* __restrict__ k_dev,
                                                          int B, int T, int r_blocks) {
  static_assert(W == 1 || W == 4, "one element or one 16-byte chunk per lane");
  const int kk = k_dev[0];
  const uint32_t k = (uint32_t)(kk < 0 ? 0 : kk > 256 ? 256 : kk);
  const long rows = (long)B * T;
  if ((int)blockIdx.x < r_blocks) {
    const uint4* src = reinterpret_cast<const uint4*>(R);
    uint4* dst = reinterpret_cast<uint4*>(Rm);
    const long per_clip = (long)T * chunks, total = rows * chunks;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < total; u += (long)r_blocks * 256) {
      const int b = (int)(u / per_clip);  // one division per lane and chunk, as in the gathers
      const int pb = perm[b];
      const uint4 a = src[u];
      uint4 o = a;
      if (!(k == 256u || pb == b || (unsigned)pb >= (unsigned)B)) {
        const uint4 q = src[u + (long)(pb - b) * per_clip];
        o = uint4{mix_bytes4(a.x, q.x, k), mix_bytes4(a.y, q.y, k), mix_bytes4(a.z, q.z, k), mix_bytes4(a.w, q.w, k)};
      }
      dst[u] = o;
    }
    return;
  }
  const float lam = (float)k * 0.00390625f, oml = (float)(256u - k) * 0.00390625f;
  const int units = D / W;  // per row
  const long total = rows * units;
  const long x_blocks = (long)gridDim.x - r_blocks;
  for (long u = ((long)blockIdx.x - r_blocks) * 256 + threadIdx.x; u < total; u += x_blocks * 256) {
    const long r = u / units;  // one division per lane and chunk, as in the gathers
    const int c = (int)(u - r * units) * W;
    const int b = (int)(r / T);
    const int pb = perm[b];
    const bool copy = k == 256u || pb == b || (unsigned)pb >= (unsigned)B;
    const float* xa = X + r * ld_x + c;
    const float* xb = X + (r + (long)((copy ? b : pb) - b) * T) * ld_x + c;
    float* d = Xm + r * ld_x + c;
    if constexpr (W == 4) {
      const float4 a = *reinterpret_cast<const float4*>(xa);
      float4 o = a;
      if (!copy) {
        const float4 p = *reinterpret_cast<const float4*>(xb);
        o = float4{mix_f32(lam, oml, a.x, p.x), mix_f32(lam, oml, a.y, p.y), mix_f32(lam, oml, a.z, p.z),
                   mix_f32(lam, oml, a.w, p.w)};
      }
      *reinterpret_cast<float4*>(d) = o;
    } else {
      const float a = *xa;
      *d = copy ? a : mix_f32(lam, oml, a, *xb);
    }
  }
}

// the launch of the f32 gather shared by its three entry points: one lane per 16-byte chunk of dst, at most 4096 workgroups
template <bool HOST_NOISE, bool SCALE>
int launch_gather_f32(const float* src, int D, const int32_t* frame_map, long rows, const float* noise, const int32_t* noise_map,
                      float noise_std, uint64_t seed, uint64_t noise_first, const float* row_scale, int rows_per_clip, float* dst,
                      ss_stream_t stream) {
  SS_REQUIRE(src && frame_map && dst && D > 0 && rows > 0 && noise_std >= 0.f, SS_ERR_ARG);
  SS_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 3) == 0, SS_ERR_ARG);
  const long chunks = (rows * D + 3) / 4;
  hipLaunchKernelGGL((batch_gather_f32_kernel<HOST_NOISE, SCALE>), dim3(ss_flat_grid(chunks, 4096)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src, D, frame_map, rows, noise, noise_map, noise_std, seed, noise_first,
                     row_scale, rows_per_clip, dst);
  return ss_launch_status();
}

// what ss_batch_plan and ss_batch_plan_aug both refuse
int plan_args_status(const int32_t* indices, int B, const int32_t* x_off, const int32_t* x_len, const int32_t* r_off,
                     const int32_t* r_len, const int64_t* y, int n_clips, int max_t, double noise_prob, double drop_prob,
                     int drop_max, const int32_t* xmap, const int32_t* nmap, const int32_t* rmap, const int64_t* lens,
                     const int64_t* y_out, const int32_t* err_flag) {
  SS_REQUIRE(indices && x_off && x_len && y && xmap && nmap && lens && y_out && err_flag, SS_ERR_ARG);
  SS_REQUIRE(B > 0 && n_clips > 0 && max_t > 0, SS_ERR_ARG);
  SS_REQUIRE((r_off == nullptr) == (r_len == nullptr) && (!r_off || rmap), SS_ERR_ARG);
  SS_REQUIRE(noise_prob >= 0.0 && noise_prob <= 1.0 && drop_prob >= 0.0 && drop_prob <= 1.0, SS_ERR_ARG);
  SS_REQUIRE(drop_max >= 1, SS_ERR_ARG);
  SS_REQUIRE(drop_max <= 2, SS_ERR_UNSUPPORTED);  // the pair draw is written for one or two dropped frames
  return SS_OK;
}

// a probability as the planner compares it with a 32-bit draw: carried in 64 bits so that p = 1 stays "always"
uint64_t prob_threshold(double p) { return (uint64_t)(p * 4294967296.0); }

}  // namespace

extern "C" int ss_epoch_sample(const int32_t* members, int n_members, const int32_t* class_start, int n_classes,
                               uint64_t first, long count, uint64_t seed, int32_t* indices, ss_stream_t stream) {
  SS_REQUIRE(members && class_start && indices && n_members > 0 && n_classes > 0 && count > 0, SS_ERR_ARG);
  SS_REQUIRE((count + 255) / 256 <= 0x7fffffffL, SS_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(epoch_sample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), members, n_members, class_start, n_classes, first, count, seed, indices);
  return ss_launch_status();
}

extern "C" int ss_batch_plan(const int32_t* indices, int B, const int32_t* x_off, const int32_t* x_len, const int32_t* r_off,
                             const int32_t* r_len, const int64_t* y, int n_clips, int max_t, int augment, uint64_t first_row,
                             uint64_t seed, double noise_prob, double drop_prob, int drop_max, int32_t* xmap, int32_t* nmap,
                             int32_t* rmap, int64_t* lens, int64_t* y_out, int32_t* err_flag, ss_stream_t stream) {
  const int status = plan_args_status(indices, B, x_off, x_len, r_off, r_len, y, n_clips, max_t, noise_prob, drop_prob, drop_max,
                                      xmap, nmap, rmap, lens, y_out, err_flag);
  if (status != SS_OK) return status;
  hipLaunchKernelGGL(batch_plan_kernel<false>, dim3((unsigned)B), dim3(SS_WAVE), 0, static_cast<hipStream_t>(stream), indices,
                     x_off, x_len, r_off, r_len, y, n_clips, max_t, augment, first_row, seed, prob_threshold(noise_prob),
                     prob_threshold(drop_prob), drop_max, PlanPolicy{}, xmap, nmap, rmap, lens, y_out, err_flag);
  return ss_launch_status();
}

extern "C" int ss_batch_gather_f32(const float* src, int D, const int32_t* frame_map, long rows, const float* noise,
                                   const int32_t* noise_map, float noise_std, uint64_t seed, float* dst,
                                   ss_stream_t stream) {
  SS_REQUIRE(!noise || noise_map, SS_ERR_ARG);
  if (noise) return launch_gather_f32<true, false>(src, D, frame_map, rows, noise, noise_map, noise_std, seed, 0, nullptr, 1, dst, stream);
  return launch_gather_f32<false, false>(src, D, frame_map, rows, nullptr, noise_map, noise_std, seed, 0, nullptr, 1, dst, stream);
}

extern "C" int ss_batch_gather_f32_at(const float* src, int D, const int32_t* frame_map, long rows, const int32_t* noise_map,
                                      float noise_std, uint64_t seed, uint64_t noise_first, float* dst, ss_stream_t stream) {
  SS_REQUIRE(noise_map, SS_ERR_ARG);
  return launch_gather_f32<false, false>(src, D, frame_map, rows, nullptr, noise_map, noise_std, seed, noise_first, nullptr, 1, dst,
                                         stream);
}

extern "C" int ss_batch_gather_u8(const uint8_t* src, int frame_bytes, const int32_t* frame_map, long rows, uint8_t* dst,
                                  ss_stream_t stream) {
  SS_REQUIRE(src && frame_map && dst && frame_bytes > 0 && rows > 0, SS_ERR_ARG);
  SS_REQUIRE((frame_bytes & 15) == 0, SS_ERR_UNSUPPORTED);
  SS_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0, SS_ERR_ARG);
  long blocks = rows > 8192 ? 8192 : rows;
  hipLaunchKernelGGL(batch_gather_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                     frame_bytes / 16, frame_map, rows, dst);
  return ss_launch_status();
}

extern "C" int ss_batch_plan_aug(const int32_t* indices, int B, const int32_t* x_off, const int32_t* x_len, const int32_t* r_off,
                                 const int32_t* r_len, const int64_t* y, int n_clips, int max_t, int augment, uint64_t first_row,
                                 uint64_t seed, double noise_prob, double drop_prob, int drop_max, double warp_prob, int warp_lo_pm,
                                 int warp_hi_pm, double scale_prob, float scale_lo, float scale_span, double shift_prob,
                                 int shift_max_x, int shift_max_y, int32_t* xmap, int32_t* nmap, int32_t* rmap, int64_t* lens,
                                 int64_t* y_out, float* row_scale, int32_t* row_shift, int32_t* err_flag, ss_stream_t stream) {
  SS_REQUIRE(row_scale && row_shift, SS_ERR_ARG);
  SS_REQUIRE(warp_prob >= 0.0 && warp_prob <= 1.0 && scale_prob >= 0.0 && scale_prob <= 1.0, SS_ERR_ARG);
  SS_REQUIRE(shift_prob >= 0.0 && shift_prob <= 1.0, SS_ERR_ARG);
  SS_REQUIRE(0 < warp_lo_pm && warp_lo_pm <= warp_hi_pm && warp_hi_pm <= 4000, SS_ERR_ARG);
  SS_REQUIRE(scale_lo > 0.f && scale_span >= 0.f, SS_ERR_ARG);  // (a NaN fails both)
  SS_REQUIRE(shift_max_x >= 0 && shift_max_y >= 0 && shift_max_x < (1 << 30) && shift_max_y < (1 << 30), SS_ERR_ARG);
  // (every refusal above is SS_ERR_ARG, so the shared checks may follow: their one SS_ERR_UNSUPPORTED still comes last)
  const int status = plan_args_status(indices, B, x_off, x_len, r_off, r_len, y, n_clips, max_t, noise_prob, drop_prob, drop_max,
                                      xmap, nmap, rmap, lens, y_out, err_flag);
  if (status != SS_OK) return status;
  const PlanPolicy pol{prob_threshold(warp_prob), warp_lo_pm, warp_hi_pm, prob_threshold(scale_prob), scale_lo, scale_span,
                       prob_threshold(shift_prob), shift_max_x, shift_max_y, row_scale, row_shift};
  hipLaunchKernelGGL(batch_plan_kernel<true>, dim3((unsigned)B), dim3(SS_WAVE), 0, static_cast<hipStream_t>(stream), indices,
                     x_off, x_len, r_off, r_len, y, n_clips, max_t, augment, first_row, seed, prob_threshold(noise_prob),
                     prob_threshold(drop_prob), drop_max, pol, xmap, nmap, rmap, lens, y_out, err_flag);
  return ss_launch_status();
}

extern "C" int ss_batch_gather_f32_aug(const float* src, int D, const int32_t* frame_map, long rows, const int32_t* noise_map,
                                       float noise_std, uint64_t seed, uint64_t noise_first, const float* row_scale,
                                       int rows_per_clip, float* dst, ss_stream_t stream) {
  SS_REQUIRE(noise_map && row_scale, SS_ERR_ARG);
  SS_REQUIRE(rows_per_clip > 0 && rows % rows_per_clip == 0, SS_ERR_ARG);
  return launch_gather_f32<false, true>(src, D, frame_map, rows, nullptr, noise_map, noise_std, seed, noise_first, row_scale,
                                        rows_per_clip, dst, stream);
}

extern "C" int ss_batch_gather_u8_shift(const uint8_t* src, int H, int W, const int32_t* frame_map, long rows,
                                        const int32_t* row_shift, int rows_per_clip, int shift_max_x, int shift_max_y,
                                        uint8_t* dst, ss_stream_t stream) {
  SS_REQUIRE(src && frame_map && row_shift && dst && H > 0 && W > 0 && rows > 0, SS_ERR_ARG);
  SS_REQUIRE(rows_per_clip > 0 && rows % rows_per_clip == 0, SS_ERR_ARG);
  SS_REQUIRE(shift_max_x >= 0 && shift_max_y >= 0 && shift_max_x < W && shift_max_y < H, SS_ERR_ARG);
  SS_REQUIRE((long)H * W <= 0x7fffffffL, SS_ERR_UNSUPPORTED);
  SS_REQUIRE(((H * W) & 15) == 0, SS_ERR_UNSUPPORTED);
  SS_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0, SS_ERR_ARG);
  const long blocks = rows > 8192 ? 8192 : rows;
  if ((W & 15) == 0)
    hipLaunchKernelGGL(batch_gather_u8_shift_kernel<true>, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, H, W, frame_map, rows, row_shift, rows_per_clip, dst);
  else
    hipLaunchKernelGGL(batch_gather_u8_shift_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), src, H, W, frame_map, rows, row_shift, rows_per_clip, dst);
  return ss_launch_status();
}

extern "C" int ss_batch_gather_z(const float* feat, int D, const int32_t* xmap, const float* emb, int E, const int32_t* rmap,
                                 const float* emb_fill, long rows, const int32_t* noise_map, float noise_std, uint64_t seed,
                                 uint64_t noise_first, const float* row_scale, int rows_per_clip, float* dst, int ld_dst,
                                 ss_stream_t stream) {
  SS_REQUIRE(feat && xmap && dst && (emb || !rmap) && rows > 0 && noise_std >= 0.f, SS_ERR_ARG);
  SS_REQUIRE(D > 0 && E > 0 && (long)D + E <= 0x7fffffffL && ld_dst >= D + E, SS_ERR_ARG);
  SS_REQUIRE(!row_scale || (rows_per_clip > 0 && rows % rows_per_clip == 0), SS_ERR_ARG);
  const uintptr_t bases = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(emb) |
                          reinterpret_cast<uintptr_t>(emb_fill) | reinterpret_cast<uintptr_t>(dst);
  SS_REQUIRE((bases & 3) == 0 && (reinterpret_cast<uintptr_t>(row_scale) & 3) == 0, SS_ERR_ARG);
  SS_REQUIRE(((reinterpret_cast<uintptr_t>(xmap) | reinterpret_cast<uintptr_t>(rmap) | reinterpret_cast<uintptr_t>(noise_map)) & 3) == 0,
             SS_ERR_ARG);
  // 16 bytes per lane where every chunk of a row is one aligned float4 on both sides; else one element per lane
  const bool wide = ((D | E | ld_dst) & 3) == 0 && (bases & 15) == 0;
  const long lanes = rows * ((D + E) / (wide ? 4 : 1));
  const int blocks = ss_flat_grid(lanes, 4096);
  if (wide)
    hipLaunchKernelGGL(batch_gather_z_kernel<4>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), feat, D,
                       xmap, emb, E, rmap, emb_fill, rows, noise_map, noise_std, seed, noise_first, row_scale,
                       row_scale ? rows_per_clip : 1, dst, ld_dst);
  else
    hipLaunchKernelGGL(batch_gather_z_kernel<1>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), feat, D,
                       xmap, emb, E, rmap, emb_fill, rows, noise_map, noise_std, seed, noise_first, row_scale,
                       row_scale ? rows_per_clip : 1, dst, ld_dst);
  return ss_launch_status();
}

extern "C" int ss_batch_plan_mask(int32_t* xmap, int32_t* nmap, int32_t* rmap, const int64_t* lens, int B, int max_t, int D, int H,
                                  int W, int augment, uint64_t first_row, uint64_t seed, double time_mask_prob, int time_mask_max,
                                  int time_mask_streams, int time_mask_fill, double feat_mask_prob, int feat_mask_max,
                                  double cutout_prob, int cut_max_w, int cut_max_h, int cutout_fill, int32_t* row_mask,
                                  ss_stream_t stream) {
  SS_REQUIRE(xmap && nmap && lens && row_mask && B > 0 && max_t > 0 && D > 0 && H >= 0 && W >= 0, SS_ERR_ARG);
  SS_REQUIRE(time_mask_prob >= 0.0 && time_mask_prob <= 1.0 && feat_mask_prob >= 0.0 && feat_mask_prob <= 1.0, SS_ERR_ARG);
  SS_REQUIRE(cutout_prob >= 0.0 && cutout_prob <= 1.0, SS_ERR_ARG);  // (a NaN fails every one of these)
  SS_REQUIRE(time_mask_max >= 0 && feat_mask_max >= 0 && cut_max_w >= 0 && cut_max_h >= 0, SS_ERR_ARG);
  SS_REQUIRE(time_mask_streams >= 0 && time_mask_streams <= 2 && time_mask_fill >= 0 && time_mask_fill <= 1, SS_ERR_ARG);
  SS_REQUIRE(cutout_fill >= 0 && cutout_fill <= 255, SS_ERR_ARG);
  const bool cut_on = cutout_prob > 0.0 && cut_max_w >= 1 && cut_max_h >= 1;
  SS_REQUIRE(!cut_on || (rmap && H > 0 && W > 0), SS_ERR_ARG);
  const MaskPolicy pol{prob_threshold(time_mask_prob), time_mask_max, time_mask_streams, time_mask_fill,
                       prob_threshold(feat_mask_prob), feat_mask_max, prob_threshold(cutout_prob), cut_max_w, cut_max_h};
  hipLaunchKernelGGL(batch_plan_mask_kernel, dim3((unsigned)B), dim3(SS_WAVE), 0, static_cast<hipStream_t>(stream), xmap, nmap,
                     rmap, lens, max_t, D, H, W, augment, first_row, seed, pol, row_mask);
  return ss_launch_status();
}

extern "C" int ss_batch_mask_apply(float* X, int ld_x, int D, uint8_t* R, int H, int W, const int32_t* rmap,
                                   const int32_t* row_mask, long rows, int rows_per_clip, int fill, ss_stream_t stream) {
  SS_REQUIRE((X || R) && row_mask && rows > 0 && rows_per_clip > 0 && rows % rows_per_clip == 0, SS_ERR_ARG);
  SS_REQUIRE(fill >= 0 && fill <= 255, SS_ERR_ARG);
  SS_REQUIRE(!X || (D > 0 && ld_x >= D && (reinterpret_cast<uintptr_t>(X) & 3) == 0), SS_ERR_ARG);
  SS_REQUIRE(!R || (rmap && H > 0 && W > 0), SS_ERR_ARG);
  SS_REQUIRE(!R || (long)H * W <= 0x7fffffffL, SS_ERR_UNSUPPORTED);
  long blocks = (rows + 3) / 4;
  blocks = blocks > 8192 ? 8192 : blocks;
  hipLaunchKernelGGL(batch_mask_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), X, ld_x, D, R,
                     H, W, rmap, row_mask, rows, rows_per_clip, fill);
  return ss_launch_status();
}

extern "C" int ss_batch_plan_mixup(const int64_t* lens, const int64_t* y, int B, int augment, uint64_t batch_first_row,
                                   uint64_t seed, double mixup_prob, const uint16_t* table, int N, int32_t* perm, int64_t* y_b,
                                   int64_t* lens_m, int32_t* k_out, float* lam_out, ss_stream_t stream) {
  SS_REQUIRE(lens && y && table && perm && y_b && lens_m && k_out && lam_out, SS_ERR_ARG);
  SS_REQUIRE(B >= 1 && B <= MIXUP_MAX_B && N > 0 && (N & (N - 1)) == 0, SS_ERR_ARG);
  SS_REQUIRE(mixup_prob >= 0.0 && mixup_prob <= 1.0, SS_ERR_ARG);  // (a NaN fails it)
  hipLaunchKernelGGL(batch_plan_mixup_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), lens, y, B, augment,
                     batch_first_row, seed, prob_threshold(mixup_prob), table, N, perm, y_b, lens_m, k_out, lam_out);
  return ss_launch_status();
}

extern "C" int ss_batch_mixup(const float* X, int ld_x, int D, float* Xm, const uint8_t* R, uint8_t* Rm, int frame_bytes,
                              const int32_t* perm, const int32_t* k, int B, int T, ss_stream_t stream) {
  SS_REQUIRE((X == nullptr) == (Xm == nullptr) && (R == nullptr) == (Rm == nullptr) && (X || R), SS_ERR_ARG);
  SS_REQUIRE(perm && k && B > 0 && T > 0, SS_ERR_ARG);
  SS_REQUIRE(!X || (D > 0 && ld_x >= D && X != Xm), SS_ERR_ARG);
  SS_REQUIRE(!X || ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Xm)) & 3) == 0, SS_ERR_ARG);
  SS_REQUIRE(!R || (frame_bytes > 0 && R != Rm), SS_ERR_ARG);
  SS_REQUIRE(!R || (frame_bytes & 15) == 0, SS_ERR_UNSUPPORTED);
  SS_REQUIRE(!R || ((reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(Rm)) & 15) == 0, SS_ERR_ARG);
  const long rows = (long)B * T;
  // at most 2048 workgroups per stream: eight of 256 lanes on each of 256 CUs is all the chip holds at once
  const int r_blocks = !R ? 0 : ss_flat_grid(rows * (frame_bytes / 16), 2048);
  const bool wide = X && ((D | ld_x) & 3) == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Xm)) & 15) == 0;
  const int x_blocks = !X ? 0 : ss_flat_grid(rows * (D / (wide ? 4 : 1)), 2048);
  const dim3 grid(r_blocks + x_blocks);
  if (wide)
    hipLaunchKernelGGL(batch_mixup_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), X, ld_x, D, Xm, R, Rm,
                       frame_bytes / 16, perm, k, B, T, r_blocks);
  else
    hipLaunchKernelGGL(batch_mixup_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), X, ld_x, D, Xm, R, Rm,
                       frame_bytes / 16, perm, k, B, T, r_blocks);
  return ss_launch_status();
}
