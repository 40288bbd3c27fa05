// Cross-workgroup exchange of the persistent recurrence kernels (gru_split.h: exact-f32, H <= 192; gru_bf16_pers.h: bf16 MFMA,
// H <= 512): 8-byte {payload, tag} granules, bounded sweeps, the block-to-(group, part) map, XCD discovery, the launch
// generation, fault injection.  See gru_split.h for the protocol.
#pragma once

namespace {

constexpr int SYNC_HDR_WORDS = 64;

// A sync workspace: SYNC_HDR_WORDS header words, then three runs of granules -- the XCD ids, the forward exchange, the backward
// exchange.  Size queries and launchers both take the sections from here, so they cannot disagree.
struct SyncSections {
  long xid_granules, fwd_granules, bwd_granules;
  long bytes() const { return SYNC_HDR_WORDS * 4L + (xid_granules + fwd_granules + bwd_granules) * 8; }
  unsigned* hdr(void* ws) const { return static_cast<unsigned*>(ws); }
  unsigned long long* xid(void* ws) const { return reinterpret_cast<unsigned long long*>(hdr(ws) + SYNC_HDR_WORDS); }
  unsigned long long* fwd(void* ws) const { return xid(ws) + xid_granules; }
  unsigned long long* bwd(void* ws) const { return fwd(ws) + fwd_granules; }
};

// Tag of a granule = (launch generation << 10) + n: n = step + 1 = 1 .. XCHG_MAX_T for the granules of a step, 1023 for the
// XCD ids; never 0, the cleared state.  A launch therefore takes at most XCHG_MAX_T steps.
constexpr int XCHG_MAX_T = 1022;
__device__ __forceinline__ unsigned xchg_tag_base(unsigned gen) { return (gen & 0x3FFFFFu) << 10; }

#define SS_AGENT __HIP_MEMORY_SCOPE_AGENT
#define NAN_F __builtin_nanf("")
typedef unsigned long long u64;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr int AUX_SC1 = 16;  // cache-policy operand of the raw buffer intrinsics: bit 4 = sc1 (agent scope)

__device__ __forceinline__ rsrc_t granule_rsrc(u64* base, long granules) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)(granules * 8), 0x00020000);
}

// Two adjacent granules in ONE 16-byte write-through store (each 8-byte half lands whole; a 16-byte sc1 store costs
// the fabric what an 8-byte one does).  `pair` = index of the granule pair; payloads raw, resp. as floats.
__device__ __forceinline__ void store_pair_raw(rsrc_t rs, int pair, unsigned tag, unsigned p0, unsigned p1, bool same_xcd) {
  const u32x4 d = {p0, tag, p1, tag};
  if (same_xcd) __builtin_amdgcn_raw_buffer_store_b128(d, rs, pair * 16, 0, 0);  // stays in the shared L2 (wave-uniform branch)
  else __builtin_amdgcn_raw_buffer_store_b128(d, rs, pair * 16, 0, AUX_SC1);
}
__device__ __forceinline__ void store_granule_pair(rsrc_t rs, int pair, unsigned tag, float v0, float v1, bool same_xcd) {
  store_pair_raw(rs, pair, tag, __float_as_uint(v0), __float_as_uint(v1), same_xcd);
}

// blockIdx -> (group = slice * 2 + direction, part) of a grid of `groups` x P workgroups.  Part-major when the group count is a
// multiple of 8: workgroups are dealt round-robin over the 8 XCDs, b and b + 8k share one, and so do the P partners of a group
// then (the f32 launch pads the group count to a multiple of 8 where the padded grid still fits -- xchg_grid in gru.hip:
// workgroups of the pad groups leave at once -- so small batches, the reference's own 16 clips among them, get the same-XCD
// exchange too).  Placement is never assumed, see partners_share_xcd.
__device__ __forceinline__ void xchg_ids(int P, int& groups, int& group, int& part) {
  groups = gridDim.x / P;
  const bool part_major = (groups & 7) == 0;
  part = part_major ? blockIdx.x / groups : blockIdx.x % P;
  group = part_major ? blockIdx.x % groups : blockIdx.x / P;
}

// Which XCD this workgroup runs on, and whether all P partners of its pair share it.  xid: [pairs][P] granules in the
// sync header area, tag = generation base + 1023.
__device__ __forceinline__ bool partners_share_xcd(u64* xid, int pair, int part, int P, unsigned base, unsigned* errors, int lane,
                                                   bool* lost) {
  base += 1023u;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 15u;
  u64* mine = xid + (long)pair * P;
  if (threadIdx.x == 0) __hip_atomic_store(mine + part, ((u64)base << 32) | xcc, __ATOMIC_RELAXED, SS_AGENT);
  bool same = true;
  for (int spins = 0;; ++spins) {
    const u64 x = lane < P ? __hip_atomic_load(mine + lane, __ATOMIC_RELAXED, SS_AGENT) : (((u64)base << 32) | xcc);
    const bool ok = (unsigned)(x >> 32) == base;
    if (__all(ok)) {
      same = __all((unsigned)x == xcc);
      break;
    }
    if (spins > (1 << 20)) {
      if (lane == 0) atomicAdd(errors, 1u);
      same = false;
      *lost = true;
      break;
    }
  }
  return same;
}

// Bounded sweep: a thread re-reads its N 16-byte granule pairs (`stride` pairs apart) until every tag matches; payloads raw.
template <int N>
__device__ __forceinline__ bool sweep_pairs(rsrc_t rs, int pair0, int stride, unsigned tag, unsigned (&v)[2 * N], unsigned* errors,
                                            int lane) {
  for (int spins = 0;;) {
    bool ok = true;
    asm volatile("" ::: "memory");  // every pass really loads again
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, (pair0 + stride * k) * 16, 0, AUX_SC1);
      v[2 * k] = x[0];
      v[2 * k + 1] = x[2];
      ok &= x[1] == tag && x[3] == tag;
    }
    if (__all(ok)) return true;
    if (++spins > (1 << 20)) {  // ~1 s of sweeping: a partner is gone
      if (lane == 0) atomicAdd(errors, 1u);
      return false;
    }
  }
}
// the float view of it, pair stride 256: the whole workgroup sweeps a contiguous run
template <int N>
__device__ __forceinline__ bool sweep_granules(rsrc_t rs, int pair0, unsigned tag, float (&v)[2 * N], unsigned* errors, int lane) {
  for (int spins = 0;;) {
    bool ok = true;
    asm volatile("" ::: "memory");  // every pass really loads again
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, (pair0 + 256 * k) * 16, 0, AUX_SC1);
      v[2 * k] = __uint_as_float(x[0]);
      v[2 * k + 1] = __uint_as_float(x[2]);
      ok &= x[1] == tag && x[3] == tag;
    }
    if (__all(ok)) return true;
    if (++spins > (1 << 20)) {  // ~1 s of sweeping: a partner is gone
      if (lane == 0) atomicAdd(errors, 1u);
      return false;
    }
  }
}

// A sweep in two halves: issue the first pass, do something else while its loads fly, then look at the tags (and fall back to
// sweep_pairs when a partner has not published yet)
template <int N>
__device__ __forceinline__ void sweep_issue(rsrc_t rs, int pair0, int stride, u32x4 (&raw)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) raw[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, (pair0 + stride * k) * 16, 0, AUX_SC1);
}
template <int N>
__device__ __forceinline__ bool sweep_check(const u32x4 (&raw)[N], unsigned tag, unsigned (&v)[2 * N]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[2 * k] = raw[k][0];
    v[2 * k + 1] = raw[k][2];
    ok &= raw[k][1] == tag && raw[k][3] == tag;
  }
  return __all(ok);
}

// sync[2] counts bounded waits that gave up (never reset by the kernels: the host reads it where it synchronises anyway, see
// engine.check_gru_sync).  In band, a workgroup that lost a partner emits NaN for everything IT owns from that step on (and
// publishes NaN, so its partners do the same): a poison that needs no ordering against anybody else's stores.  (Rounds 1-2
// wrote the NaN over element 0 of the result, which another workgroup owns: two XCDs then hold dirty copies of one line and the
// order of their write-backs decides -- the test of this channel found the poison lost.)
__device__ __forceinline__ void finish_launch(unsigned* sync, unsigned gen) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned done = atomicAdd(&sync[1], 1u);
    if (done == gridDim.x - 1) {
      __hip_atomic_store(&sync[1], 0u, __ATOMIC_RELAXED, SS_AGENT);
      __hip_atomic_store(&sync[0], gen + 1u, __ATOMIC_RELEASE, SS_AGENT);
    }
  }
}

// Fault injection for the tests of the failure channel (tests/test_gpu_kernels.py::test_gru_lost_partner_reaches_the_host):
// sync[5] = 1 + the index of a workgroup that plays dead -- it publishes nothing and only arrives at the end, so its partners'
// bounded waits run out.  Zero (the cleared state) = off; the owner of the workspace sets it, the kernels never do.
__device__ __forceinline__ bool plays_dead(const unsigned* sync) {
  return __hip_atomic_load(&sync[5], __ATOMIC_RELAXED, SS_AGENT) == blockIdx.x + 1u;
}

// First thing in a kernel: thread 0 requests the launch generation into s_gen (shared).  False = this workgroup takes no part
// (it plays dead, or its group is one of the grid's pad, group >= live_groups: both wave-uniform) and has already arrived at
// the end of the launch.  True: the kernel raises its priority (s_setprio 3: every cycle of the chain is on the step's
// critical path, it issues ahead of the weight-gradient GEMM waves that share the SIMDs), loads its weight fragments, which
// overlap the generation load, passes a barrier and calls xchg_open.
__device__ __forceinline__ bool xchg_begin(unsigned* sync, unsigned& s_gen, int group, int live_groups) {
  if (threadIdx.x == 0) s_gen = __hip_atomic_load(&sync[0], __ATOMIC_RELAXED, SS_AGENT);
  if (plays_dead(sync) || group >= live_groups) {
    __syncthreads();
    finish_launch(sync, s_gen);
    return false;
  }
  return true;
}

// Behind that barrier: the generation, the tag base of this launch, whether the partners share an XCD (counted in sync[3]:
// workgroup-launches on the fast path), and `dead` = a partner never arrived, whatever this workgroup emits is NaN.
__device__ __forceinline__ bool xchg_open(unsigned* sync, const unsigned& s_gen, u64* xid, int group, int part, int P, int lane,
                                          unsigned& gen, unsigned& base, bool& dead) {
  gen = s_gen;
  base = xchg_tag_base(gen);
  dead = false;
  const bool same_xcd = partners_share_xcd(xid, group, part, P, base, &sync[2], lane, &dead);
  if (threadIdx.x == 0 && same_xcd) atomicAdd(&sync[3], 1u);
  return same_xcd;
}

}  // namespace
