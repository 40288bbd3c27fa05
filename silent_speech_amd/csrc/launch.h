// Host-side launch state, kept per device: the CU count, which kernels have had their dynamic-LDS limit raised, and the grid of a
// persistent kernel; and the GEMM launchers' alignment test and layout dispatch.  Host only -- nothing here reaches device code.
// One definition for the whole library: the functions are C++17 inline, so their local state is shared by every translation unit;
// hidden, so they add nothing to the exported C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/ss_hotpath.h"

#define SS_HOST_INLINE __attribute__((visibility("hidden"))) inline

constexpr int SS_MAX_DEVICES = 64;   // a device index past the table still works: it is asked again on every call
constexpr int SS_LDS_KERNELS = 128;  // kernels x template instances that ask for more than 64 KB; past it: set on every launch

// Written idempotently with relaxed atomics, no lock: two host threads racing to fill an entry both store the same value, and a lost
// slot in `raised` only means that kernel's attribute is set once more.
struct ss_device_state {
  std::atomic<int> cus{0};
  std::atomic<const void*> raised[SS_LDS_KERNELS] = {};
};

SS_HOST_INLINE ss_device_state* ss_current_device_state(int* dev) {
  static ss_device_state table[SS_MAX_DEVICES];
  if (hipGetDevice(dev) != hipSuccess) *dev = -1;
  return *dev >= 0 && *dev < SS_MAX_DEVICES ? &table[*dev] : nullptr;
}

// Compute units of the current device (MI355X: 256).  Every persistent grid, co-residency bound and workspace layout that depends
// on the chip's size asks here -- no launcher hard-codes 256.
SS_HOST_INLINE int ss_device_cus() {
  int dev = -1;
  ss_device_state* st = ss_current_device_state(&dev);
  int n = st ? st->cus.load(std::memory_order_relaxed) : 0;
  if (n > 0) return n;
  hipDeviceProp_t prop;
  if (dev >= 0 && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
  if (n <= 0) return 256;  // (no device: the size queries a CPU test makes answer for the target chip)
  if (st) st->cus.store(n, std::memory_order_relaxed);
  return n;
}

// Raise the kernel's dynamic-LDS limit to `bytes` (a launch gets 64 KB by default), once per (device, kernel).  `bytes` must be
// the same on every call for a kernel (each caller passes a compile-time constant of the instance): later values are not looked at.
SS_HOST_INLINE int ss_dynamic_lds(const void* kernel, int bytes) {
  int dev = -1;
  ss_device_state* st = ss_current_device_state(&dev);
  int slot = 0;
  for (; st && slot < SS_LDS_KERNELS; ++slot) {
    const void* k = st->raised[slot].load(std::memory_order_relaxed);
    if (k == kernel) return SS_OK;
    if (!k) break;
  }
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return SS_ERR_LAUNCH;
  if (st && slot < SS_LDS_KERNELS) st->raised[slot].store(kernel, std::memory_order_relaxed);
  return SS_OK;
}

// Test hook (ss_roi_cnn_set_max_workgroups, roi_cnn.hip): CUs a persistent kernel may count on, 0 = all of the device's.  A small
// cap makes a test walk many frames per workgroup.
inline int ss_cnn_max_wgs = 0;

// Workgroups of a persistent kernel that walks `items` (frames), `per_cu` of them resident on a CU.
SS_HOST_INLINE int ss_persistent_grid(int items, int per_cu = 1) {
  const int cap = per_cu * (ss_cnn_max_wgs > 0 ? ss_cnn_max_wgs : ss_device_cus());
  return items < cap ? items : cap;
}

SS_HOST_INLINE bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// f(a, b) with the two layout flags of a GEMM as compile-time constants: launch(K<decltype(a)::value, decltype(b)::value>)
template <class F>
SS_HOST_INLINE void by_layout(bool a_kcontig, bool b_kcontig, F&& f) {
  using T = std::true_type;
  using N = std::false_type;
  if (a_kcontig && b_kcontig) f(T{}, T{});
  else if (a_kcontig && !b_kcontig) f(T{}, N{});
  else if (!a_kcontig && b_kcontig) f(N{}, T{});
  else f(N{}, N{});
}

#undef SS_HOST_INLINE
