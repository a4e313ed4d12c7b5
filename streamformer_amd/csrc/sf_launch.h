// How every kernel of the library gets onto a stream (host side only).
//   sf_launch          launch, return hipGetLastError()
//   sf_launch_big_lds  the same for a kernel that may take more dynamic LDS than the 64 KB a kernel gets by default: before an instance's
//                      first launch on a device its hipFuncAttributeMaxDynamicSharedMemorySize is raised to SF_LDS_CAP, the CU's whole LDS,
//                      whatever this launch asks for.  One fixed cap, set once: sizes that grow later (temporal kernels with the cache
//                      length, pooling kernels under SF_POOL_SHARE_CU) never call hipFuncSetAttribute again, e.g. inside a stream capture.
//                      A refused attribute is returned, and tried again at the next launch.
//   sf_device_cus      CU count of the current device
// The dispatch (`switch (a.epi)`, ...) that picks an instance is the only list of instances: whatever it launches is set up here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <utility>
#include "sf_switches.h"

#define SF_LDS_CAP (160 * 1024)                                       // bytes of LDS per CU (gfx950)
#define SF_HOST_LOCAL __attribute__((visibility("hidden"))) inline    // one copy per library, not an exported symbol

// the current device as an index of a 64-entry per-device table, or -1 (unknown or past the table: the caller does its set-up every time)
SF_HOST_LOCAL int sf_device_slot() {
  int d = 0;
  return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) ? d : -1;
}

// Which kernel instances have their attribute on which devices: kernel address -> bit mask of devices, open addressing, entries are
// never removed.  Unsynchronised like the per-site flags it replaces (two threads that meet on a kernel's first launch both set the
// attribute, to the same value); only the claim of an empty entry is one compare-and-swap, so that no two kernels share an entry.
// A full table sets the attribute on every launch.
struct SfBigLdsTable {
  static constexpr unsigned N = 256;
  const void* fn[N] = {};
  uint64_t devices[N] = {};
  uint64_t* find(const void* k) {
    unsigned i = (unsigned)(((uintptr_t)k >> 4) * 0x9E3779B1u) % N;
    for (unsigned probes = 0; probes < N; ++probes, i = (i + 1) % N) {
      const void* cur = __atomic_load_n(&fn[i], __ATOMIC_ACQUIRE);
      if (!cur && __atomic_compare_exchange_n(&fn[i], &cur, k, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) cur = k;
      if (cur == k) return &devices[i];
    }
    return nullptr;
  }
};

template <typename... KArgs, typename... Args>
SF_HOST_LOCAL hipError_t sf_launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args) {
  kernel<<<grid, block, lds, s>>>(std::forward<Args>(args)...);
  return hipGetLastError();
}

template <typename... KArgs, typename... Args>
SF_HOST_LOCAL hipError_t sf_launch_big_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args) {
  static SfBigLdsTable ready;                     // the instances of this kernel signature
  const int d = sf_device_slot();
  uint64_t* devices = d >= 0 ? ready.find(reinterpret_cast<const void*>(kernel)) : nullptr;
  if (!devices || !((*devices >> d) & 1)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SF_LDS_CAP);
    if (e != hipSuccess) return e;
    if (devices) *devices |= (uint64_t)1 << d;
  }
  return sf_launch(kernel, grid, block, lds, s, std::forward<Args>(args)...);
}

// multiProcessorCount of the current device (0: the query failed), or what SF_ASSUME_CUS says: the switch is looked up on every call,
// so sf_reload_switches() takes effect.  Fallback and rounding are the caller's.
SF_HOST_LOCAL int sf_device_cus() {
  if (const char* e = sf_sw(SW_ASSUME_CUS)) return atoi(e);      // experiment: kernels sized for a CU-masked stream
  static int cus[64] = {};
  const int d = sf_device_slot();
  if (d >= 0 && cus[d]) return cus[d];
  int dev = 0;
  hipDeviceProp_t prop;
  const int n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0;
  if (d >= 0) cus[d] = n;
  return n;
}
