// Host-side launch setup, kept per device: a kernel's dynamic-LDS limit and the device queries that shape a launch.  HIP holds kernel
// attributes and device properties per device, so one process may drive several devices -- in turn, or one per thread -- as long as
// every launcher goes through these helpers; tests/test_launch_setup_cpu.py holds the .hip files to that.  Host code only, and static:
// nothing here is exported from the library or part of its C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <atomic>
#include <mutex>

#define MMEGO_MAX_DEVICES 64

// The current device, or -1 when HIP names none that the per-device tables below can hold.
static inline int mmego_device() {
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MMEGO_MAX_DEVICES ? dev : -1;
}

// Makes the current device's dynamic-LDS limit for Kernel at least `bytes`: 0, or the HIP error (positive; hipErrorInvalidDevice
// without a usable current device).  The limit only grows.  Once it covers `bytes`, a call is one hipGetDevice and one atomic load;
// raising it takes a lock, so that two threads raising at once cannot leave HIP holding the smaller of their two limits.
template <auto Kernel>
static int mmego_allow_lds(size_t bytes) {
  static std::atomic<size_t> limit[MMEGO_MAX_DEVICES];       // per device: the limit set for Kernel (0: none set, HIP's default)
  static std::mutex raising;
  const int dev = mmego_device();
  if (dev < 0) return (int)hipErrorInvalidDevice;
  if (bytes <= limit[dev].load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> hold(raising);
  if (bytes <= limit[dev].load(std::memory_order_relaxed)) return 0;
  const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return (int)e;
  limit[dev].store(bytes, std::memory_order_release);
  return 0;
}

// query(dev) >= 0 of the current device, asked once per device and kept in known[dev] as value + 1 (0: not asked yet; threads that
// race on the first call both ask and agree); 0 without a usable current device.
template <class Query>
static int mmego_per_device(std::atomic<int> (&known)[MMEGO_MAX_DEVICES], Query query) {
  const int dev = mmego_device();
  if (dev < 0) return 0;
  int v = known[dev].load(std::memory_order_relaxed);
  if (v == 0) {
    v = query(dev) + 1;
    known[dev].store(v, std::memory_order_relaxed);
  }
  return v - 1;
}

// The current device's compute units; 0 when HIP cannot say.
static inline int mmego_cu_count() {
  static std::atomic<int> known[MMEGO_MAX_DEVICES];
  return mmego_per_device(known, [](int dev) {
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 0;
  });
}

// Workgroups of Kernel (Block threads, no dynamic LDS) that the current device holds at once: its occupancy per CU x the CU count;
// 0 when HIP cannot say.
template <auto Kernel, int Block>
static int mmego_resident_blocks() {
  static std::atomic<int> known[MMEGO_MAX_DEVICES];
  return mmego_per_device(known, [](int) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, Block, 0) != hipSuccess || per_cu < 0) per_cu = 0;
    return per_cu * mmego_cu_count();
  });
}
