// Host side of a kernel launch, shared by the kernels_*.hip units: the current device, and the "first launch of this kernel
// instantiation on this device" step that every persistent launcher opens with.
#pragma once
#include <algorithm>
#include <atomic>

#include "fav_internal.h"

namespace fav {

// Launch-time facts that are cached per kernel instantiation are kept PER DEVICE (function attributes and CU counts belong to
// the device that is current at the launch): a single process may drive several GPUs.
constexpr int MAX_DEVICES = 64;
inline int cur_dev() { int d = 0; (void)hipGetDevice(&d); return (d >= 0 && d < MAX_DEVICES) ? d : 0; }

// One cached int per device, 0 = not set yet.  A launcher keeps one as a function-local static: one per call site and, in a launcher
// template, per instantiation (the LDS limit is a property of each kernel instantiation).  Relaxed atomics and no lock: two threads
// that race on a first launch both do the idempotent setup and store the same value.
struct PerDevice {
    std::atomic<int> v[MAX_DEVICES];
    int get(int dv) const { return v[dv].load(std::memory_order_relaxed); }
    void set(int dv, int x) { v[dv].store(x, std::memory_order_relaxed); }
};

// First launch on device dv: every kernel given may use the CU's whole 160 KB of LDS; *cus = the device's CU count.
template <class... K>
inline hipError_t first_launch_setup(int dv, int* cus, K... kernels)
{
    hipError_t e = hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...})
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dv);      // (hipGetDeviceProperties costs a millisecond or two per call)
    return e;
}

// The whole prologue of a persistent launcher: *cus = the current device's CU count, from the call site's cache after the first launch.
// (A launcher that also asks the runtime about occupancy spells the three steps out and puts its query between setup and set.)
template <class... K>
inline hipError_t launch_cus(PerDevice& cache, int* cus, K... kernels)
{
    const int dv = cur_dev();
    if ((*cus = cache.get(dv)) != 0) return hipSuccess;
    const hipError_t e = first_launch_setup(dv, cus, kernels...);
    if (e == hipSuccess) cache.set(dv, *cus);
    return e;
}

// blocks of a persistent grid: one per CU, less the CUs left to concurrent side-queue work
inline int persistent_slots(int cus, int reserve_cus) { return std::max(1, cus - reserve_cus); }

}  // namespace fav
