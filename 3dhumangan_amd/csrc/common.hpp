// Shared host/device helpers for libh3d (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/h3d.h"

namespace h3d {

void set_error(const char* fmt, ...);

// Drop any stale (sticky) error another library left in the HIP runtime before we launch.
inline void pre_launch() { (void)hipGetLastError(); }

inline int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return H3D_ELAUNCH;
    }
    return H3D_OK;
}

#define H3D_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) {                                 \
            h3d::set_error(__VA_ARGS__);               \
            return H3D_EINVAL;                         \
        }                                              \
    } while (0)

constexpr int kWave = 64;   // CDNA wavefront

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Number of CUs of the current device (cached per device; falls back to the MI355X value).
int compute_units();

// Workgroups per batch item of a persistent grid [this, B]: about `per_cu` workgroups per CU in total walk the `groups` work items
// of every batch item, so that the tables are staged once per many items while the tail of the launch stays short.
inline int64_t persistent_wgs(int64_t groups, int B, int per_cu) {
    const int64_t want = ((int64_t)per_cu * compute_units() + B - 1) / B;
    const int64_t n = groups < want ? groups : want;
    return n < 1 ? 1 : n;
}

// Work counters of a persistent launch (synthesis_x3.hip, field_x3.hip): a workgroup of batch item b starts at index blockIdx.x
// and takes every further index as gridDim.x + atomic_add(counter[b], 1) -- a workgroup on a faster XCD comes back sooner and
// takes more.  Returns int[B] of device memory, zeroed on `st` in front of the launch that follows; nullptr (error set) on failure.
// The blocks come out of one pool per device, allocated at the first call and handed out round robin (a host-side atomic cursor:
// no allocation and no synchronisation per call, any number of host threads and streams).  A block is handed out again when the
// cursor has gone once round the pool: with kWorkCounterPool ints and batches of at most kWorkCounterMaxB that is after at least
// kWorkCounterPool / kWorkCounterMaxB - 1 = 15 later launches of the largest batch the engines accept, after 65 535 later launches
// at the 16 items of the flagship workload -- the depth of launches in flight behind one another, over all streams of a device,
// that the pool covers.
constexpr int kWorkCounterPool = 1 << 20;
constexpr int kWorkCounterMaxB = 65535;
static_assert(kWorkCounterPool / kWorkCounterMaxB - 1 >= 15, "work-counter pool: fewer than 15 launches between two uses of a block");
int* work_counters(int B, hipStream_t st);

// Function attributes are per device: raise the dynamic-LDS limit of `kernel` to the full 160 KB once per
// (expansion site = kernel instantiation, device).  Idempotent, so a race between two host threads is harmless.
#define H3D_ALLOW_MAX_LDS(kernel)                                                                         \
    do {                                                                                                  \
        static unsigned long long done_ = 0;                                                              \
        int dev_ = 0;                                                                                     \
        (void)hipGetDevice(&dev_);                                                                        \
        const unsigned long long bit_ = 1ull << (dev_ & 63);                                              \
        if (!(done_ & bit_)) {                                                                            \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),                              \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);            \
            done_ |= bit_;                                                                                \
        }                                                                                                 \
    } while (0)

}  // namespace h3d
