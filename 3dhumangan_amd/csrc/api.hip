// libh3d: version / error plumbing of the C ABI (include/h3d.h).
#include "common.hpp"
#include <string.h>
#include <atomic>
#include <mutex>

namespace h3d {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int compute_units() {
    static int cached[64] = {0};
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int& c = cached[dev & 63];
    if (c) return c;
    c = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    return c;
}

namespace {
struct WorkCounterPool {
    std::atomic<int*> base{nullptr};
    std::atomic<unsigned> next{0};
    std::mutex alloc;
};
WorkCounterPool g_work_pools[64];
}  // namespace

int* work_counters(int B, hipStream_t st) {
    int dev = 0;
    if (B < 1 || B > kWorkCounterMaxB || hipGetDevice(&dev) != hipSuccess) {
        set_error("work_counters: B=%d", B);
        return nullptr;
    }
    WorkCounterPool& P = g_work_pools[dev & 63];
    int* base = P.base.load(std::memory_order_acquire);
    if (!base) {
        std::lock_guard<std::mutex> lock(P.alloc);
        base = P.base.load(std::memory_order_acquire);
        if (!base) {
            void* p = nullptr;
            if (hipMalloc(&p, sizeof(int) * kWorkCounterPool) != hipSuccess) {
                (void)hipGetLastError();
                set_error("work_counters: cannot allocate the pool");
                return nullptr;
            }
            base = static_cast<int*>(p);
            P.base.store(base, std::memory_order_release);
        }
    }
    // the next B ints (a block never straddles the end of the pool)
    unsigned at = P.next.load(std::memory_order_relaxed), start;
    do {
        start = at + (unsigned)B > (unsigned)kWorkCounterPool ? 0u : at;
    } while (!P.next.compare_exchange_weak(at, start + (unsigned)B, std::memory_order_relaxed));
    if (hipMemsetAsync(base + start, 0, sizeof(int) * (size_t)B, st) != hipSuccess) {
        set_error("work_counters: %s", hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return base + start;
}

}  // namespace h3d

extern "C" int h3d_version(void) { return H3D_VERSION; }

extern "C" const char* h3d_last_error(void) { return h3d::g_err; }

extern "C" int h3d_device_info(int* n_cu, char* name, int name_len) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        h3d::set_error("h3d_device_info: no HIP device");
        return H3D_ELAUNCH;
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (name && name_len > 0) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    return H3D_OK;
}
