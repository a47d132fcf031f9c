// Shared host-side helpers for libsnvc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "snvc_hip.h"

namespace snvc {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

inline int fail(int code, const char *msg) {
    set_error("%s", msg);
    return code;
}

// Set by launch_lds when the attribute call failed (the launch is skipped and the caller's check_launch reports the
// failure, message already recorded by set_error).
inline thread_local bool g_launch_aborted = false;

// Called after every launch: hipGetLastError is a host-side query (no device sync).
inline int check_launch(const char *what) {
    if (g_launch_aborted) {
        g_launch_aborted = false;
        (void)hipGetLastError();
        return SNVC_ERR_HIP;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return SNVC_ERR_HIP;
    }
    return SNVC_OK;
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

namespace detail {
inline std::mutex g_lds_raise_mutex;

// Kernels that need more than 48 KB of dynamic LDS must say so per device (one process may drive several, from several
// host threads: nn.DataParallel replicas).  `granted` holds the bytes last granted on each device, written only after the
// attribute call succeeded; a call that needs more raises the grant under the mutex, so that two threads raising at once
// cannot leave the attribute at the smaller size while the record holds the larger.
inline bool grant_lds(const void *func, int bytes, std::atomic<int> (&granted)[32]) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = 0;
    if (granted[dev].load(std::memory_order_acquire) >= bytes) return true;
    std::lock_guard<std::mutex> lock(g_lds_raise_mutex);
    if (granted[dev].load(std::memory_order_relaxed) >= bytes) return true;
    const hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %d): %s", bytes, hipGetErrorString(e));
        g_launch_aborted = true;
        return false;
    }
    granted[dev].store(bytes, std::memory_order_release);
    return true;
}
}  // namespace detail

// Launches Kernel with `bytes` of dynamic LDS.  The grant record is per kernel (one instantiation each) and per device.
template <auto Kernel, class... Args>
void launch_lds(dim3 grid, dim3 block, size_t bytes, hipStream_t st, const Args &...args) {
    static std::atomic<int> granted[32] = {};
    if (bytes > 48 * 1024 && !detail::grant_lds(reinterpret_cast<const void *>(Kernel), (int)bytes, granted)) return;
    Kernel<<<grid, block, bytes, st>>>(args...);
}

// True when every pointer is a multiple of n bytes (n a power of two; NULL counts as aligned).
template <class... T>
inline bool aligned(uintptr_t n, const T *...ptrs) {
    return ((reinterpret_cast<uintptr_t>(ptrs) | ...) & (n - 1)) == 0;
}

// Compute units of the current device, rounded down to whole XCD octets (persistent-grid sizing).
inline int device_cu_count() {
    static int cached[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
        cached[dev] = n / 8 * 8;
    }
    return cached[dev];
}

template <typename T>
__host__ __device__ inline T ceil_div(T a, T b) { return (a + b - 1) / b; }

constexpr int kWave = 64;  // gfx950 wavefront

}  // namespace snvc
