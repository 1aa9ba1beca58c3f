// Host side of a kernel launch, shared by every launch_* of the library (no device code): the runtime `dim` and flags of a
// system become template arguments through with_dim / with_flag, and launch<Kern> raises the kernel's dynamic-LDS limit
// where the request needs it, enqueues, and reports the first error.
//
//     return with_dim(P.dim, [&](auto D) { return launch<k_foo<D()>>(dim3(grid), dim3(block), lds, st, P, ...); });
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

namespace pigs {

constexpr int kLaunchMaxDev = 64;
constexpr size_t kLdsNoGrant = 64 * 1024;        // dynamic LDS a kernel may ask for without a grant

// f(std::integral_constant<int, dim>) for dim = 1, 2, and 3 for everything else; returns what f returns
template <class F>
inline auto with_dim(int dim, F &&f)
{
    if (dim == 1) return f(std::integral_constant<int, 1>{});
    if (dim == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

// f(std::true_type) or f(std::false_type)
template <class F>
inline auto with_flag(bool flag, F &&f)
{
    if (flag) return f(std::true_type{});
    return f(std::false_type{});
}

// CUs of the current device, asked once per device; 256 where the runtime does not say, and, without asking, for a
// device id beyond the table
inline int device_cus()
{
    static std::atomic<int> cus[kLaunchMaxDev];                 // zero-initialised
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLaunchMaxDev) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t pr;
        n = hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// raise a kernel's dynamic-LDS limit once per (kernel, device) -- and again only for a larger request -- instead of on
// every launch: setting the attribute is a host call on the enqueue path of every step
template <auto Kern>
inline hipError_t grant_lds(size_t bytes)
{
    if (bytes <= kLdsNoGrant) return hipSuccess;
    static std::atomic<size_t> granted[kLaunchMaxDev];          // one table per kernel instantiation, zero-initialised
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLaunchMaxDev) dev = -1;
    if (dev >= 0 && bytes <= granted[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev >= 0) {
        size_t g = granted[dev].load(std::memory_order_relaxed);
        while (g < bytes && !granted[dev].compare_exchange_weak(g, bytes, std::memory_order_release)) {}
    }
    return e;
}

// grant, enqueue, and the first error of the two: a refused grant launches nothing
template <auto Kern, class... Args>
inline hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args)
{
    const hipError_t e = grant_lds<Kern>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, grid, block, lds, st, args...);
    return hipGetLastError();
}

} // namespace pigs
