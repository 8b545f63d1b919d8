// lf_i8_launch.h -- host side of the int8 matrix-core family (the translation units of lf_i8_mma.cuh): one result convention and the large-LDS opt-in.
//
// Every launch_* of the family returns  >= 0: launched (0, or the workgroup count where the caller sizes by it),  I8_ERR_SHAPE: the shape is not handled and
// nothing was launched -- the caller takes its other kernel or answers LF_ERR_UNSUPPORTED --,  I8_ERR_HIP: a HIP call failed -- the caller answers LF_ERR_HIP.
// The statuses of the side calls (attribute, memset, symbol copy) are checked as they are made, hipGetLastError() after the last launch of the call.  A launcher
// that stays `void` (the digit passes launch_i8g_cut_*) is followed by a checked launch on the same stream in the same call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

namespace i8mma {
enum { I8_ERR_SHAPE = -1, I8_ERR_HIP = -2 };
inline int i8_launched() { return hipGetLastError() == hipSuccess ? 0 : I8_ERR_HIP; }   // after the last launch of a call
#define I8_HIPCHK(x) do { if ((x) != hipSuccess) return ::i8mma::I8_ERR_HIP; } while (0)
// The kernels that keep a whole tile set in LDS ask for 160 KB of dynamic shared memory, above the default limit: opt in once per (kernel instantiation, device).
// The attribute belongs to the current device (every entry point has made its context's device current); a context on a second device opts in again.  Lane
// threads may race here: the mask is atomic and setting the attribute twice is harmless.
template <auto KERNEL>
inline hipError_t i8_lds_optin() {
    static std::atomic<uint64_t> done{0};   // bit d: device d has the attribute (devices from 64 on set it at every launch)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t)1 << dev : 0;
    if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
    e = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}
// the opt-in for the current device, then the launch of a kernel that takes one argument struct
template <auto KERNEL, class A>
inline int i8_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &a) {
    I8_HIPCHK(i8_lds_optin<KERNEL>());
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, a);
    return i8_launched();
}
}  // namespace i8mma
