// lf_dev_ptr.h -- where the O(n) array arguments of an entry point live, and THE pointer check of every _dev entry point of both ABIs (include/lfhip.h
// "device-resident callers", include/lfplus.h "device-resident callers"): shared by lf_ring_host.h (lf_* / bb_*) and lfp_capi.cpp (lfplus_*).
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace lfdev {
// Origin::host (every call without the suffix): pageable host memory.  Origin::device (the _dev twins): the caller's own memory on the context's device, in the
// layout of the host ABI
enum class Origin { host, device };
// [p, p + bytes) lies inside the allocation [base, base + size): the whole range arithmetic of the pointer checks
inline bool range_inside(uintptr_t base, size_t size, uintptr_t p, size_t bytes) { return p >= base && p - base <= size && bytes <= size - (p - base); }
// Before anything is enqueued: device memory of `device`, aligned to `align` bytes (a power of two: 8 for the relayout kernels of lfhip.h, 16 for the vector
// accesses of the LatticeFold+ kernels), `bytes` bytes inside one allocation.  A host or pinned pointer, managed memory, another device's memory, a range that
// runs off its allocation: -1 (LF_ERR_INVALID and LFPLUS_E_ARG are both spelt -1, LF_OK and LFPLUS_OK 0), never a launch
inline int dev_array_check(int device, const void *p, size_t bytes, size_t align = 8) {
    if (!p || ((uintptr_t)p & (align - 1))) return -1;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }   // (older runtimes fail on plain host memory)
    if (at.type != hipMemoryTypeDevice || at.isManaged || at.device != device) return -1;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return range_inside((uintptr_t)base, size, (uintptr_t)p, bytes) ? 0 : -1;
}
}  // namespace lfdev
