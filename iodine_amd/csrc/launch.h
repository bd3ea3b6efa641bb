// Host side of every kernel launch that is more than two lines (included by common.h; nothing here is ABI): the max-LDS attribute
// with its per-(kernel, device) cache, the launch itself, the runtime-to-template dispatch (dispatch.h) and the persistent grid
// (xcd_sched.h).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "dispatch.h"
#include "xcd_sched.h"

#pragma GCC visibility push(hidden)
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) belongs to (function, device): `devs` is a bit mask of the devices the function
// is configured on instead of one process-wide flag, so a second device in the same process - tests, one handle per device - gets
// the attribute too.  Idempotent, so a race between two threads is benign.
inline hipError_t iod_set_max_lds(const void* fn, int bytes, std::atomic<unsigned>& devs)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned bit = 1u << (dev & 31);
    if (devs.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) devs.fetch_or(bit, std::memory_order_release);
    return e;
}
// the attribute step alone; the mask lives in the template: one per kernel instantiation by construction.  (A launcher that
// configures more kernels than it launches keeps doing so: a graphed caller relies on the first, eager call having made every
// attribute call before a later one is captured.)
template <auto Kernel>
inline hipError_t iod_configure(int max_lds)
{
    static std::atomic<unsigned> devs{0};
    return iod_set_max_lds((const void*)Kernel, max_lds, devs);
}
// max_lds != 0: configure, then launch; returns the launch's error
template <auto Kernel, class... A>
inline hipError_t iod_launch(hipStream_t st, dim3 grid, dim3 block, size_t lds, int max_lds, A... args)
{
    if (max_lds != 0)
        if (hipError_t e = iod_configure<Kernel>(max_lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}
#pragma GCC visibility pop
