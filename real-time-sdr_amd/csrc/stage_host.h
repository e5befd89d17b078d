// stage_host.h -- the host side the stage handles of libsdr_amd.so share (not installed, host code only). A stage
// keeps its argument checks, its fail() texts and its kernels; the steps between them are here, once.
#pragma once

#include <initializer_list>
#include <new>

#include "sdr_internal.h"

namespace sdrk SDRK_HIDDEN {

// a create behind its checks: the device, and the handle with its defaults on that device
template <typename H>
inline int create_begin(H** h, int device, const char* what) {
    HIP_TRY(hipSetDevice(device));
    *h = new (std::nothrow) H;
    if (!*h) return fail(SDR_E_NOMEM, "%s: out of memory", what);
    (*h)->device = device;
    return SDR_OK;
}

// one link of a create's chain of allocations: nothing once an earlier link has failed
template <typename T>
inline void dev_alloc(hipError_t& e, T** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc((void**)p, bytes);
}

// workgroups of 256 threads for n items, one thread each (the reset and stats kernels)
inline unsigned groups256(size_t n) { return (unsigned)((n + 255) / 256); }

// the last links of a create's chain: the reset kernel on the null stream, and the wait for it
template <typename... P, typename... A>
inline void create_reset(hipError_t& e, void (*kernel)(P...), unsigned groups, A... args) {
    if (e != hipSuccess) return;
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(256), 0, nullptr, static_cast<P>(args)...);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
}

// the tail of a create: a failed chain destroys what there is of the handle and names the error
template <typename H>
inline int create_done(hipError_t e, H* h, H** out, int (*destroy)(H*), const char* what) {
    if (e != hipSuccess) {
        destroy(h);
        return fail(e == hipErrorOutOfMemory ? SDR_E_NOMEM : SDR_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    *out = h;
    return SDR_OK;
}

// a destroy: the handle's device, idle (a pending call may still use the buffers), its device allocations in
// the order given, the handle
template <typename H>
inline int destroy_handle(H* h, std::initializer_list<void*> dev_ptrs) {
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (void* p : dev_ptrs)
        if (p) (void)hipFree(p);
    delete h;
    return SDR_OK;
}

// a reset or stats kernel, `groups` workgroups of 256 threads, on s of the handle's device
template <typename... P, typename... A>
inline int launch_on(int device, void (*kernel)(P...), unsigned groups, hipStream_t s, A... args) {
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(256), 0, s, static_cast<P>(args)...);
    LAUNCH_CHECK();
    return SDR_OK;
}

// host[0 .. n) = dev[0 .. n) on s of the current device, waited for
template <typename T>
inline int copy_records(const T* dev, T* host, size_t n, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SDR_OK;
}

}  // namespace sdrk
