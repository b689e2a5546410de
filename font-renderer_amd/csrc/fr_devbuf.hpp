// fr_devbuf.hpp — the one owner of device memory in the C ABI units, and the one mapping of a HIP error to the ABI's codes.
#pragma once
#include "../../include/fr_raster.h"
#include "fr_raster_plan.hpp"          // fr::set_error

#include <hip/hip_runtime.h>

// "<what>: <HIP's text>" as FR_E_NOMEM for an allocation that failed, else FR_E_HIP
inline int hip_fail(hipError_t e, const char *what)
{
    return fr::set_error(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

// Device memory of T, freed by the destructor; move-only.  alloc and upload continue a chain of HIP calls: they do nothing
// once `e` holds an error, and leave theirs in it.  Freeing does not wait for the device: whoever owns a DevBuf synchronises
// the streams that use it first (~fr_glyphset, ~fr_plan; the one-shot calls before they return).
template <class T>
class DevBuf {
    T *p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    void reset()
    {
        if (p_) { (void)hipFree(p_); p_ = nullptr; }
    }
    void alloc(hipError_t &e, size_t bytes)
    {
        if (e != hipSuccess) return;
        reset();
        e = hipMalloc(reinterpret_cast<void **>(&p_), bytes);
        if (e != hipSuccess) p_ = nullptr;
    }
    // room for `bytes` and their copy from host memory on `st`; nothing for no bytes
    void upload(hipError_t &e, const void *src, size_t bytes, hipStream_t st)
    {
        if (!bytes) return;
        alloc(e, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(p_, src, bytes, hipMemcpyHostToDevice, st);
    }
    template <class VEC>
    void upload(hipError_t &e, const VEC &v, hipStream_t st)
    {
        upload(e, v.data(), v.size() * sizeof(typename VEC::value_type), st);
    }
};
