// dev_owned.h -- what fills the owning handles of dev_handles.h on the host side of libfav.  A function that fails half-way just
// returns: the handles it filled free what they hold.
// Every helper returns FAV_OK or FAV_EHIP (hip_fail: the error text names the call, or `what`), so several chain with ||.
#pragma once
#include "dev_handles.h"
#include "fav_internal.h"

namespace fav {

// n elements of T (dev_ptr<void>: n bytes), uninitialised
template <class T> int dev_alloc(dev_ptr<T>& out, size_t n, const char* what = "hipMalloc")
{
    const size_t bytes = n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    void* p = nullptr; const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) return hip_fail(e, what);
    out.reset(static_cast<T*>(p));
    return FAV_OK;
}

// h on the device, zero-padded to pad_to elements.  `out` changes only when everything worked: a failed copy leaves nothing allocated
template <class T> int dev_upload(dev_ptr<T>& out, const std::vector<T>& h, size_t pad_to = 0)
{
    if (pad_to > h.size()) { std::vector<T> padded(h); padded.resize(pad_to); return dev_upload(out, padded); }
    dev_ptr<T> d;
    if (dev_alloc(d, h.size())) return FAV_EHIP;
    if (!h.empty()) FAV_HIP(hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    out = std::move(d);
    return FAV_OK;
}

template <class T> int host_alloc(host_ptr<T>& out, size_t n, unsigned flags)
{
    void* p = nullptr;
    FAV_HIP(hipHostMalloc(&p, n * sizeof(T), flags));
    out.reset(static_cast<T*>(p));
    return FAV_OK;
}

inline int event_create(event_h& out, unsigned flags, const char* what = "hipEventCreateWithFlags")
{
    hipEvent_t e = nullptr; const hipError_t err = hipEventCreateWithFlags(&e, flags);
    if (err != hipSuccess) return hip_fail(err, what);
    out.reset(e);
    return FAV_OK;
}

// a non-blocking queue (no implicit ordering with the null stream)
inline int queue_create(queue_h& out, const char* what = "hipStreamCreateWithFlags")
{
    hipStream_t q = nullptr; const hipError_t err = hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
    if (err != hipSuccess) return hip_fail(err, what);
    out.reset(q);
    return FAV_OK;
}

}  // namespace fav
