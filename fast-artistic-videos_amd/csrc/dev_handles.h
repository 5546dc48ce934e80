// dev_handles.h -- owning handles for device memory, pinned memory, events and queues: std::unique_ptr with one deleter per kind of
// resource.  An object whose members are handles needs no destructor that lists them, and std::swap / std::move work as on any
// unique_ptr.  Needs the HIP runtime only: libfav fills the handles through dev_owned.h (FAV_* codes), the executables through
// host/fav_cli.h (die on failure).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <type_traits>

namespace fav {

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { using pointer = hipEvent_t; void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
// a queue is drained before it goes: what it still holds may read buffers that are freed next
struct QueueDestroy { using pointer = hipStream_t; void operator()(hipStream_t q) const { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); } };

template <class T> using dev_ptr = std::unique_ptr<T, DevFree>;        // hipMalloc
template <class T> using host_ptr = std::unique_ptr<T, HostFree>;      // hipHostMalloc
using event_h = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using queue_h = std::unique_ptr<std::remove_pointer_t<hipStream_t>, QueueDestroy>;

}  // namespace fav
