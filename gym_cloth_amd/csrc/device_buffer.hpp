// device_buffer.hpp -- the host API's error reporting and the owners of everything it gets from the HIP runtime: device memory, pinned host
// memory, stream, events. Whoever holds one of these as a member or a local needs no free list and no cleanup on its error paths.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>

#include "../../include/clothhip.h"

namespace clothhip {
inline thread_local std::string g_err;      // clothhip_last_error
inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// the ONE mapping from a HIP error to a status: out of memory is CLOTHHIP_ENOMEM whichever call or buffer ran out
inline int hip_status(hipError_t err) { return err == hipErrorOutOfMemory ? CLOTHHIP_ENOMEM : CLOTHHIP_EHIP; }
#define HIPCHECK(expr)                                                                                                                   \
    do {                                                                                                                                 \
        hipError_t err_ = (expr);                                                                                                        \
        if (err_ != hipSuccess)                                                                                                          \
            return clothhip::fail(clothhip::hip_status(err_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err_), __FILE__, __LINE__); \
    } while (0)

// One allocation of device memory (Pinned: of hipHostMalloc memory) with its capacity: move-only, freed by the destructor on the device that
// is current then (~clothhip_handle selects its own first). Empty, it converts to a null pointer. Buffer<void> is a table whose element
// type follows the handle's precision: (T *)buf names it.
template <typename T, bool Pinned = false> class Buffer {
    void *p = nullptr;
    size_t cap = 0;
    void release() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buffer &operator=(Buffer &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buffer() { release(); }
    // at least `bytes` of capacity: nothing if it is there, else free and allocate -- the contents are NOT kept
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        const hipError_t err = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (err != hipSuccess) { p = nullptr; return fail(hip_status(err), "%s(%zu) failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(err)); }
        cap = bytes;
        return 0;
    }
    operator T *() const { return (T *)p; }
    template <typename U> explicit operator U *() const { return (U *)p; }
};
template <typename T> using PinnedBuffer = Buffer<T, true>;

// a stream or an event, destroyed with its owner (&x.v: where hip*Create puts it)
template <typename H, hipError_t (*Destroy)(H)> struct Owned {
    H v = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete; Owned &operator=(const Owned &) = delete;
    ~Owned() { if (v) (void)Destroy(v); }
    operator H() const { return v; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
}  // namespace clothhip
