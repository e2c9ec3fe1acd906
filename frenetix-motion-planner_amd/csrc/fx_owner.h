// fx_owner.h -- the owners of everything the host code takes from the HIP runtime: device arrays, pinned host blocks, events,
// the stream.  Move-only; each gives back what it holds in its destructor, so a context, a pass state or a self-test hook frees by
// going out of scope.  The only calls of hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipEventCreate / hipEventDestroy /
// hipStreamCreate* / hipStreamDestroy in the library are here; so is the account of device bytes (fx_device_bytes).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <utility>

#include "fx_policy.h"

extern thread_local char g_err[512];   // (defined in fx_api.hip)

inline int set_err(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return set_err(FX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                             __FILE__, __LINE__);                                           \
    } while (0)

// A device array of n elements of T; it reads as a T *.  `account` is the byte count it keeps (the context's dev_bytes; none: a
// temporary that fx_device_bytes never saw).  An array of n elements counts max(n, 1) * sizeof(T) bytes.
// ensure() is grow-only: it grows to the largest call and never shrinks, and a growing call gives back what the array held before
// it allocates.  Whether the stream is drained before a block that may still be read is freed is the caller's decision.
template <typename T>
class FxDeviceArray {
    T *p = nullptr;
    size_t n = 0;
    int64_t *account = nullptr;
    static int64_t bytes_of(size_t n) { return (int64_t)(std::max<size_t>(n, 1) * sizeof(T)); }

public:
    explicit FxDeviceArray(int64_t *account = nullptr) : account(account) {}
    FxDeviceArray(FxDeviceArray &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)), account(o.account) {}
    FxDeviceArray &operator=(FxDeviceArray &&o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); account = o.account; }
        return *this;
    }
    ~FxDeviceArray() { release(); }
    operator T *() const { return p; }
    T *get() const { return p; }
    size_t size() const { return n; }   // elements asked for; 0 while empty
    void release() {
        if (!p) return;
        (void)hipFree(p);
        if (account) *account -= bytes_of(n);
        p = nullptr; n = 0;
    }
    int alloc(size_t count) {
        release();
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), (size_t)bytes_of(count)));
        n = count;
        if (account) *account += bytes_of(n);
        return FX_OK;
    }
    int ensure(size_t count) { return count <= n ? FX_OK : alloc(count); }
};
using FxDeviceBlock = FxDeviceArray<char>;   // the block of a pass: bytes, laid out by FxBlockLayout (fx_pass.h)

// A pinned host block of n elements of T with the flags it was made with; `dev` is the device address of a mapped block.  Pinned
// memory is no device memory: fx_device_bytes does not count it.
template <typename T>
class FxPinned {
    T *p = nullptr;
    size_t n = 0;

public:
    T *dev = nullptr;
    unsigned flags = 0;
    FxPinned() = default;
    FxPinned(FxPinned &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)), dev(std::exchange(o.dev, nullptr)), flags(o.flags) {}
    FxPinned &operator=(FxPinned &&o) noexcept {
        if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); dev = std::exchange(o.dev, nullptr); flags = o.flags; }
        return *this;
    }
    ~FxPinned() { release(); }
    operator T *() const { return p; }
    T *get() const { return p; }
    size_t size() const { return n; }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr; n = 0;
    }
    int alloc(size_t count, unsigned with_flags) {
        release();
        flags = with_flags;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), flags));
        n = count;
        if (flags & hipHostMallocMapped) HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), p, 0));
        return FX_OK;
    }
    int ensure(size_t count, unsigned with_flags) { return count <= n ? FX_OK : alloc(count, with_flags); }
};

class FxEvent {
    hipEvent_t e = nullptr;

public:
    FxEvent() = default;
    FxEvent(FxEvent &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    FxEvent &operator=(FxEvent &&o) noexcept { std::swap(e, o.e); return *this; }
    ~FxEvent() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create() {
        if (!e) HIP_TRY(hipEventCreate(&e));
        return FX_OK;
    }
};

// The context's stream: its own (destroyed with it) or a caller's (fx_set_stream: left alone)
class FxStream {
    hipStream_t s = nullptr;
    bool own = false;

public:
    FxStream() = default;
    FxStream(const FxStream &) = delete;
    FxStream &operator=(const FxStream &) = delete;
    ~FxStream() { release(); }
    operator hipStream_t() const { return s; }
    void release() {
        if (own && s) (void)hipStreamDestroy(s);
        s = nullptr; own = false;
    }
    // a non-blocking stream of the library's own, with the priority pointed at if there is one
    int create(const int *priority) {
        release();
        if (priority) HIP_TRY(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority));
        else HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        own = true;
        return FX_OK;
    }
    void borrow(hipStream_t callers) {   // an own stream runs out first
        if (own && s) (void)hipStreamSynchronize(s);
        release();
        s = callers;
    }
};
