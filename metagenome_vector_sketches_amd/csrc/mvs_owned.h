// mvs_owned.h -- the four owners of runtime resources in the C ABI's objects: device memory, pinned host memory, an event, a
// stream.  Each is move-only, empty until asked to create, and releases in reset() and in its destructor; a member of one of
// these types needs no line in any destroy function or failure path.  Not installed.
#ifndef MVS_OWNED_H
#define MVS_OWNED_H

#include <algorithm>
#include <cstddef>
#include <utility>

#ifndef MVS_OWNED_NO_RUNTIME   // the self-test (host/mvs_owned_selftest.cpp) supplies counting stand-ins for the runtime's calls
#include <hip/hip_runtime.h>
#endif

namespace mvs_capi {

// device memory with its size: staging of a call, a handle's state, a context's grow-only buffer (ensure_buf)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) reset(), p = std::exchange(o.p, nullptr), bytes = std::exchange(o.bytes, 0);
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr, bytes = 0;
    }
    // a new block of max(n, 1) bytes (what was held is freed first); empty when the runtime refuses
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p, n ? n : 1);
        if (e == hipSuccess) bytes = n ? n : 1;
        else p = nullptr;
        return e;
    }
    // what a grow-only buffer asks for when n bytes are wanted: head room, so that small changes do not regrow it
    static size_t grown(size_t n) { return n + std::min<size_t>(n / 4, (size_t)256 << 20) + 4096; }
    // grow-only: nothing when n bytes are held, else the block is freed and grown(n) bytes are asked for.  The caller has
    // waited for the work that still uses the block.
    hipError_t grow(size_t n) { return bytes >= n ? hipSuccess : alloc(grown(n)); }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

// pinned host memory with its size; every user has its own growth rule
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) reset(), p = std::exchange(o.p, nullptr), bytes = std::exchange(o.bytes, 0);
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = nullptr, bytes = 0;
    }
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipHostMalloc(&p, n, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) reset(), e = std::exchange(o.e, nullptr);
        return *this;
    }
    ~Event() { reset(); }
    void reset() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess) e = nullptr;
        return rc;
    }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) reset(), s = std::exchange(o.s, nullptr);
        return *this;
    }
    ~Stream() { reset(); }
    void reset() {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
        if (rc != hipSuccess) s = nullptr;
        return rc;
    }
    operator hipStream_t() const { return s; }
};

}  // namespace mvs_capi

#endif
