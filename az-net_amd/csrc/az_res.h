// az_res.h -- the owners of everything the library allocates: device memory, pinned host memory, events and streams.
// THE RULE: every allocation and handle is held by one of the move-only types below, whose destructor releases it; a raw
// pointer or handle field anywhere else (az_ctx, az_trainer, Batch, StaticPlan, ...) is a VIEW, and nothing is freed
// through a view.  The owners return hipError_t and keep no error state of their own: a call site that must report a
// failure does so (dalloc, HIPCHK), one that tolerates it ("try": the int7 slab ring, the stage streams, the upload ring)
// just carries on with an empty owner.
// AZ_RES_FAKE_HIP: the including file declares the nine runtime calls used here (and their types and flags) itself (tests/host/az_res_main.cpp).
#pragma once
#ifndef AZ_RES_FAKE_HIP
#include <hip/hip_runtime.h>
#endif
#include <cstddef>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

// how a failed device allocation of `bytes` is named in an error text
inline std::string alloc_what(size_t bytes) { return "hipMalloc(" + std::to_string(bytes) + " B)"; }

// A list of device allocations, each with 256 B of slack behind it (kernels over-read into it); released as a whole, or
// from a mark on (newest first).
struct DevList {
    std::vector<void *> v;
    DevList() = default;
    DevList(DevList &&o) noexcept : v(std::move(o.v)) { o.v.clear(); }
    DevList &operator=(DevList &&o) noexcept { if (this != &o) { release(); v = std::move(o.v); o.v.clear(); } return *this; }
    DevList(const DevList &) = delete;
    DevList &operator=(const DevList &) = delete;
    ~DevList() { release(); }
    template <typename T>
    hipError_t alloc(T **view, size_t elems)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, elems * sizeof(T) + 256);
        if (e != hipSuccess) return e;
        v.push_back(q);
        *view = (T *)q;
        return hipSuccess;
    }
    size_t mark() const { return v.size(); }
    void release(size_t from = 0) { while (v.size() > from) { hipFree(v.back()); v.pop_back(); } }
};

// One buffer with its capacity in bytes and its kind.  reserve(need, want): holds at least `need` bytes afterwards; when it
// has to grow it frees first and allocates `want` (the call site's growth policy; 0: exactly `need`).  A failed reserve
// leaves it empty with capacity 0.
struct Buf {
    enum Kind { DEVICE, PINNED, MAPPED };
    void *p = nullptr;
    size_t cap = 0;
    Kind kind = DEVICE;
    Buf(Kind k = DEVICE) : kind(k) {}
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap), kind(o.kind) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; kind = o.kind; o.p = nullptr; o.cap = 0; } return *this; }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }
    void reset()
    {
        if (p) { if (kind == DEVICE) hipFree(p); else hipHostFree(p); }
        p = nullptr; cap = 0;
    }
    hipError_t reserve(size_t need, size_t want = 0)
    {
        if (p && need <= cap) return hipSuccess;
        reset();
        if (want < need) want = need;
        const hipError_t e = kind == DEVICE ? hipMalloc(&p, want)
                                            : hipHostMalloc(&p, want, kind == MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    template <typename T> T *as() const { return (T *)p; }
};

// Buffers that are grown together: all of them are freed, then allocated at the sizes given; a failure leaves EVERY member
// empty (the call site keeps the group's shared capacity, which it sets to 0 before and to the new value after success).
struct BufSize { Buf *b; size_t bytes; };
inline hipError_t reserve_group(std::initializer_list<BufSize> g)
{
    for (const BufSize &m : g) m.b->reset();
    for (const BufSize &m : g) {
        const hipError_t e = m.b->reserve(m.bytes);
        if (e != hipSuccess) { for (const BufSize &k : g) k.b->reset(); return e; }
    }
    return hipSuccess;
}

// An event / a stream; created at most once (create on a live one is a no-op), flags at the call site.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { reset(); }
    hipError_t create(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    void reset() { if (e) hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { reset(); s = o.s; o.s = nullptr; } return *this; }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { reset(); }
    hipError_t create(unsigned flags) { return s ? hipSuccess : hipStreamCreateWithFlags(&s, flags); }
    hipError_t create(unsigned flags, int priority) { return s ? hipSuccess : hipStreamCreateWithPriority(&s, flags, priority); }
    void reset() { if (s) hipStreamDestroy(s); s = nullptr; }
    operator hipStream_t() const { return s; }
};

// Recycled timing events (profiling): handed out raw, given back by put(); whatever it holds at the end it destroys.
struct EventPool {
    std::vector<hipEvent_t> free_;
    EventPool() = default;
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool() { for (hipEvent_t e : free_) hipEventDestroy(e); }
    bool grab(hipEvent_t *e)
    {
        if (!free_.empty()) { *e = free_.back(); free_.pop_back(); return true; }
        return hipEventCreateWithFlags(e, hipEventDefault) == hipSuccess;
    }
    void put(hipEvent_t e) { if (free_.size() < 4096) free_.push_back(e); else hipEventDestroy(e); }
};
