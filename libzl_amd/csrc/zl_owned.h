// zl_owned.h -- the owners of the engine's HIP resources: a device buffer, a page-locked host buffer with its device view, a device
// buffer with an optional host twin that only grows, an event, a stream.  Each is move-only, empty after a move, gives back what it
// holds in its destructor and has an explicit reset().  Host-only, nothing of the engine: tests/cpp/owned_check.cpp compiles it against
// a stand-in for the HIP calls below.  hipFree and hipHostFree wait for the device: WHEN an owner may free is its holder's part (ZlQuiesce).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

#pragma GCC visibility push(hidden)
// resources of the process that live: one up at every successful create, one down at every free (zlhip_debug_live_resources)
enum { ZL_LIVE_DEV, ZL_LIVE_HOST, ZL_LIVE_EVENTS, ZL_LIVE_STREAMS, ZL_LIVE_COUNT };
inline std::atomic<int32_t> zl_live[ZL_LIVE_COUNT] = {};
inline void zl_live_add(int kind, int32_t n) { zl_live[kind].fetch_add(n, std::memory_order_relaxed); }

// what makes a struct with swap() and reset() an owner
#define ZL_OWNER(Name)                                                                          \
    Name() = default; ~Name() { reset(); } Name(Name &&o) noexcept { swap(o); }                 \
    Name &operator=(Name &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }

// a create call's result: one up where it succeeded, else the handle stays null
template <typename H> hipError_t zl_made(int kind, hipError_t r, H *handle) { if (r == hipSuccess) zl_live_add(kind, 1); else *handle = nullptr; return r; }
inline void zl_dev_free(void **p) { if (*p) { (void)hipFree(*p); *p = nullptr; zl_live_add(ZL_LIVE_DEV, -1); } }
inline void zl_host_free(void **h) { if (*h) { (void)hipHostFree(*h); *h = nullptr; zl_live_add(ZL_LIVE_HOST, -1); } }

// n elements of T on the device; reads as the pointer
template <typename T> struct ZlDev {
    T *p = nullptr;
    ZL_OWNER(ZlDev)
    operator T *() const { return p; }
    hipError_t alloc(size_t n) { reset(); return zl_made(ZL_LIVE_DEV, hipMalloc((void **)&p, n * sizeof(T)), &p); }   // frees first; a failure leaves it empty
    void reset() { zl_dev_free((void **)&p); }
    void swap(ZlDev &o) { std::swap(p, o.p); }
};

// page-locked host memory mapped into the device (hipHostMalloc's default flags): h on the host, d the same bytes seen from the device,
// cap in elements.  The kernels read commands from it and write results into it in place; nothing is copied
template <typename T> struct ZlMapped {
    T *h = nullptr, *d = nullptr; size_t cap = 0;
    ZL_OWNER(ZlMapped)
    hipError_t alloc(size_t n)                                     // frees first; a failure leaves it empty
    {
        reset();
        hipError_t r = zl_made(ZL_LIVE_HOST, hipHostMalloc((void **)&h, n * sizeof(T)), &h);
        if (r == hipSuccess) r = hipHostGetDevicePointer((void **)&d, h, 0);
        if (r == hipSuccess) cap = n; else reset();
        return r;
    }
    hipError_t grow(size_t need) { return need <= cap ? hipSuccess : alloc(need * 2); }   // by doubling (the buffer must be idle)
    void reset() { zl_host_free((void **)&h); d = nullptr; cap = 0; }
    void swap(ZlMapped &o) { std::swap(h, o.h); std::swap(d, o.d); std::swap(cap, o.cap); }
};

// a call's records and staging on the device, allocated by the first call that needs them and grown only; h: the page-locked host
// twin, where there is one; cap in elements of the holder's choice.  grow: a too small one is freed, then `bytes` allocated for
// new_cap elements; a failure leaves both halves empty
struct GrowBuf {
    void *d = nullptr, *h = nullptr; size_t cap = 0;
    ZL_OWNER(GrowBuf)
    hipError_t grow(size_t need, size_t new_cap, size_t bytes, bool twin)
    {
        if (need <= cap) return hipSuccess;
        reset();
        hipError_t r = twin ? zl_made(ZL_LIVE_HOST, hipHostMalloc(&h, bytes), &h) : hipSuccess;
        if (r == hipSuccess) r = zl_made(ZL_LIVE_DEV, hipMalloc(&d, bytes), &d);
        if (r == hipSuccess) cap = new_cap; else reset();
        return r;
    }
    void reset() { zl_dev_free(&d); zl_host_free(&h); cap = 0; }
    void swap(GrowBuf &o) { std::swap(d, o.d); std::swap(h, o.h); std::swap(cap, o.cap); }
};

// reads as the handle.  flags: 0 a timing event, or hipEventDisableTiming
struct ZlEvent {
    hipEvent_t ev = nullptr;
    ZL_OWNER(ZlEvent)
    operator hipEvent_t() const { return ev; }
    hipError_t create(unsigned flags = 0) { reset(); return zl_made(ZL_LIVE_EVENTS, flags ? hipEventCreateWithFlags(&ev, flags) : hipEventCreate(&ev), &ev); }
    void reset() { if (ev) { (void)hipEventDestroy(ev); ev = nullptr; zl_live_add(ZL_LIVE_EVENTS, -1); } }
    void swap(ZlEvent &o) { std::swap(ev, o.ev); }
};

// reads as the handle.  Non-blocking; with a priority where one is given
struct ZlStream {
    hipStream_t s = nullptr;
    ZL_OWNER(ZlStream)
    operator hipStream_t() const { return s; }
    hipError_t create(const int *prio = nullptr) { reset(); return zl_made(ZL_LIVE_STREAMS, prio ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *prio) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking), &s); }
    void reset() { if (s) { (void)hipStreamDestroy(s); s = nullptr; zl_live_add(ZL_LIVE_STREAMS, -1); } }
    void swap(ZlStream &o) { std::swap(s, o.s); }
};
#undef ZL_OWNER
#pragma GCC visibility pop
