// owned_check.cpp -- the owners of the engine's HIP resources (libzl_amd/csrc/zl_owned.h) on the host, under AddressSanitizer and UBSan
// (tests/test_owned_cpu.py builds and runs it).  The HIP calls the owners make are stood in for below with malloc / free: every
// resource is a heap block of its own, so a double free, a use after a move or a leak is the sanitizers' to report, and the stand-in
// keeps a live count of its own next to the owners' four, a log of the calls and a "fail the k-th call" switch.
#include <hip/hip_runtime_api.h>

#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "zl_owned.h"

// ---- the stand-in -----------------------------------------------------------------------------------------------------------------
static int g_live = 0;                 // resources the stand-in has handed out and not got back
static long g_calls = 0, g_failAt = -1;   // creating calls so far; the one that fails (counted from 0), -1 = none
static std::string g_log;              // one letter per call: M F (device), H h (host), E e (event), S s (stream)
static int g_lastPriority = 0; static unsigned g_lastFlags = 0;

static bool stub_fails() { return g_calls++ == g_failAt; }
template <typename P> static hipError_t stub_make(P *out, size_t bytes, char tag, hipError_t err)
{
    if (stub_fails()) return err;      // (*out is left as it was, as the runtime leaves it)
    *out = (P)std::malloc(bytes ? bytes : 1);
    ++g_live; g_log += tag;
    return hipSuccess;
}
static hipError_t stub_drop(void *p, char tag)
{
    assert(p);
    std::free(p);
    --g_live; g_log += tag;
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return stub_make(p, bytes, 'M', hipErrorOutOfMemory); }
hipError_t hipFree(void *p) { return stub_drop(p, 'F'); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return stub_make(p, bytes, 'H', hipErrorOutOfMemory); }
hipError_t hipHostFree(void *p) { return stub_drop(p, 'h'); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int)
{
    if (stub_fails()) return hipErrorInvalidValue;
    *dev = host;
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { g_lastFlags = 0; return stub_make(e, 8, 'E', hipErrorOutOfMemory); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { g_lastFlags = flags; return stub_make(e, 8, 'E', hipErrorOutOfMemory); }
hipError_t hipEventDestroy(hipEvent_t e) { return stub_drop(e, 'e'); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags) { g_lastFlags = flags; g_lastPriority = 0; return stub_make(s, 8, 'S', hipErrorOutOfMemory); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int priority) { g_lastFlags = flags; g_lastPriority = priority; return stub_make(s, 8, 'S', hipErrorOutOfMemory); }
hipError_t hipStreamDestroy(hipStream_t s) { return stub_drop(s, 's'); }
}

// ---- the checks -------------------------------------------------------------------------------------------------------------------
#define CHECK(x) do { if (!(x)) { std::printf("owned check FAILED, line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

static int live(int kind) { return zl_live[kind].load(); }
static bool all_zero() { return g_live == 0 && !live(ZL_LIVE_DEV) && !live(ZL_LIVE_HOST) && !live(ZL_LIVE_EVENTS) && !live(ZL_LIVE_STREAMS); }

// construct, move-construct, move-assign onto a full one, self-move-assign, reset, destruct -- `make` fills an owner, `full` says
// whether it holds anything, `kind` is its live count
template <typename O, typename Make, typename Full> static void life(int kind, Make make, Full full)
{
    CHECK(all_zero());
    {
        O a;
        CHECK(!full(a) && g_live == 0);                            // empty: nothing taken
        CHECK(make(a) == hipSuccess && full(a) && g_live == 1 && live(kind) == 1);
        O b(std::move(a));                                         // move-construct: the source is empty, nothing is created or freed
        CHECK(!full(a) && full(b) && g_live == 1 && live(kind) == 1);
        O c;
        CHECK(make(c) == hipSuccess && g_live == 2 && live(kind) == 2);
        c = std::move(b);                                          // move-assign onto a full one: what it held is freed
        CHECK(!full(b) && full(c) && g_live == 1 && live(kind) == 1);
        O &self = c;
        c = std::move(self);                                       // self-move-assign: keeps what it holds
        CHECK(full(c) && g_live == 1 && live(kind) == 1);
        c.reset();
        CHECK(!full(c) && g_live == 0 && live(kind) == 0);
        c.reset();                                                 // (twice: nothing to free)
        a = std::move(c);                                          // empty onto empty
        CHECK(!full(a) && g_live == 0);
        CHECK(make(a) == hipSuccess && g_live == 1);
        g_failAt = g_calls;                                        // a failed create of a full one frees first and leaves it empty
        CHECK(make(a) != hipSuccess && !full(a) && g_live == 0 && live(kind) == 0);
        g_failAt = -1;
        CHECK(make(a) == hipSuccess && g_live == 1);
    }                                                              // destruct: the full one gives back, the empty ones do nothing
    CHECK(all_zero());
}

static void lives()
{
    life<ZlDev<float>>(ZL_LIVE_DEV, [](ZlDev<float> &x) { return x.alloc(10); }, [](ZlDev<float> &x) { return x.p != nullptr && (float *)x == x.p; });
    life<ZlMapped<int>>(ZL_LIVE_HOST, [](ZlMapped<int> &x) { return x.alloc(10); }, [](ZlMapped<int> &x) { CHECK((x.h != nullptr) == (x.d != nullptr) && (x.h != nullptr) == (x.cap == 10)); return x.h != nullptr; });
    life<ZlEvent>(ZL_LIVE_EVENTS, [](ZlEvent &x) { return x.create(); }, [](ZlEvent &x) { return (hipEvent_t)x != nullptr; });
    life<ZlStream>(ZL_LIVE_STREAMS, [](ZlStream &x) { return x.create(); }, [](ZlStream &x) { return (hipStream_t)x != nullptr; });
    life<GrowBuf>(ZL_LIVE_DEV, [](GrowBuf &x) { return x.grow(x.cap + 1, x.cap + 1, 64, false); }, [](GrowBuf &x) { CHECK((x.d != nullptr) == (x.cap != 0) && !x.h); return x.d != nullptr; });
    // creation flags: a timing event or the flags given; non-blocking streams, with the priority where one is given
    ZlEvent e; ZlStream s; const int hi = -3;
    CHECK(e.create() == hipSuccess && g_lastFlags == 0);
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && g_lastFlags == hipEventDisableTiming && g_live == 1);
    CHECK(s.create() == hipSuccess && g_lastFlags == hipStreamNonBlocking && g_lastPriority == 0);
    CHECK(s.create(&hi) == hipSuccess && g_lastFlags == hipStreamNonBlocking && g_lastPriority == -3 && g_live == 2);
}

// the growth rules: mapped host memory frees first, then takes twice the need; a GrowBuf frees first, then takes new_cap; what fits
// makes no call; a failure leaves the buffer empty with capacity 0
static void growth()
{
    CHECK(all_zero());
    {
        ZlMapped<double> m;
        g_log.clear();
        CHECK(m.grow(0) == hipSuccess && g_log.empty() && !m.h);   // nothing needed, nothing taken
        CHECK(m.grow(5) == hipSuccess && m.cap == 10 && m.h && m.d == m.h && g_log == "H");
        m.h[9] = 1.0;                                              // (the last element is there)
        const long calls = g_calls;
        CHECK(m.grow(10) == hipSuccess && m.cap == 10 && g_calls == calls && g_log == "H");   // fits: no call
        CHECK(m.grow(11) == hipSuccess && m.cap == 22 && g_log == "HhH" && g_live == 1);      // free, then allocate
        m.h[21] = 1.0;
        g_failAt = g_calls;                                        // the allocation fails
        CHECK(m.grow(23) == hipErrorOutOfMemory && !m.h && !m.d && m.cap == 0 && g_log == "HhHh" && g_live == 0 && live(ZL_LIVE_HOST) == 0);
        CHECK(m.grow(23) == hipSuccess && m.cap == 46);
        g_failAt = g_calls + 1;                                    // the device view fails: the fresh block goes back
        CHECK(m.grow(47) == hipErrorInvalidValue && !m.h && !m.d && m.cap == 0 && g_live == 0 && live(ZL_LIVE_HOST) == 0);
        g_failAt = -1;
        CHECK(m.grow(1) == hipSuccess && m.cap == 2 && g_live == 1);
    }
    CHECK(all_zero());
    {
        GrowBuf b;
        g_log.clear();
        CHECK(b.grow(3, 8, 8 * 4, true) == hipSuccess && b.cap == 8 && b.d && b.h && g_log == "HM" && g_live == 2);
        ((int *)b.d)[7] = 1; ((int *)b.h)[7] = 1;
        const long calls = g_calls;
        CHECK(b.grow(8, 100, 100 * 4, true) == hipSuccess && b.cap == 8 && g_calls == calls);   // fits: no call
        CHECK(b.grow(9, 20, 20 * 4, true) == hipSuccess && b.cap == 20 && g_log == "HMFhHM" && g_live == 2);   // free both, then allocate
        CHECK(live(ZL_LIVE_DEV) == 1 && live(ZL_LIVE_HOST) == 1);
        g_failAt = g_calls + 1;                                    // the device half fails: the fresh twin goes back
        CHECK(b.grow(21, 40, 40 * 4, true) == hipErrorOutOfMemory && !b.d && !b.h && b.cap == 0 && g_live == 0);
        g_failAt = g_calls;                                        // the twin fails: the device half is not asked for
        g_log.clear();
        CHECK(b.grow(1, 4, 16, true) == hipErrorOutOfMemory && !b.d && !b.h && b.cap == 0 && g_log.empty());
        g_failAt = -1;
        CHECK(b.grow(1, 4, 16, false) == hipSuccess && b.d && !b.h && b.cap == 4 && g_live == 1);   // no twin
        CHECK(b.grow(5, 6, 24, false) == hipSuccess && !b.h && b.cap == 6 && g_live == 1 && live(ZL_LIVE_HOST) == 0);
    }
    CHECK(all_zero());
}

// a dozen mixed allocations the way the engine makes them -- members of a struct, events in a vector, locals moved in when all of them
// exist (rt_start) -- with the k-th creating call failing, for every k: whatever was built goes back
struct Holder {
    ZlStream stream, plan; ZlDev<float> arena; ZlDev<int> table; ZlMapped<float> bus; ZlMapped<int> ops;
    GrowBuf scratch[2]; std::vector<ZlEvent> evs; ZlEvent join;
    ZlMapped<long> mail; ZlStream rt; ZlDev<long> dev;
};
static bool build(Holder &h)
{
    const int hi = -1;
    bool ok = h.stream.create() == hipSuccess;
    ok = ok && h.plan.create(&hi) == hipSuccess;
    ok = ok && h.arena.alloc(1000) == hipSuccess && h.table.alloc(7) == hipSuccess;
    ok = ok && h.bus.alloc(64) == hipSuccess && h.ops.grow(40) == hipSuccess;
    ok = ok && h.scratch[0].grow(5, 8, 64, true) == hipSuccess && h.scratch[1].grow(5, 8, 64, false) == hipSuccess;
    h.evs.resize(3);
    for (ZlEvent &e : h.evs) ok = ok && e.create() == hipSuccess;
    while (ok && h.evs.size() < 6) { ZlEvent e; ok = e.create(hipEventDisableTiming) == hipSuccess; if (ok) h.evs.push_back(std::move(e)); }   // (the vector moves its elements as it grows)
    ok = ok && h.join.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && h.ops.grow(200) == hipSuccess && h.scratch[0].grow(9, 16, 128, true) == hipSuccess;
    if (!ok) return false;
    ZlMapped<long> mail; ZlStream rt; ZlDev<long> dev;             // all or none
    if (mail.alloc(1) != hipSuccess || rt.create() != hipSuccess || dev.alloc(1) != hipSuccess) return false;
    h.rt = std::move(rt); h.dev = std::move(dev); h.mail = std::move(mail);
    return true;
}
static void failures()
{
    CHECK(all_zero());
    const long c0 = g_calls;
    { Holder h; CHECK(build(h) && h.mail.h && h.evs.size() == 6 && g_live == 19 && live(ZL_LIVE_EVENTS) == 7 && live(ZL_LIVE_STREAMS) == 3 && live(ZL_LIVE_DEV) == 5 && live(ZL_LIVE_HOST) == 4); }
    CHECK(all_zero());
    const long n = g_calls - c0;                                   // creating calls of the whole sequence
    CHECK(n >= 24);
    for (long k = 0; k < n; ++k) {
        g_failAt = g_calls + k;
        { Holder h; CHECK(!build(h)); CHECK(!h.mail.h && !h.rt && !h.dev); }
        CHECK(all_zero());
    }
    g_failAt = -1;
    std::printf("%ld failure points\n", n);
}

int main()
{
    lives();
    CHECK(all_zero());
    growth();
    failures();
    std::printf("owned check ok\n");
    return 0;
}
