// A random walk over the source arena's allocator (libzl_amd/csrc/zl_arena.h) with its invariants as asserts, for a build with
// libstdc++'s checked iterators and the sanitizers (tests/test_arena_cpu.py builds and runs it): an iterator used after erase() or
// insert(), a read past the free list or an overflow ends the program.  The model beside the allocator is a list of the live extents
// and the allocations; what is free follows from them.  The walk is the one of tests/test_arena_cpu.py: a first arena of 4096 floats,
// requests of 4 .. 6000 floats, up to six segments at synthetic offsets -- some of them near 2^64, below the first arena -- 1024 floats
// and more away from each other.
//   arena_check <seed> <steps> <cap bytes, 0 = none>        exit 0 and "arena check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "zl_arena.h"

typedef ZlArena::Extent Extent;
static const size_t FIRST = 4096, GAP = 1024;

struct Model {
    std::vector<Extent> live;
    std::vector<ZlArena::Segment> segs;

    std::vector<Extent> allocations() const
    {
        std::vector<Extent> a(1, Extent(0, FIRST & ~(size_t)3));
        for (const auto &s : segs) a.push_back(Extent(s.off, s.floats));
        std::sort(a.begin(), a.end());
        return a;
    }
    // what the allocations hold besides the live extents: maximal runs, by offset
    std::vector<Extent> gaps() const
    {
        std::vector<Extent> out, l = live;
        std::sort(l.begin(), l.end());
        for (const Extent &a : allocations()) {
            size_t at = a.first;
            for (const Extent &x : l) {
                if (x.first < a.first || x.first >= a.first + a.second) continue;
                assert(x.first >= at && x.first + x.second <= a.first + a.second);     // live extents: disjoint, inside their allocation
                if (x.first > at) out.push_back(Extent(at, x.first - at));
                at = x.first + x.second;
            }
            if (at < a.first + a.second) out.push_back(Extent(at, a.first + a.second - at));
        }
        return out;
    }
    int owner(size_t off) const
    {
        for (size_t i = 0; i < segs.size(); ++i) if (segs[i].off <= off && off < segs[i].off + segs[i].floats) return (int)i;
        return -1;
    }
};

static void check(const ZlArena &a, const Model &m)
{
    size_t freeFloats = 0, liveFloats = 0, segFloats = 0;
    for (size_t i = 0; i < a.free.size(); ++i) {
        assert(a.free[i].second > 0 && a.free[i].first % 4 == 0 && a.free[i].second % 4 == 0);
        assert(a.free[i].first + a.free[i].second > a.free[i].first);                  // nothing wraps
        if (i) assert(a.free[i - 1].first + a.free[i - 1].second <= a.free[i].first);  // sorted, disjoint
        freeFloats += a.free[i].second;
    }
    for (const Extent &x : m.live) { assert(x.first % 4 == 0 && x.second % 4 == 0); liveFloats += x.second; }
    for (const auto &s : m.segs) segFloats += s.floats;
    assert(a.arenaFloats == FIRST && a.arenaSegmentFloats == segFloats && a.segments.size() == m.segs.size());
    assert(freeFloats + liveFloats == (FIRST & ~(size_t)3) + segFloats);
    assert(a.free == m.gaps());                                    // sorted, coalesced inside every allocation, nothing lost
}

// a synthetic offset for a segment, GAP floats and more away from every allocation
static size_t place(std::mt19937_64 &rng, const Model &m, size_t floats)
{
    const std::vector<Extent> allocs = m.allocations();
    for (;;) {
        size_t off;
        switch (rng() % 4) {
        case 0: off = (size_t)0 - floats - GAP - 4 * (size_t)(rng() % 64); break;                       // ends a padding below the arena's base
        case 1: off = (size_t)0 - 4 * ((floats + GAP) / 4 + (size_t)(rng() % 65536)); break;
        case 2: { const Extent &n = allocs[rng() % allocs.size()]; off = n.first + n.second + GAP; break; }   // right behind a neighbour's padding
        default: off = 4 * (size_t)(rng() % 65536); break;
        }
        if (off + floats + GAP - 1 < off) continue;                // it would wrap
        bool ok = true;
        for (const Extent &n : allocs) ok = ok && (off + floats + GAP - 1 < n.first || (n.first + n.second <= off && off - (n.first + n.second) >= GAP));
        if (ok) return off;
    }
}

int main(int argc, char **argv)
{
    const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1, steps = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20000;
    const uint64_t cap = argc > 3 ? strtoull(argv[3], nullptr, 10) : 0;
    std::mt19937_64 rng(seed);
    ZlArena a;
    a.init(FIRST);
    Model m;
    uintptr_t handle = 0x1000;
    unsigned long long grown = 0, returned = 0, refused = 0;
    auto give = [&](size_t i) {
        const Extent x = m.live[i];
        m.live.erase(m.live.begin() + (long)i);
        const int own = m.owner(x.first);
        bool last = own >= 0;
        for (const Extent &y : m.live) if (m.owner(y.first) == own) last = false;
        ZlArena::Segment gone{nullptr, 0, 0};
        const bool got = a.give(x.first, x.second, &gone);
        assert(got == last);                                       // a segment goes exactly when its last extent does, never the first arena
        if (got) {
            assert(gone.handle == m.segs[(size_t)own].handle && gone.off == m.segs[(size_t)own].off && gone.floats == m.segs[(size_t)own].floats);
            m.segs.erase(m.segs.begin() + own);
            ++returned;
        }
        check(a, m);
    };
    check(a, m);
    for (unsigned long long s = 0; s < steps; ++s) {
        if (m.live.size() < 48 && (m.live.empty() || rng() % 100 < 55)) {
            const size_t floats = 4 * (size_t)(1 + rng() % 1500);
            size_t want = (size_t)-1, off = 0;
            for (const Extent &g : m.gaps()) if (g.second >= floats) { want = g.first; break; }
            bool got = a.take(floats, &off);
            assert(got == (want != (size_t)-1) && (!got || off == want));              // first fit
            if (!got) {
                const size_t seg = a.segment_floats(floats, cap);
                const size_t mseg = (std::max(floats, FIRST) + 3) & ~(size_t)3;
                assert(seg == (cap > 0 && (FIRST + a.arenaSegmentFloats + mseg) * 4 > cap ? 0 : mseg));
                if (seg == 0 || m.segs.size() == 6) { ++refused; check(a, m); continue; }
                const size_t at = place(rng, m, seg);
                handle += 16;
                a.add_segment((void *)handle, at, seg);
                m.segs.push_back(ZlArena::Segment{ (void *)handle, at, seg });
                got = a.take(floats, &off);
                assert(got && off == at);
                ++grown;
            }
            m.live.push_back(Extent(off, floats));
            check(a, m);
        } else {
            give((size_t)(rng() % m.live.size()));
        }
    }
    while (!m.live.empty()) give(m.live.size() - 1);
    assert(a.free.size() == 1 && a.free[0] == Extent(0, FIRST & ~(size_t)3) && a.segments.empty() && a.arenaSegmentFloats == 0);
    assert(returned == grown);
    printf("arena check ok: %llu steps, %llu segments added and handed back, %llu requests refused\n", steps, grown, refused);
    return 0;
}
