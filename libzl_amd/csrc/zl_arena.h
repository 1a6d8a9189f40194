// zl_arena.h -- the allocator of the source arena: which floats of the arena a source gets and which become
// free again, decided on the host without a HIP call.  The engine (zl_engine.cpp: alloc_extent / free_extent) owns the device memory:
// it allocates a segment when this says one is needed and frees the segment this hands back.  A host build for the CPU tier is
// tests/cpu_harness/arena_host.cpp; tests/cpp/arena_check.cpp walks it under a sanitizer with checked iterators.
//
// An ALLOCATION is the first arena (offset 0, arenaFloats floats, kept for the engine's life) or a later segment.  An EXTENT is
// (offset, floats) inside one allocation; offsets count floats from the first arena's base, modulo 2^64.  Clips are loaded and
// destroyed freely (SamplerSynth::registerClip / unregisterClip, SamplerSynth.cpp:285-312): first fit over the free extents, sorted
// by offset; a released extent is coalesced with its free neighbours; a later segment that is wholly free again is handed back.
//
// What the engine guarantees:
//   * every offset and size is a multiple of 4 floats (sources stay 16-byte aligned); sizes are above 0 except in give()
//   * two allocations never abut in offset space: every allocation carries 1024 floats of padding behind it that the allocator does
//     not own, so free extents of different allocations are never coalesced and a free extent lies inside ONE allocation
//   * offsets are compared as unsigned 64-bit numbers: a segment below the first arena in the address space has a "negative"
//     offset, which sorts last; no allocation wraps (offset + floats does not pass 2^64)
//   * give() gets extents that take() handed out (or the two parts such an extent was cut into), each once
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "zl_stretch.h"

static_assert(sizeof(size_t) == 8, "arena offsets are 64-bit");

// floats of the arena extent of a source of `length` frames: ZL_ST_PAD zero frames behind it, 16-byte aligned
inline size_t zl_extent_floats(int64_t length, int channels)
{
    const size_t floats = ((size_t)length + ZL_ST_PAD) * (size_t)channels;
    return (floats + 3) & ~(size_t)3;
}

struct ZlArena {
    typedef std::pair<size_t, size_t> Extent;                      // (offset, floats)
    struct Segment { void *handle; size_t off, floats; };          // handle: the engine's (its device pointer); off: modulo 2^64
    std::vector<Extent> free;                                      // sorted by offset, no empty entry, neighbours coalesced
    std::vector<Segment> segments;                                 // the later segments, in the order they were added
    size_t arenaFloats = 0;                                        // floats of the first arena
    size_t arenaSegmentFloats = 0;                                 // floats in the later segments

    void init(size_t first_floats)
    {
        arenaFloats = first_floats;
        arenaSegmentFloats = 0;
        segments.clear();
        free.assign(1, Extent(0, first_floats & ~(size_t)3));
    }

    // first fit: the free extent of the lowest offset that holds `floats`; false = none does
    bool take(size_t floats, size_t *off)
    {
        for (size_t i = 0; i < free.size(); ++i) {
            if (free[i].second < floats) continue;
            *off = free[i].first;
            free[i].first += floats; free[i].second -= floats;
            if (free[i].second == 0) free.erase(free.begin() + (long)i);
            return true;
        }
        return false;
    }

    // the segment to add when take() found nothing: at least as large as the first arena (and as the source); 0 = it would take the
    // arena over max_bytes (0 = no cap)
    size_t segment_floats(size_t floats, uint64_t max_bytes) const
    {
        const size_t seg = (std::max(floats, arenaFloats) + 3) & ~(size_t)3;
        if (max_bytes > 0 && (arenaFloats + arenaSegmentFloats + seg) * sizeof(float) > max_bytes) return 0;
        return seg;
    }

    // a new segment, wholly free: the take() that follows finds it (nothing else held the source)
    void add_segment(void *handle, size_t off, size_t floats)
    {
        arenaSegmentFloats += floats;
        segments.push_back(Segment{ handle, off, floats });
        const Extent whole(off, floats);
        free.insert(std::lower_bound(free.begin(), free.end(), whole), whole);
    }

    // an extent goes back to the free list, coalesced with its neighbours.  true: a later segment has become wholly free and is no
    // longer the arena's -- *gone is its record, the caller frees its memory (the first arena is never handed back)
    bool give(size_t off, size_t n, Segment *gone)
    {
        if (n == 0) return false;
        auto it = free.insert(std::lower_bound(free.begin(), free.end(), Extent(off, 0)), Extent(off, n));
        if (it + 1 != free.end() && it->first + it->second == (it + 1)->first) { it->second += (it + 1)->second; free.erase(it + 1); }
        if (it != free.begin() && (it - 1)->first + (it - 1)->second == it->first) {
            (it - 1)->second += it->second;
            it = free.erase(it) - 1;                               // (the iterator erase() returns, not one from before it)
        }
        for (size_t si = 0; si < segments.size(); ++si) {
            const Segment seg = segments[si];
            if (!(it->first <= seg.off && seg.off + seg.floats <= it->first + it->second)) continue;
            // (one extent, at most one whole segment: segments are separate allocations; what lies around it stays free)
            const Extent whole = *it;
            it = free.erase(it);
            if (seg.off + seg.floats < whole.first + whole.second)
                it = free.insert(it, Extent(seg.off + seg.floats, whole.first + whole.second - (seg.off + seg.floats)));
            if (whole.first < seg.off) free.insert(it, Extent(whole.first, seg.off - whole.first));
            arenaSegmentFloats -= seg.floats;
            segments.erase(segments.begin() + (long)si);
            *gone = seg;
            return true;
        }
        return false;
    }
};
