// Host build of the source arena's allocator (libzl_amd/csrc/zl_arena.h) for the CPU tier -- TEST HARNESS ONLY.
#include "zl_arena.h"

extern "C" {

void *zla_new(uint64_t first_floats) { ZlArena *a = new ZlArena(); a->init((size_t)first_floats); return a; }
void zla_delete(void *a) { delete (ZlArena *)a; }

uint64_t zla_extent_floats(int64_t length, int channels) { return zl_extent_floats(length, channels); }

int zla_take(void *a, uint64_t floats, uint64_t *off)
{
    size_t o = 0;
    const bool ok = ((ZlArena *)a)->take((size_t)floats, &o);
    if (ok) *off = o;
    return ok ? 1 : 0;
}

uint64_t zla_segment_floats(void *a, uint64_t floats, uint64_t max_bytes) { return ((ZlArena *)a)->segment_floats((size_t)floats, max_bytes); }

void zla_add_segment(void *a, uint64_t handle, uint64_t off, uint64_t floats) { ((ZlArena *)a)->add_segment((void *)(uintptr_t)handle, (size_t)off, (size_t)floats); }

// 1: a segment was handed back, out = (handle, offset, floats)
int zla_give(void *a, uint64_t off, uint64_t n, uint64_t *out)
{
    ZlArena::Segment g{nullptr, 0, 0};
    if (!((ZlArena *)a)->give((size_t)off, (size_t)n, &g)) return 0;
    out[0] = (uint64_t)(uintptr_t)g.handle; out[1] = g.off; out[2] = g.floats;
    return 1;
}

// the free list as (offset, floats) pairs; returns the number of entries (out holds `cap` of them)
int zla_free_list(void *a, uint64_t *out, int cap)
{
    const ZlArena &A = *(ZlArena *)a;
    for (size_t i = 0; i < A.free.size() && (int)i < cap; ++i) { out[2 * i] = A.free[i].first; out[2 * i + 1] = A.free[i].second; }
    return (int)A.free.size();
}

// the later segments as (handle, offset, floats) triples
int zla_segments(void *a, uint64_t *out, int cap)
{
    const ZlArena &A = *(ZlArena *)a;
    for (size_t i = 0; i < A.segments.size() && (int)i < cap; ++i) {
        out[3 * i] = (uint64_t)(uintptr_t)A.segments[i].handle; out[3 * i + 1] = A.segments[i].off; out[3 * i + 2] = A.segments[i].floats;
    }
    return (int)A.segments.size();
}

uint64_t zla_arena_floats(void *a) { return ((ZlArena *)a)->arenaFloats; }
uint64_t zla_arena_segment_floats(void *a) { return ((ZlArena *)a)->arenaSegmentFloats; }

}
