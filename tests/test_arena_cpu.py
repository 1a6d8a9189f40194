"""The source arena's allocator (libzl_amd/csrc/zl_arena.h), CPU tier: first fit over the free extents, coalescing on release, further
segments addressed by an offset modulo 2^64, a wholly free segment handed back -- built for the host (tests/cpu_harness/arena_host.cpp) and
walked next to a model written independently here: a plain list of the live extents and the set of allocations, no free list.  The free
extents the model expects are what the allocations hold besides the live extents.  tests/cpp/arena_check.cpp repeats the walk under
AddressSanitizer with checked iterators; tests/test_engine_lifecycle.py holds the engine around it on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libzl_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1 << 64
GAP = 1024                         # floats behind every allocation that the allocator does not own
FIRST = 4096

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_arena_harness())
        u64, p64 = C.c_uint64, C.POINTER(C.c_uint64)
        l.zla_new.restype = C.c_void_p; l.zla_new.argtypes = [u64]
        l.zla_delete.restype = None; l.zla_delete.argtypes = [C.c_void_p]
        l.zla_extent_floats.restype = u64; l.zla_extent_floats.argtypes = [C.c_int64, C.c_int]
        l.zla_take.restype = C.c_int; l.zla_take.argtypes = [C.c_void_p, u64, p64]
        l.zla_segment_floats.restype = u64; l.zla_segment_floats.argtypes = [C.c_void_p, u64, u64]
        l.zla_add_segment.restype = None; l.zla_add_segment.argtypes = [C.c_void_p, u64, u64, u64]
        l.zla_give.restype = C.c_int; l.zla_give.argtypes = [C.c_void_p, u64, u64, p64]
        l.zla_free_list.restype = C.c_int; l.zla_free_list.argtypes = [C.c_void_p, p64, C.c_int]
        l.zla_segments.restype = C.c_int; l.zla_segments.argtypes = [C.c_void_p, p64, C.c_int]
        l.zla_arena_floats.restype = u64; l.zla_arena_floats.argtypes = [C.c_void_p]
        l.zla_arena_segment_floats.restype = u64; l.zla_arena_segment_floats.argtypes = [C.c_void_p]
        _lib = l
    return _lib


class Arena:
    """the allocator under test"""
    def __init__(self, first):
        self.a = lib().zla_new(first)

    def close(self):
        lib().zla_delete(self.a)

    def take(self, floats):
        off = C.c_uint64(0)
        return off.value if lib().zla_take(self.a, floats, C.byref(off)) else None

    def segment_floats(self, floats, cap):
        return lib().zla_segment_floats(self.a, floats, cap)

    def add_segment(self, handle, off, floats):
        lib().zla_add_segment(self.a, handle, off, floats)

    def give(self, off, n):
        out = (C.c_uint64 * 3)()
        return tuple(out) if lib().zla_give(self.a, off, n, out) else None

    def free_list(self):
        buf = (C.c_uint64 * 512)()
        n = lib().zla_free_list(self.a, buf, 256)
        assert n <= 256
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    def segments(self):
        buf = (C.c_uint64 * 96)()
        n = lib().zla_segments(self.a, buf, 32)
        assert n <= 32
        return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]

    def floats(self):
        return lib().zla_arena_floats(self.a), lib().zla_arena_segment_floats(self.a)


class Model:
    """live extents and allocations; what is free follows from them"""
    def __init__(self, first):
        self.first = first
        self.live = []                                             # (off, n)
        self.segs = {}                                             # handle -> (off, floats)

    def allocations(self):
        return sorted([(0, self.first & ~3)] + list(self.segs.values()))

    def gaps(self):
        """what the allocations hold besides the live extents: maximal runs, by offset (unsigned)"""
        out = []
        for a0, an in self.allocations():
            at = a0
            for off, n in sorted(x for x in self.live if a0 <= x[0] < a0 + an):
                if off > at:
                    out.append((at, off - at))
                at = off + n
            if at < a0 + an:
                out.append((at, a0 + an - at))
        return out

    def first_fit(self, floats):
        return next((off for off, n in self.gaps() if n >= floats), None)

    def segment_floats(self, floats, cap):
        seg = (max(floats, self.first) + 3) & ~3
        total = self.first + sum(n for _, n in self.segs.values())
        return 0 if cap > 0 and (total + seg) * 4 > cap else seg

    def owner(self, off):
        return next((h for h, (s0, sn) in self.segs.items() if s0 <= off < s0 + sn), None)

    def give(self, off, n):
        """-> the (handle, off, floats) of the segment whose last live extent this was, else None"""
        self.live.remove((off, n))
        h = self.owner(off)
        if h is None or any(self.owner(o) == h for o, _ in self.live):
            return None
        s0, sn = self.segs.pop(h)
        return (h, s0, sn)


def check(ar, mo):
    free, live, allocs = ar.free_list(), sorted(mo.live), mo.allocations()
    inside = lambda off, n: any(a0 <= off and off + n <= a0 + an for a0, an in allocs)
    assert all(off % 4 == 0 and n % 4 == 0 and n > 0 for off, n in free + live)
    assert all(off + n < M for off, n in free + live)                                   # nothing wraps
    assert all(inside(off, n) for off, n in free + live)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(live, live[1:]))                     # live extents are pairwise disjoint
    assert free == sorted(free)
    for a, b in zip(free, free[1:]):                                                    # disjoint; abutting only across two allocations
        assert a[0] + a[1] <= b[0]
        assert a[0] + a[1] < b[0] or not any(a0 <= a[0] and b[0] + b[1] <= a0 + an for a0, an in allocs)
    first, segf = ar.floats()
    assert first == mo.first and segf == sum(n for _, n in mo.segs.values())
    assert sum(n for _, n in free) + sum(n for _, n in live) == (first & ~3) + segf
    assert sorted((h, o, n) for h, (o, n) in mo.segs.items()) == sorted(ar.segments())
    assert free == mo.gaps()                                                            # all of the above at once, and that nothing is lost


def place_segment(rng, mo, floats):
    """a synthetic offset for a new segment, GAP floats and more away from every allocation: half of them below the first arena
    (offsets near 2^64), some as close to a neighbour as the padding allows"""
    allocs = mo.allocations()
    for _ in range(1000):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            off = M - floats - GAP - 4 * int(rng.integers(0, 64))                      # ends a padding below the arena's base
        elif kind == 1:
            off = M - 4 * int(rng.integers((floats + GAP) // 4, 1 << 16))
        elif kind == 2:
            a0, an = allocs[int(rng.integers(0, len(allocs)))]
            off = (a0 + an + GAP) % M                                                   # right behind a neighbour's padding
        else:
            off = 4 * int(rng.integers(0, 1 << 16))
        if off + floats + GAP > M:
            continue
        if all(off + floats + GAP <= a0 or a0 + an + GAP <= off for a0, an in allocs):
            return off
    raise AssertionError("no place for a segment")


def walk(seed, steps, cap):
    rng = np.random.default_rng(seed)
    ar, mo = Arena(FIRST), Model(FIRST)
    handle = 0x1000
    grown = returned = refused = 0
    try:
        check(ar, mo)
        for _ in range(steps):
            if len(mo.live) < 48 and (not mo.live or rng.random() < 0.55):
                floats = 4 * int(rng.integers(1, 1501))                                 # 4 .. 6000: some larger than the first arena
                want = mo.first_fit(floats)
                got = ar.take(floats)
                assert got == want, (floats, got, want)                                # first fit: the lowest free extent that holds it
                if got is None:
                    seg = ar.segment_floats(floats, cap)
                    assert seg == mo.segment_floats(floats, cap)
                    if seg == 0 or len(mo.segs) == 6:
                        refused += 1
                        check(ar, mo)
                        continue
                    handle += 16
                    off = place_segment(rng, mo, seg)
                    ar.add_segment(handle, off, seg)
                    mo.segs[handle] = (off, seg)
                    got = ar.take(floats)
                    assert got == off
                    grown += 1
                mo.live.append((got, floats))
            else:
                off, n = mo.live[int(rng.integers(0, len(mo.live)))]
                want = mo.give(off, n)
                assert ar.give(off, n) == want                                         # a segment goes exactly when its last extent does
                returned += want is not None
            check(ar, mo)
        for off, n in list(mo.live):
            want = mo.give(off, n)
            assert ar.give(off, n) == want
            returned += want is not None
            check(ar, mo)
        assert ar.free_list() == [(0, FIRST & ~3)] and ar.segments() == [] and ar.floats() == (FIRST, 0)
    finally:
        ar.close()
    return grown, returned, refused


def test_random_walk_against_the_model():
    grown, returned, refused = walk(1, 20000, 0)
    assert grown > 100 and returned == grown and refused > 0       # (refused: six segments were live)


def test_random_walk_under_a_cap():
    grown, returned, refused = walk(2, 20000, 4 * (FIRST + 3 * 6000))
    assert grown > 100 and returned == grown and refused > 100


def test_extent_floats():
    f = lib().zla_extent_floats
    assert f(1, 1) == 12 and f(1, 2) == 20 and f(4, 1) == 12 and f(5, 1) == 16 and f(100, 2) == 216 and f(101, 2) == 220
    assert f((1 << 31) - 1, 2) == (((1 << 31) + 7) * 2 + 3) & ~3


def test_first_arena_is_cut_to_a_multiple_of_four():
    ar = Arena(4099)
    assert ar.free_list() == [(0, 4096)] and ar.floats() == (4099, 0)
    ar.close()


def test_exact_fit_erases_the_entry():
    ar = Arena(64)
    assert ar.take(16) == 0 and ar.free_list() == [(16, 48)]
    assert ar.take(48) == 16 and ar.free_list() == []
    assert ar.take(4) is None
    ar.close()


@pytest.mark.parametrize("order,lists", [
    ("ab", [[(0, 16)], [(0, 32)]]),                                # b merges to the left only
    ("cb", [[(32, 16)], [(16, 32)]]),                              # b merges to the right only
    ("acb", [[(0, 16)], [(0, 16), (32, 16)], [(0, 48)]]),          # b merges on both sides
])
def test_release_merges(order, lists):
    ar = Arena(48)
    ext = {"a": ar.take(16), "b": ar.take(16), "c": ar.take(16)}
    assert ext == {"a": 0, "b": 16, "c": 32} and ar.free_list() == []
    for name, want in zip(order, lists):
        assert ar.give(ext[name], 16) is None
        assert ar.free_list() == want
    ar.close()


def test_release_into_a_region_holding_a_whole_segment_with_head_and_tail():
    """Three segments that abut in offset space (which the engine's padding rules out; here it is what puts one free extent around a whole
    segment): the middle one is handed back, what is free in its neighbours stays as a head and a tail."""
    ar = Arena(64)
    base = 1 << 20
    assert ar.take(64) == 0
    ar.add_segment(0xA, base, 64)
    assert ar.take(16) == base and ar.take(48) == base + 16
    ar.add_segment(0xB, base + 64, 64)
    assert ar.take(64) == base + 64
    ar.add_segment(0xC, base + 128, 64)
    assert ar.take(48) == base + 128 and ar.take(16) == base + 176
    assert ar.free_list() == [] and ar.floats() == (64, 192)
    assert ar.give(base + 16, 48) is None and ar.give(base + 128, 48) is None
    assert ar.free_list() == [(base + 16, 48), (base + 128, 48)]
    assert ar.give(base + 64, 64) == (0xB, base + 64, 64)
    assert ar.free_list() == [(base + 16, 48), (base + 128, 48)]
    assert ar.segments() == [(0xA, base, 64), (0xC, base + 128, 64)] and ar.floats() == (64, 128)
    # a segment below the first arena: its offset sorts last, and it goes back as a whole
    low = M - 4096
    assert ar.take(64) is None
    ar.add_segment(0xD, low, 128)
    assert ar.take(64) == low and ar.free_list()[-1] == (low + 64, 64)
    assert ar.give(low, 64) == (0xD, low, 128) and ar.free_list() == [(base + 16, 48), (base + 128, 48)]
    assert ar.floats() == (64, 128)
    ar.close()


def test_cap_reached_and_exceeded():
    ar = Arena(FIRST)
    assert ar.segment_floats(4, 0) == FIRST                        # at least as large as the first arena
    assert ar.segment_floats(6000, 0) == 6000 and ar.segment_floats(5998, 0) == 6000
    assert ar.segment_floats(4, 4 * 2 * FIRST) == FIRST            # exactly reached
    assert ar.segment_floats(4, 4 * 2 * FIRST - 4) == 0            # exceeded by 4 bytes
    ar.add_segment(1, 1 << 20, FIRST)
    assert ar.segment_floats(6000, 4 * (2 * FIRST + 6000)) == 6000
    assert ar.segment_floats(6000, 4 * (2 * FIRST + 6000) - 4) == 0
    ar.close()


def test_random_walk_with_checked_iterators_under_the_sanitizers(tmp_path):
    """tests/cpp/arena_check.cpp: the same kind of walk with the invariants as asserts, built with libstdc++'s checked iterators,
    AddressSanitizer and UBSan -- an iterator used after erase() or insert() ends the program.  The sanitizers' runtimes are linked
    into the program (-static-lib*san), so it runs whatever else the environment loads in front of it."""
    exe = str(tmp_path / "arena_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D_GLIBCXX_DEBUG", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "arena_check.cpp"), "-o", exe])
    for args in (["1", "20000", "0"], ["2", "20000", str(4 * (FIRST + 3 * 6000))]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "arena check ok" in rc.stdout
