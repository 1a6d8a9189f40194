"""Waveform overviews, CPU tier: the host build of libzl_amd/csrc/zl_overview.h (tests/cpu_harness/overview_host.cpp walks a request
the way the kernel does, with the header's own arithmetic) against the numpy restatement (tests/overview_ref.py) -- column bounds,
the cut into pieces with its masked 16-byte groups, the sample order -- and the new kernels' resources.
tests/test_overview_gpu.py holds the kernels themselves to the restatement on the GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import overview_ref as ov
from libzl_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32 = np.uint32

FRAMES = (1, 2, 3, 63, 64, 65, 4099)
COLUMNS = (1, 2, 3, 7, 64, 100, 4096)
FIRSTS = (0, 1, 3)
PAD = 8

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_overview_harness())
        l.zlov_key.restype = l.zlov_unkey.restype = C.c_uint32
        l.zlov_key.argtypes = l.zlov_unkey.argtypes = [C.c_uint32]
        l.zlov_column.restype = None
        l.zlov_column.argtypes = [C.c_int64] * 4 + [C.POINTER(C.c_int64)] * 2
        l.zlov_pieces_per_column.restype = C.c_int32
        l.zlov_pieces_per_column.argtypes = [C.c_int64, C.c_int64]
        l.zlov_items.restype = C.c_int64
        l.zlov_items.argtypes = [C.c_int64, C.c_int64]
        l.zlov_run.restype = C.c_int64
        l.zlov_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def host_bounds(first, n, columns):
    lo, hi = C.c_int64(0), C.c_int64(0)
    out = np.zeros((columns, 2), np.int64)
    for c in range(columns):
        lib().zlov_column(first, n, columns, c, C.byref(lo), C.byref(hi))
        out[c] = lo.value, hi.value
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", FRAMES)
def test_column_bounds(n, first):
    for columns in COLUMNS:
        lo, hi = host_bounds(first, n, columns)
        rlo, rhi = ov.bounds(first, n, columns)
        assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (n, columns, first)
        # the formula itself, in Python's integers
        assert [int(v) for v in lo] == [first + (c * n) // columns for c in range(columns)]
        assert (hi > lo).all() and lo[0] == first and (lo >= first).all() and (hi <= first + n).all() and hi[-1] == first + n
        assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all()
        if columns <= n:
            assert np.array_equal(lo[1:], hi[:-1])                 # the columns tile [first, first + n) in order
            w = hi - lo
            assert w.max() - w.min() <= 1
        else:
            assert ((hi - lo) == 1).all()


def extent(planar):
    """the arena extent of a sound: interleaved, 8 zero frames behind it, rounded up to 16 bytes"""
    ch, length = planar.shape
    words = ((length + PAD) * ch + 3) & ~3
    ext = np.zeros(words, u32)
    ext[:length * ch] = planar.T.reshape(-1).view(u32)
    return ext


def run(planar, first, n, columns):
    ch, length = planar.shape
    ext = extent(planar)
    visits = np.zeros(ext.size, np.int32)
    owner = np.full(ext.size, -1, np.int32)
    out = np.zeros((columns, 4), u32)
    top = lib().zlov_run(ext.ctypes.data, ch, first, n, columns, visits.ctypes.data, owner.ctypes.data, out.ctypes.data)
    return out.view(np.float32), visits, owner, top, ext.size


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("first", FIRSTS)
def test_every_frame_of_every_column_is_visited_exactly_once(ch, first):
    for n, columns in itertools.product(FRAMES, COLUMNS):
        for tail in (0, 1, 2, 3, 5):                               # frames of the sound behind the request: the last group's tail is masked
            length = first + n + tail
            x = np.random.default_rng(n + columns).uniform(0.25, 1.0, (ch, length)).astype(np.float32)
            out, visits, owner, top, words = run(x, first, n, columns)
            assert top >= 0, "a piece is empty or longer than the bound"
            assert top < words, (n, columns, first, tail, "a load leaves the extent")
            lo, hi = ov.bounds(first, n, columns)
            expect = np.zeros(words, np.int32)
            for c in range(columns):                               # (more columns than frames: a frame is in several columns)
                expect[lo[c] * ch:hi[c] * ch] += 1
            assert np.array_equal(visits, expect), (n, columns, first, tail, np.flatnonzero(visits != expect)[:8])
            if columns <= n:
                own = np.full(words, -1, np.int32)
                for c in range(columns):
                    own[lo[c] * ch:hi[c] * ch] = c
                assert np.array_equal(owner, own), (n, columns, first, tail)
            assert ov.same_bits(out, ov.overview(x, columns, first, n)), (n, columns, first, tail)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_long_columns_are_cut_into_pieces_that_cover_them(ch):
    """columns of thousands of frames: several pieces per column, piece edges at every alignment"""
    l = lib()
    for n, columns, first in ((70001, 1, 0), (70001, 7, 3), (20011, 3, 1), (9973, 2, 5), (4099, 3, 2)):
        assert l.zlov_pieces_per_column(n, columns) >= 2
        x = np.random.default_rng(n).uniform(-1.0, 1.0, (ch, first + n + 3)).astype(np.float32)
        out, visits, owner, top, words = run(x, first, n, columns)
        assert 0 <= top < words
        lo, hi = ov.bounds(first, n, columns)
        expect = np.zeros(words, np.int32)
        expect[first * ch:(first + n) * ch] = 1
        assert np.array_equal(visits, expect)
        assert np.array_equal(owner[first * ch:(first + n) * ch], np.repeat(np.arange(columns), (hi - lo) * ch))
        assert ov.same_bits(out, ov.overview(x, columns, first, n))
        assert ov.same_bits(out, ov.overview(x, columns, first, n, loop=True))


def test_items_count_the_waves_of_both_forms():
    l = lib()
    for n, columns in itertools.product(FRAMES + (70001, 2 ** 31 - 1), COLUMNS):
        w = 1 if n <= columns else -(-n // columns)
        ppc = l.zlov_pieces_per_column(n, columns)
        if w <= l.zlov_narrow_frames():
            assert ppc == 0 and l.zlov_items(n, columns) == -(-columns // 64)
        else:
            assert ppc == -(-w // l.zlov_piece_frames()) and l.zlov_items(n, columns) == columns * ppc


SPECIAL = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800001,            # NaNs with the sign bit set (the largest payload lowest)
                    0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80000001, 0x80000000,     # -inf, -FLT_MAX, -1, -denormal min, -0
                    0x00000000, 0x00000001, 0x3F800000, 0x7F7FFFFF, 0x7F800000,     # +0, +denormal min, 1, FLT_MAX, +inf
                    0x7F800001, 0x7FC00000, 0x7FFFFFFF], u32)      # NaNs with the sign bit clear


def test_key_map_round_trips_and_is_strictly_monotone():
    l = lib()
    keys = np.array([l.zlov_key(int(b)) for b in SPECIAL], np.uint64)
    assert (np.diff(keys.astype(np.int64)) > 0).all(), keys        # SPECIAL is listed in the order of the definition
    assert np.array_equal(keys.astype(u32), ov.key(SPECIAL))
    # key and unkey undo each other, on the list and on random words, and agree with the restatement
    rng = np.random.default_rng(1)
    words = np.concatenate([SPECIAL, rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(u32)])
    for b in words:
        k = l.zlov_key(int(b))
        assert l.zlov_unkey(k) == int(b) and l.zlov_key(l.zlov_unkey(int(b))) == int(b)
    assert np.array_equal(ov.unkey(ov.key(words)), words)
    # on ordinary floats the integer order is the float order
    f = np.sort(rng.uniform(-2.0, 2.0, 1000).astype(np.float32))
    assert (np.diff(ov.key(f.view(u32)).astype(np.int64)) >= 0).all()


def test_special_values_come_back_with_their_own_bits():
    for ch in (1, 2):
        x = np.tile(SPECIAL, 80)[:600 * ch].reshape(ch, -1).view(np.float32)
        x = np.ascontiguousarray(np.random.default_rng(3).permutation(x, axis=1))
        for columns, first, n in ((1, 0, 600), (7, 1, 597), (64, 3, 300), (600, 0, 600), (4096, 2, 3)):
            out, *_ = run(x, first, n, columns)
            assert ov.same_bits(out, ov.overview(x, columns, first, n, loop=True)), (ch, columns)
    # min and max of the whole list: the lowest negative NaN, the highest positive one
    out, *_ = run(SPECIAL.view(np.float32)[None, :], 0, SPECIAL.size, 1)
    assert list(out.view(u32)[0]) == [0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FFFFFFF]


def test_overview_request_struct_layout(tmp_path):
    import subprocess
    from libzl_amd import _abi
    prog = tmp_path / "p.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){printf("%d %d %d %d %d %d\\n",(int)sizeof(zlhip_overview_request),'
                    '(int)offsetof(zlhip_overview_request,id),(int)offsetof(zlhip_overview_request,first_frame),'
                    '(int)offsetof(zlhip_overview_request,num_frames),(int)offsetof(zlhip_overview_request,columns),ZLHIP_OVERVIEW_MAX_COLUMNS);return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _abi.OverviewRequest
    assert got == [C.sizeof(P), P.id.offset, P.first_frame.offset, P.num_frames.offset, P.columns.offset, _abi.OVERVIEW_MAX_COLUMNS] == [16, 0, 4, 8, 12, 4096]


def test_overview_kernels_have_no_scratch_memory(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_overview_kernel_resources.txt")
    if not os.path.exists(path):
        pytest.skip("no zl_overview kernel resources file (the library was not built by this build.py)")
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    reduce_ = [r for n, r in rows.items() if "zl_k_overview_reduce" in n]
    finish = [r for n, r in rows.items() if "zl_k_overview_finish" in n]
    assert len(reduce_) == 1 and len(finish) == 1 and len(rows) == 2, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, rows
    assert reduce_[0]["waves"] >= 8, rows                          # the reduction hides HBM latency with resident waves
