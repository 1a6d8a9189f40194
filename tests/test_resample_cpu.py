"""Sample-rate conversion, CPU tier: zlhip_resample_design (the library's own table) against the numpy restatement
(tests/resample_ref.py); the host build of libzl_amd/csrc/zl_resample.h (tests/cpu_harness/resample_host.cpp walks a clip the way
the kernel does, with the library's table) against the restatement bit for bit, with every float of the extent written exactly once
and no read outside the clip's own floats (the harness reads the source through an accessor that checks the index against the
buffer); what the definition does to sines (it guards the design constants, not the kernel); the new kernels' resources and what the C-ABI answers without a GPU; the header's position and span at the far end of the range
(j * M beyond 2^31) against Python integers.  tests/test_resample_gpu.py and tests/test_resample_geometry_gpu.py hold the kernel itself
to the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as rr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32

# (fs, ft) -> what the issue states about the ratio
RATIOS = {
    (44100, 48000): {"L": 160, "M": 147, "T": 64},
    (48000, 44100): {"L": 147, "M": 160, "T": 70},
    (96000, 48000): {"L": 1, "T": 128},
    (8000, 48000): {"L": 6, "M": 1},
    (22050, 48000): {"L": 320},
    (192000, 44100): {"T": 280},
    # the geometries of tests/test_resample_geometry_gpu.py: an odd `half` while downsampling, M = 8 L (the staging at its limit),
    # L at its limit, the table at its limit (2048 * 128 = 262144 floats), the lowest and the highest accepted rate
    (88200, 48000): {"L": 80, "M": 147, "T": 118},
    (384000, 48000): {"L": 1, "M": 8, "T": 512},
    (51175, 51200): {"L": 2048, "M": 2047, "T": 64},
    (102375, 51200): {"L": 2048, "M": 4095, "T": 128},
    (1000, 6000): {"L": 6, "M": 1, "T": 64},
    (768000, 96000): {"L": 1, "M": 8, "T": 512},
}

_h = None
_z = None


def harness():
    global _h
    if _h is None:
        l = C.CDLL(build.build_resample_harness())
        l.zl_rs_host_geometry.restype = C.c_int
        l.zl_rs_host_geometry.argtypes = [C.c_double, C.c_double, C.c_void_p]
        l.zl_rs_host_out_frames.restype = C.c_int64
        l.zl_rs_host_out_frames.argtypes = [C.c_double, C.c_double, C.c_int64]
        l.zl_rs_host_extent_floats.restype = C.c_int64
        l.zl_rs_host_extent_floats.argtypes = [C.c_int64, C.c_int32]
        l.zl_rs_host_design.restype = C.c_int
        l.zl_rs_host_design.argtypes = [C.c_double, C.c_double, C.c_void_p]
        l.zl_rs_host_convert.restype = C.c_int64
        l.zl_rs_host_convert.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.zl_rs_host_stage_frames.restype = C.c_int32
        l.zl_rs_host_stage_frames.argtypes = []
        l.zl_rs_host_walk.restype = C.c_int
        l.zl_rs_host_walk.argtypes = [C.c_double, C.c_double, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
        _h = l
    return _h


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


_tables = {}


def library_table(fs, ft):
    """(L, M, taps, row, table [L, row]) from zlhip_resample_design"""
    if (fs, ft) not in _tables:
        L, M, T, row = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        assert zlhip().zlhip_resample_design(fs, ft, C.byref(L), C.byref(M), C.byref(T), C.byref(row), None, 0) == 0, (fs, ft)
        table = np.full((L.value, row.value), np.nan, f32)
        assert zlhip().zlhip_resample_design(fs, ft, None, None, None, None, table.ctypes.data, table.size) == 0
        _tables[(fs, ft)] = (L.value, M.value, T.value, row.value, table)
    return _tables[(fs, ft)]


# ---- the design -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,ft", list(RATIOS))
def test_design_matches_the_restatement(built, fs, ft):
    L, M, T, row, table = library_table(fs, ft)
    rL, rM, rhalf, rT, rrow = rr.geometry(fs, ft)
    assert (L, M, T, row) == (rL, rM, rT, rrow)
    for k, v in RATIOS[(fs, ft)].items():
        assert {"L": L, "M": M, "T": T}[k] == v, (fs, ft, k)
    ref = rr.design(fs, ft)
    assert table.shape == ref.shape
    assert np.all(table[:, T:] == 0.0) and not np.any(np.signbit(table[:, T:]))
    # both sides round a double evaluation whose absolute error is far below 1e-12: they may differ by one fp32 rounding
    tol = np.maximum(rr.ulp32(ref), 1e-12)
    d = np.abs(table.astype(np.float64) - ref.astype(np.float64))
    assert np.all(d <= tol), (fs, ft, float(d.max()))
    sums = table[:, :T].astype(np.float64).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) <= 4 * rr.ulp32(f32(1.0))), (fs, ft, float(np.abs(sums - 1.0).max()))
    # the harness's table is the header's, the library's is the header's: the same bits
    mine = np.zeros_like(table)
    assert harness().zl_rs_host_design(fs, ft, mine.ctypes.data) == 0
    assert np.array_equal(mine.view(u32), table.view(u32))


def test_design_sizes_only_and_capacity(built):
    L, M, T, row = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert zlhip().zlhip_resample_design(44100.0, 48000.0, C.byref(L), C.byref(M), C.byref(T), C.byref(row), None, 0) == 0
    assert (L.value, M.value, T.value, row.value) == (160, 147, 64, 64)
    small = np.zeros(160 * 64 - 1, f32)
    assert zlhip().zlhip_resample_design(44100.0, 48000.0, None, None, None, None, small.ctypes.data, small.size) == _abi.ZLHIP_ERR_CAPACITY
    assert not small.any()
    assert zlhip().zlhip_resample_design(48000.0, 44100.0, None, None, C.byref(T), C.byref(row), None, 0) == 0
    assert (T.value, row.value) == (70, 72)


@pytest.mark.parametrize("fs,ft", [(44100, 47999), (48000, 5000), (44100.5, 48000), (44100, 48000.25), (999, 48000), (48000, 768001),
                                   (0, 48000), (-44100, 48000), (float("nan"), 48000), (48000, float("inf"))])
def test_design_rejects(built, fs, ft):
    assert zlhip().zlhip_resample_design(fs, ft, None, None, None, None, None, 0) == _abi.ZLHIP_ERR_INVALID
    out = (C.c_int32 * 5)()
    assert harness().zl_rs_host_geometry(fs, ft, out) == -1
    if fs == fs and abs(ft) != float("inf"):
        assert rr.geometry(fs, ft) is None


# ---- the bits -------------------------------------------------------------------------------------------------------------------
def source(rng, n, ch):
    x = rng.uniform(-1.0, 1.0, (n, ch)).astype(f32)
    special = np.array([0.0, -0.0, 1e-39, -1e-39, 1.0, -1.0], f32)   # +-0, denormals, +-1
    at = rng.integers(0, n, size=max(1, n // 5))
    x[at, rng.integers(0, ch, size=at.size)] = special[rng.integers(0, special.size, size=at.size)]
    return x


def run_harness(fs, ft, table, x, src_floats=None):
    n, ch = x.shape
    N = rr.out_frames(fs, ft, n)
    assert harness().zl_rs_host_out_frames(fs, ft, n) == N
    floats = harness().zl_rs_host_extent_floats(N, ch)
    dst = np.full(floats, np.nan, f32)
    writes = np.zeros(floats, np.int32)
    verdict = C.c_uint32(9)
    # the source in a buffer of its own size; the harness's accessor refuses (and counts) a read at an index outside [0, src_floats)
    src = np.ascontiguousarray(x.reshape(-1))
    refused = harness().zl_rs_host_convert(fs, ft, table.ctypes.data, src.ctypes.data, src.size if src_floats is None else src_floats, n, ch, dst.ctypes.data, writes.ctypes.data, C.byref(verdict))
    return dst, writes, refused, verdict.value


def lengths(fs, ft):
    half, T = rr.geometry(fs, ft)[2:4]
    out = [1, 2, 63, 64, 65, 1000, half - 1, half, half + 1, T + 1]   # (shorter than the filter: both ends of the taps hang outside)
    for N in (255, 256, 257, 513):                                 # the workgroup edges
        out += rr.lengths_for(fs, ft, N)
    return sorted(set(out))


@pytest.mark.parametrize("fs,ft", list(RATIOS))
@pytest.mark.parametrize("ch", [1, 2])
def test_harness_matches_the_restatement_bit_for_bit(built, fs, ft, ch):
    table = library_table(fs, ft)[4]
    rng = np.random.default_rng(fs * 7 + ft + ch)
    counts = set()
    for n in lengths(fs, ft):
        counts.add(int(harness().zl_rs_host_out_frames(fs, ft, n)))
        x = source(rng, n, ch)
        got, writes, refused, verdict = run_harness(fs, ft, table, x)
        ref = rr.extent(rr.convert(table, fs, ft, x))
        assert got.size == ref.size
        assert np.all(writes == 1), (fs, ft, ch, n, np.flatnonzero(writes != 1)[:8])
        assert refused == 0
        assert np.array_equal(got.view(u32), ref.view(u32)), (fs, ft, ch, n, np.flatnonzero(got.view(u32) != ref.view(u32))[:8])
        assert verdict == 0
    # the workgroup edges were among them: N = 255, 256, 257 and 513 where a length gives them (a ratio that goes down reaches every
    # count); an upsampling ratio skips counts (1:6 gives multiples of 6): there a count on either side of the edge
    for N in (255, 256, 257, 513):
        assert N in counts or (ft > fs and any(c < N for c in counts if c > N - 8) and any(c > N for c in counts if c < N + 8)), (fs, ft, N, sorted(counts))


def walk(fs, ft, length, j, w):
    """(rc, N, i, p, first, count) of the header's zl_rs_out_frames, zl_rs_position(j) and zl_rs_span(w)"""
    out = (C.c_int64 * 5)()
    rc = harness().zl_rs_host_walk(fs, ft, length, j, w, out)
    return (rc,) + tuple(out)


def test_the_staging_reaches_its_limit_at_eight_to_one_and_never_passes_it(built):
    """M = 8 L, T = 512: a full workgroup stages 255 * 8 + 512 = 2552 frames, one below ZL_RS_STAGE_FRAMES.  The harness answers -2
    where a span is longer than the stage or a lane's taps leave it"""
    fs, ft = 384000, 48000
    assert harness().zl_rs_host_stage_frames() == rr.STAGE_FRAMES == 2553
    table = library_table(fs, ft)[4]
    rng = np.random.default_rng(17)
    counts = []
    for n in lengths(fs, ft) + [8 * 256 * 3 + 5]:
        N = rr.out_frames(fs, ft, n)
        got, writes, refused, verdict = run_harness(fs, ft, table, source(rng, n, 2))
        assert refused == 0 and np.all(writes == 1), (n, refused)   # (-2 is not 0)
        for w in range((N + rr.WG - 1) // rr.WG):
            rc, hN, _, _, first, count = walk(fs, ft, n, 0, w)
            assert rc == 0 and hN == N and (first, count) == rr.span(fs, ft, N, w), (n, w)
            counts.append(count)
    assert max(counts) == rr.STAGE_FRAMES - 1, max(counts)
    # no accepted ratio passes it: the span of a full workgroup is floor(255 M / L) + T at most
    for (a, b) in RATIOS:
        L, M, half, T, _ = rr.geometry(a, b)
        assert (255 * M) // L + 1 + T <= rr.STAGE_FRAMES, (a, b)


INT32_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("fs,ft", [(384000, 48000), (51175, 51200), (44100, 48000)])
def test_position_and_span_at_the_far_end_of_the_range(built, fs, ft):
    """the longest clip the definition takes (N + 8 <= INT32_MAX; j * M passes 2^31, which no small device shape reaches): the
    header's position and span against Python integers at the first, a middle and the last workgroup, every lane's first tap inside
    the staged span, and zl_rs_out_frames answering 0 one frame beyond"""
    L, M, half, T, _ = rr.geometry(fs, ft)
    n = ((INT32_MAX - 8) * M) // L
    while (n * L + M - 1) // M + 8 > INT32_MAX:
        n -= 1
    while ((n + 1) * L + M - 1) // M + 8 <= INT32_MAX:
        n += 1
    N = (n * L + M - 1) // M
    if M >= L:
        assert N + 8 == INT32_MAX                                  # (a ratio that goes down reaches every count)
    else:
        assert INT32_MAX - 8 - (L + M - 1) // M < N <= INT32_MAX - 8
    assert harness().zl_rs_host_out_frames(fs, ft, n) == N
    assert harness().zl_rs_host_out_frames(fs, ft, n + 1) == 0 and walk(fs, ft, n + 1, 0, 0)[0] == -3
    wgs = (N + rr.WG - 1) // rr.WG
    assert (N - 1) * M > 2 ** 31
    for w in (0, wgs // 2, wgs - 1):
        first, count = rr.span(fs, ft, N, w)
        assert 0 < count <= rr.STAGE_FRAMES
        j0, j1 = w * rr.WG, min((w + 1) * rr.WG, N) - 1
        assert j1 == N - 1 or w < wgs - 1
        for j in sorted({j0, j0 + 1, (j0 + j1) // 2, j1 - 1, j1}):
            rc, hN, i, p, hfirst, hcount = walk(fs, ft, n, j, w)
            assert rc == 0 and hN == N
            assert (i, p) == rr.position(fs, ft, j), (w, j)
            assert (hfirst, hcount) == (first, count), (w, j)
            o = i - half + 1 - hfirst
            assert 0 <= o and o + T <= hcount, (w, j, o)
        # the last input frame a lane of the last workgroup reads lies at most `half` behind the clip
        if w == wgs - 1:
            assert first + count - 1 <= n - 1 + half


def test_the_harness_refuses_a_read_outside_the_buffer_it_was_given(built):
    """the refusal is the accessor's, not the staging mask's: told that the buffer is one float shorter than the clip, the same walk is
    refused exactly the reads of that float, and the NaN it gets instead shows in the output"""
    fs, ft = 44100, 48000
    table = library_table(fs, ft)[4]
    x = source(np.random.default_rng(3), 300, 2)
    got, writes, refused, verdict = run_harness(fs, ft, table, x)
    assert refused == 0 and verdict == 0
    got, writes, refused, verdict = run_harness(fs, ft, table, x, src_floats=x.size - 1)
    assert refused == 1 and verdict == 1 and np.all(writes == 1)   # of the two workgroups (327 frames) only the second stages frame 299
    assert np.isnan(got[1::2][:327]).any() and not np.isnan(got[0::2]).any()


def test_non_finite_input_sets_the_verdict_and_stays_local(built):
    fs, ft = 44100, 48000
    L, M, T, row, table = library_table(fs, ft)
    half = T // 2
    rng = np.random.default_rng(5)
    x = source(rng, 1000, 2)
    clean = rr.convert(table, fs, ft, x)
    x[500, 1] = np.inf
    got, writes, refused, verdict = run_harness(fs, ft, table, x)
    assert verdict == 1 and refused == 0 and np.all(writes == 1)
    N = clean.shape[0]
    y = got[:N * 2].reshape(N, 2)
    centre = (np.arange(N, dtype=np.int64) * M) // L
    far = np.abs(centre - 500) > half                              # farther than `half` input frames from the non-finite sample
    assert np.array_equal(y[far].view(u32), clean[far].view(u32))
    assert np.array_equal(y[:, 0].view(u32), clean[:, 0].view(u32))   # the other channel never sees it
    assert not np.all(np.isfinite(y[~far, 1]))


# ---- the quality of the definition ----------------------------------------------------------------------------------------------
def db(v):
    return 20.0 * np.log10(max(float(v), 1e-30))


def sine(fs, hz, seconds=0.5):
    n = int(fs * seconds)
    return np.sin(2.0 * np.pi * hz * np.arange(n, dtype=np.float64) / fs).astype(f32)[:, None]


def rms_error(fs, ft, hz, y):
    N = y.shape[0]
    exact = np.sin(2.0 * np.pi * hz * np.arange(N, dtype=np.float64) / ft)
    e = y[:, 0].astype(np.float64) - exact
    return float(np.sqrt(np.mean(e[2000:N - 2000] ** 2)))


# (fs, ft, tone): passband, RMS error against the exact sine; the definition measures -103 dB or better at every one of them
PASSBAND = [(44100, 48000, 1000), (44100, 48000, 18000), (48000, 44100, 1000), (48000, 44100, 18000), (96000, 48000, 20000), (22050, 48000, 9000)]
# stopband: what is left of a tone the target rate cannot hold, as output RMS; the definition measures -101 dB or better
STOPBAND = [(96000, 48000, 26000), (96000, 48000, 30000), (48000, 44100, 23999)]


@pytest.mark.parametrize("fs,ft,hz", PASSBAND)
def test_passband_error_is_below_minus_90_db(built, fs, ft, hz):
    table = library_table(fs, ft)[4]
    y = rr.convert(table, fs, ft, sine(fs, hz))
    assert db(rms_error(fs, ft, hz, y)) <= -90.0, db(rms_error(fs, ft, hz, y))


@pytest.mark.parametrize("fs,ft,hz", STOPBAND)
def test_stopband_is_below_minus_90_db(built, fs, ft, hz):
    table = library_table(fs, ft)[4]
    y = rr.convert(table, fs, ft, sine(fs, hz))[:, 0].astype(np.float64)
    rms = float(np.sqrt(np.mean(y[2000:-2000] ** 2)))
    assert db(rms) <= -90.0, db(rms)


@pytest.mark.parametrize("fs,ft", [(44100, 48000), (48000, 44100)])
def test_linear_resampling_of_18_khz_fails_the_same_bound_by_tens_of_db(built, fs, ft):
    """the feature's reason: the voice's own two-tap resampler, which is what a clip at a foreign rate plays through"""
    y = rr.linear(fs, ft, sine(fs, 18000))
    assert db(rms_error(fs, ft, 18000, y)) >= -90.0 + 20.0, db(rms_error(fs, ft, 18000, y))


@pytest.mark.parametrize("fs,ft", list(RATIOS))
def test_dc_stays_dc(built, fs, ft):
    L, M, T, row, table = library_table(fs, ft)
    x = np.ones((4000, 1), f32)
    y = rr.convert(table, fs, ft, x)[:, 0]
    edge = int(np.ceil(T * L / M)) + 2                             # output frames whose taps reach over an end
    assert np.all(np.abs(y[edge:-edge].astype(np.float64) - 1.0) <= 1e-6), float(np.abs(y[edge:-edge] - 1.0).max())


# ---- the C-ABI without a GPU, the kernels' resources ----------------------------------------------------------------------------
def test_without_a_gpu_the_calls_answer_invalid(built):
    l = zlhip()
    ids = (C.c_int32 * 1)(0)
    info = _abi.SoundInfo()
    assert l.zlhip_sound_convert_rate(None, 0, 48000.0) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_convert_rate_batch(None, ids, 1, 48000.0) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_convert_rate_batch(None, ids, 1, 48000.0) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_info_get(None, 0, C.byref(info)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_convert_timings(None, None) == _abi.ZLHIP_ERR_INVALID


def test_resample_kernels_have_no_scratch_memory(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_resample_kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resources of zl_resample.hip's kernels"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    assert sorted(n for n in rows if "zl_k_resample" in n) and len(rows) == 2, rows
    assert any("zl_k_resample_publish" in n for n in rows) and any("zl_k_resample" in n and "publish" not in n for n in rows), rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    main = [r for n, r in rows.items() if "publish" not in n][0]
    assert 0 < main["lds"] <= 21 * 1024, rows                      # the staged frames: at most 2553 stereo frames
