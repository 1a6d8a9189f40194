"""Peaks and limiter, CPU tier: the host build of libzl_amd/csrc/zl_limit.h (tests/cpu_harness/limit_host.cpp walks a call the way the
kernels do, chunk by chunk and tile by tile, with the header's own arithmetic) against the numpy restatement (tests/limit_ref.py) with ==
on every float of every extent, every chunk record, every weight table, frames_reduced and min_gain; every float of an extent written
exactly once, no read outside the buffers, no cold tile with a hot frame in its reach; that the grid hits the edges it is aimed at; the
definition's two properties -- the exact ceiling, bit-identity out of reach -- and the clamp's bound on every case; the resolve at every
limit from both sides; the library's host-only calls, the struct layouts, the kernels' resources; the walk under the sanitizers
(tests/cpp/limit_check.cpp).  tests/test_limit_gpu.py holds the kernels themselves to the restatement on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import limit_cases as lc
import limit_ref as lr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32

_h = None
_z = None


def harness():
    global _h
    if _h is None:
        l = C.CDLL(build.build_limit_harness())
        l.zllm_resolve.restype = C.c_int
        l.zllm_resolve.argtypes = [C.c_double, C.POINTER(_abi.LimitRequest)]
        l.zllm_peak_resolve.restype = C.c_int
        l.zllm_peak_resolve.argtypes = [C.c_double, C.c_int32, C.POINTER(_abi.PeakRequest)]
        l.zllm_design.restype = None
        l.zllm_design.argtypes = [C.c_int32, C.c_void_p]
        l.zllm_tables.restype = None
        l.zllm_tables.argtypes = [C.c_void_p]
        l.zllm_table_at.restype = C.c_int32
        l.zllm_table_at.argtypes = [C.c_int32]
        l.zllm_oversampling.restype = C.c_int32
        l.zllm_oversampling.argtypes = [C.c_double]
        l.zllm_extent_floats.restype = C.c_int64
        l.zllm_extent_floats.argtypes = [C.c_int64, C.c_int32]
        l.zllm_call.restype = C.c_int32
        l.zllm_call.argtypes = [C.c_int32] + [C.c_void_p] * 11
        l.zllm_peak_call.restype = C.c_int32
        l.zllm_peak_call.argtypes = [C.c_int32] + [C.c_void_p] * 10
        _h = l
    return _h


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def tables():
    t = np.zeros(384, f32)
    harness().zllm_tables(t.ctypes.data)
    return {4: t[:256].reshape(4, 64).copy(), 2: t[256:].reshape(2, 64).copy()}


def abi_request(q, cid=0):
    return _abi.LimitRequest(cid, int(q.get("flags", 0)), int(q.get("lookahead_frames", 0)), int(q.get("hold_frames", 0)), float(q.get("ceiling", 0.0)), float(q.get("gain", 0.0)))


def extent_source(x, pad=np.nan):
    """the clip as it lies in the arena, with something that is not zero behind the data: the pad is produced, not copied"""
    ch, n = x.shape
    e = np.full(lr.extent_floats(n, ch), pad, f32)
    e[:n * ch] = x.T.reshape(-1)
    return e


def run_call(cases):
    """one harness call over the cases -> (status, results, extents, writes, verdicts, walk)"""
    n = len(cases)
    reqs = (_abi.LimitRequest * n)(*[abi_request(c["q"]) for c in cases])
    srcs = [extent_source(c["x"]) for c in cases]
    dst = [np.full(s.size, np.nan, f32) for s in srcs]
    writes = [np.zeros(s.size, np.int32) for s in srcs]
    ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    nsrc = (C.c_int64 * n)(*[s.size for s in srcs])
    length = (C.c_int32 * n)(*[c["x"].shape[1] for c in cases])
    chans = (C.c_int32 * n)(*[c["x"].shape[0] for c in cases])
    rate = (C.c_double * n)(*[c["rate"] for c in cases])
    out = (_abi.Limit * n)()
    verdicts = (C.c_uint32 * n)()
    walk = (C.c_int64 * 8)()
    pSrc, pDst, pWrites = ptrs(srcs), ptrs(dst), ptrs(writes)
    rc = harness().zllm_call(n, C.addressof(reqs), C.addressof(pSrc), C.addressof(nsrc), C.addressof(length), C.addressof(chans), C.addressof(rate),
                             C.addressof(pDst), C.addressof(pWrites), C.addressof(out), C.addressof(verdicts), C.addressof(walk))
    res = [{k: getattr(out[i], k) for k in lr.RESULT_FIELDS} for i in range(n)]
    return rc, res, dst, writes, list(verdicts), tuple(walk)


def same_result(got, ref):
    for k in lr.RESULT_FIELDS:
        a, b = got[k], ref[k]
        if isinstance(b, (float, np.floating)):
            assert f32(a).view(u32) == f32(b).view(u32), (k, a, b)
        else:
            assert a == b, (k, a, b)


@pytest.fixture(scope="module")
def grid():
    return lc.grid()


@pytest.fixture(scope="module")
def ref(grid):
    t = tables()
    return [lr.limit(c["x"], c["rate"], c["q"], t) for c in grid]


# ---- the grid hits what it is aimed at ------------------------------------------------------------------------------------------------
def test_the_header_and_the_restatement_agree_on_the_shapes():
    h = harness()
    assert (h.zllm_chunk(), h.zllm_tile(), h.zllm_wg()) == (lr.CHUNK, lr.TILE, lr.WG)
    assert [h.zllm_oversampling(r) for r in (44100, 48000, 69999, 70000, 96000, 139999, 140000, 192000)] == [lr.oversampling(r) for r in (44100, 48000, 69999, 70000, 96000, 139999, 140000, 192000)] == [4, 4, 4, 2, 2, 2, 1, 1]
    for ch in (1, 2):
        for n in (1, 2, 3, 4, 5, 1023, 1024, 1025):
            assert h.zllm_extent_floats(n, ch) == lr.extent_floats(n, ch)


def test_the_grid_covers_what_it_is_meant_to(grid, ref):
    by = {}
    for c, r in zip(grid, ref):
        by.setdefault(c["tag"], []).append((c, r))
    T = lr.TILE
    # lengths, both layouts, a hot frame at frame 0 and at the last frame
    assert {(c["x"].shape[0], c["x"].shape[1]) for c, _ in by["length"]} == {(ch, n) for ch in (1, 2) for n in (1, 2, 240, 241, 1023, 1024, 1025, 3 * T + 5)}
    for c, (res, _, _, d) in by["length"]:
        assert res["applied"] and d["hot"][0] and d["hot"][-1] and res["lookahead_frames"] == 240
    # L and H at their limits, hot at a tile's last frame and at the next one's first
    edge = by["tile edge, last frame"] + by["tile edge, first frame"]
    assert {(r[0]["lookahead_frames"], r[0]["hold_frames"]) for _, r in edge} == {(L, H) for L in (1, 2, 240, 512) for H in (0, 1, 512)}
    assert all(r[3]["hot"][T - 1] and r[3]["hot"].sum() == 1 for _, r in by["tile edge, last frame"]) and len(by["tile edge, last frame"]) == 6
    assert all(r[3]["hot"][T] and r[3]["hot"].sum() == 1 for _, r in by["tile edge, first frame"]) and len(by["tile edge, first frame"]) == 6
    # the quiet neighbour tiles are reached
    (c, r), = by["quiet tile before"]
    assert not r[3]["hot"][:T].any() and (r[3]["G"][:T] < 1).any() and (r[3]["G"][:T] == 1).any()
    (c, r), = by["quiet tile behind"]
    assert not r[3]["hot"][T:].any() and (r[3]["G"][T:2 * T] < 1).any() and (r[3]["G"][T:2 * T] == 1).any()
    (c, r), = by["right channel only"]
    assert r[0]["applied"] and np.abs(c["x"][0]).max() < lr.CEILING
    (c, r), = by["at the ceiling"]
    assert not r[0]["applied"] and r[0]["peak_before"] == lr.CEILING
    assert len(by["one ulp above"]) == 2 and all(r[0]["applied"] and r[0]["frames_reduced"] > 0 and r[3]["hot"].sum() == 1 for _, r in by["one ulp above"])
    (c, r), = by["two hot frames"]
    g = r[3]["G"]
    assert r[3]["hot"].sum() == 2 and g[600] < g[500] < 1 and (g[500:600] < 1).all()
    (c, r), = by["plateau"]
    g = r[3]["G"][400 + 16:520 - 16]
    assert r[0]["lookahead_frames"] == 16 and r[0]["hold_frames"] == 8 and g.size > 2 * 16 + 8 and (g == g[0]).all() and g[0] < 1
    (c, r), = by["gain makes it hot"]
    assert r[0]["applied"] and np.abs(c["x"]).max() < lr.CEILING and r[3]["hot"].any()
    (c, r), = by["gain, nothing hot"]
    assert r[0]["applied"] and not r[3]["hot"].any() and r[0]["frames_reduced"] == 0 and np.array_equal(r[1][:c["x"].size], (c["x"] * f32(0.5)).T.reshape(-1))
    assert [r[0]["applied"] for _, r in by["identity"]] == [0, 0] and grid[0]["tag"] == grid[-1]["tag"] == "identity"
    (c, r), = by["overflow"]
    assert np.isinf(r[3]["v"]).any() and np.isinf(r[0]["peak_before"])
    assert [(c["rate"], r[0]["oversampling"]) for c, r in by["true peak, hot sample"]] == [(48000.0, 4), (96000.0, 2), (192000.0, 1)]
    # fs/4 at 45 degrees: the samples are under the ceiling, the peak between them about 3 dB above them and over it
    t = tables()
    for c, r in by["sine45, flag"]:
        pk, rec = lr.peak(c["x"], c["rate"], 0, c["x"].shape[1], lr.TRUE_PEAK, t)
        # (the chunk in the middle sees the steady sine: its amplitude within 1e-4; the ends see the onset against the +0 outside, 1.2 % over)
        assert np.abs(c["x"]).max() < 0.7072 < lr.CEILING and r[0]["applied"] and abs(rec[1, 2] - 1.0) < 1e-4 and 0.99 < pk["true_peak"][0] < 1.02 and r[0]["oversampling"] in (2, 4)
    assert len(by["sine45, flag"]) == 3 and all(not r[0]["applied"] for _, r in by["sine45, no flag"])
    for tag, where in (("inter-sample peak at the start", slice(0, 32)), ("inter-sample peak at the end", slice(-32, None))):
        (c, r), = by[tag]
        assert np.abs(c["x"]).max() < lr.CEILING and r[3]["hot"][where].any() and not r[3]["hot"][32:-32].any()
    (c, r), = by["inter-sample peak at a chunk edge"]
    assert r[3]["hot"][T - 1] and r[3]["hot"][T]
    assert max(c["x"].shape[1] for c in grid) <= 3 * T + 5


# ---- the harness against the restatement ------------------------------------------------------------------------------------------------
def test_the_harness_gives_the_restatements_bits_on_the_grid_in_one_call(grid, ref):
    rc, res, dst, writes, verdicts, walk = run_call(grid)
    assert rc == sum(r[0]["applied"] for r in ref) > 40
    assert walk[3] == 0 and walk[5] == 0 and walk[7] == 0 and walk[0] > 10 and walk[1] > 40, walk
    for i, (c, (want, ext, finite, _)) in enumerate(zip(grid, ref)):
        same_result(res[i], want)
        if not want["applied"]:
            assert not writes[i].any(), c["tag"]
            continue
        assert (writes[i] == 1).all(), c["tag"]
        assert np.array_equal(dst[i].view(u32), ext.view(u32)), (i, c["tag"])
        assert verdicts[i] == (0 if finite else 1), c["tag"]


def test_every_case_alone_gives_the_same_bits(grid, ref):
    for i in (1, 8, 17, 20, len(grid) - 3):
        rc, res, dst, writes, verdicts, walk = run_call([grid[i]])
        assert rc == 1 and np.array_equal(dst[0].view(u32), ref[i][1].view(u32)) and walk[3] == 0


def test_the_ceiling_is_exact_and_what_is_out_of_reach_keeps_its_bits(grid, ref):
    """the definition's two properties and the clamp's bound, on every case, from the restatement (which the harness equals)"""
    checked = 0
    for c, (res, ext, finite, d) in zip(grid, ref):
        if not res["applied"]:
            continue
        n, L, H, cl = c["x"].shape[1], res["lookahead_frames"], res["hold_frames"], res["ceiling"]
        out, v = d["out"], d["v"]
        if finite:
            assert np.abs(out).max() <= cl, c["tag"]
        else:
            assert not (np.abs(out[np.isfinite(out)]) > cl).any(), c["tag"]
        hot = np.flatnonzero(d["hot"])
        reach = np.zeros(n, bool)
        for f in hot:
            reach[max(f - L, 0):f + L + H + 1] = True
        assert np.array_equal(out[:, ~reach].view(u32), v[:, ~reach].view(u32)), c["tag"]
        assert (d["G"][~reach] == 1).all(), c["tag"]
        # the clamp moves a sample by at most |v| (L + 4) 2^-23
        fin = np.isfinite(v) & np.isfinite(d["y"])
        moved = np.abs(d["y"].astype(np.float64) - out.astype(np.float64))[fin]
        bound = (np.abs(v.astype(np.float64)) * (L + 4) * 2.0 ** -23)[fin]
        assert (moved <= bound).all(), (c["tag"], (moved / np.maximum(bound, 1e-300)).max())
        checked += 1
    assert checked > 40


def test_the_window_is_the_restatements_and_sums_to_one():
    for L in (1, 2, 3, 16, 240, 441, 511, 512):
        w = np.zeros(L + 1, f32)
        harness().zllm_design(L, w.ctypes.data)
        want = lr.design(L)
        assert np.array_equal(w.view(u32), want.view(u32)), L
        assert abs(want.astype(np.float64).sum() - 1.0) <= (L + 1) * 2.0 ** -25 and (want > 0).all() and np.array_equal(want, want[::-1])
        z = np.zeros(L + 1, f32)
        assert zlhip().zlhip_limit_design(L, z.ctypes.data) == 0 and np.array_equal(z.view(u32), want.view(u32))
    z = np.zeros(4, f32)
    assert zlhip().zlhip_limit_design(0, z.ctypes.data) == zlhip().zlhip_limit_design(513, z.ctypes.data) == zlhip().zlhip_limit_design(4, None) == _abi.ZLHIP_ERR_INVALID and not z.any()


def test_the_filter_rows_are_section_elevens_table_unchanged():
    z = zlhip()
    t = tables()
    for F, rate in ((4, 48000.0), (4, 44100.0), (2, 96000.0)):
        L, M, taps, row = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        tab = np.zeros(F * 64, f32)
        assert z.zlhip_resample_design(rate, rate * F, C.byref(L), C.byref(M), C.byref(taps), C.byref(row), tab.ctypes.data, tab.size) == 0
        assert (L.value, M.value, taps.value, row.value) == (F, 1, 64, 64)
        assert np.array_equal(tab.view(u32), t[F].reshape(-1).view(u32))
    assert harness().zllm_table_at(4) == 0 and harness().zllm_table_at(2) == 256


# ---- the analysis ---------------------------------------------------------------------------------------------------------------------
def run_peak(cases):
    n = len(cases)
    reqs = (_abi.PeakRequest * n)(*[_abi.PeakRequest(0, first, num, flags) for _, _, first, num, flags in cases])
    srcs = [extent_source(x, 7.0) for x, *_ in cases]
    ptrs = (C.c_void_p * n)(*[s.ctypes.data for s in srcs])
    nsrc = (C.c_int64 * n)(*[s.size for s in srcs])
    length = (C.c_int32 * n)(*[x.shape[1] for x, *_ in cases])
    chans = (C.c_int32 * n)(*[x.shape[0] for x, *_ in cases])
    rate = (C.c_double * n)(*[r for _, r, *_ in cases])
    total = sum((num + lr.CHUNK - 1) // lr.CHUNK for _, _, _, num, _ in cases)
    rec = np.full((total, 4), np.nan, f32)
    rw = np.zeros(total, np.int32)
    out = (_abi.Peak * n)()
    walk = (C.c_int64 * 8)()
    rc = harness().zllm_peak_call(n, C.addressof(reqs), C.addressof(ptrs), C.addressof(nsrc), C.addressof(length), C.addressof(chans), C.addressof(rate),
                                  C.addressof(out), rec.ctypes.data, rw.ctypes.data, C.addressof(walk))
    return rc, out, rec, rw, tuple(walk)


def test_the_analysis_gives_the_restatements_records():
    cases = lc.peak_cases()
    rc, out, rec, rw, walk = run_peak(cases)
    assert rc == rec.shape[0] and (rw == 1).all() and walk[3] == 0
    t = tables()
    at = 0
    for i, (x, rate, first, num, flags) in enumerate(cases):
        want, wrec = lr.peak(x, rate, first, num, flags, t)
        k = wrec.shape[0]
        assert np.array_equal(rec[at:at + k].view(u32), wrec.view(u32)), i
        at += k
        assert (out[i].oversampling, out[i].chunks) == (want["oversampling"], want["chunks"])
        assert np.array_equal(np.array(out[i].sample_peak, f32).view(u32), np.array(want["sample_peak"], f32).view(u32))
        assert np.array_equal(np.array(out[i].true_peak, f32).view(u32), np.array(want["true_peak"], f32).view(u32))
        if x.shape[0] == 1:
            assert out[i].sample_peak[1] == 0 and out[i].true_peak[1] == 0
    # the true peak of the sine is its amplitude, within the filter's ripple; at 192 kHz it is the sample peak
    x = lc.sine45(3 * lr.CHUNK, 0.9, 1)
    for rate in (44100.0, 96000.0, 192000.0):
        p, r = lr.peak(x, rate, 0, x.shape[1], lr.TRUE_PEAK, t)
        if rate < 140000:
            assert abs(r[1, 2] - 0.9) < 1e-4 and p["sample_peak"][0] < 0.64        # (the middle chunk: the steady sine)
        else:
            assert p["true_peak"][0] == p["sample_peak"][0] and not r[:, 2:].any()


# ---- the resolve ------------------------------------------------------------------------------------------------------------------------
def test_the_resolve_at_every_limit_from_both_sides():
    h, z = harness(), zlhip()

    def both(rate, **q):
        a, b = abi_request(q), abi_request(q)
        ra, rb = h.zllm_resolve(rate, C.byref(a)), z.zlhip_limit_resolve(rate, C.byref(b))
        assert (ra == 0) == (rb == 0) and bytes(a) == bytes(b)
        want = lr.resolve(rate, q)
        assert (want is None) == (ra != 0)
        if want is not None:
            assert (a.lookahead_frames, a.hold_frames, a.flags) == (want["lookahead_frames"], want["hold_frames"], want["flags"])
            assert f32(a.ceiling) == want["ceiling"] and f32(a.gain) == want["gain"]
        else:
            assert bytes(a) == bytes(abi_request(q))                  # a refused request is left as it was
        return None if ra else a

    d = both(48000.0)
    assert (d.lookahead_frames, d.hold_frames) == (240, 0) and f32(d.ceiling) == f32(0.8912509381337456) and d.gain == 1.0
    assert both(44100.0).lookahead_frames == 221 and both(100.0).lookahead_frames == 1 and both(192000.0).lookahead_frames == 512 and both(102500.0).lookahead_frames == 512
    assert both(102300.0).lookahead_frames == 512 and both(102299.0).lookahead_frames == 511
    for ok in (dict(lookahead_frames=1), dict(lookahead_frames=512), dict(hold_frames=512), dict(ceiling=1.0), dict(ceiling=1e-30), dict(gain=3e38), dict(gain=1e-40), dict(flags=1)):
        assert both(48000.0, **ok) is not None, ok
    for bad in (dict(lookahead_frames=-1), dict(lookahead_frames=513), dict(hold_frames=-1), dict(hold_frames=513), dict(ceiling=float(np.nextafter(f32(1), f32(2)))), dict(ceiling=-0.5),
                dict(ceiling=float("nan")), dict(ceiling=float("inf")), dict(gain=-1.0), dict(gain=float("inf")), dict(gain=float("nan")), dict(flags=2), dict(flags=3), dict(flags=-1)):
        assert both(48000.0, **bad) is None, bad
    # the flag at a rate section 11's design refuses
    for rate, ok in ((48000.0, True), (999.0, False), (1000.0, True), (48000.5, False), (768000.0, True), (768001.0, False), (192000.0, True)):
        assert (both(rate, flags=1) is not None) == ok, rate
        assert both(rate) is not None
    for rate, length, first, num, flags, ok in ((48000.0, 10, 0, 10, 0, True), (48000.0, 10, 0, 11, 0, False), (48000.0, 10, 9, 1, 1, True), (48000.0, 10, 10, 1, 0, False),
                                                (48000.0, 10, -1, 2, 0, False), (48000.0, 10, 0, 0, 0, False), (48000.0, 10, 0, 1, 2, False), (48000.5, 10, 0, 1, 1, False),
                                                (48000.5, 10, 0, 1, 0, True), (48000.0, 2 ** 31 - 1, 2 ** 31 - 2, 1, 0, True), (48000.0, 2 ** 31 - 1, 2 ** 31 - 2, 2, 0, False)):
        q = _abi.PeakRequest(0, first, num, flags)
        assert (h.zllm_peak_resolve(rate, length, C.byref(q)) == 0) == ok == (z.zlhip_peak_resolve(rate, length, C.byref(q)) == 0), (rate, length, first, num, flags)


# ---- the C-ABI without a GPU, the layouts, the kernels' resources ---------------------------------------------------------------------
def test_without_a_gpu_the_calls_answer_invalid(built):
    l = zlhip()
    q, p = abi_request({}), _abi.PeakRequest(0, 0, 1, 0)
    out, pout = _abi.Limit(), _abi.Peak()
    C.memset(C.byref(out), 0x5A, C.sizeof(out)); C.memset(C.byref(pout), 0x5A, C.sizeof(pout))
    assert l.zlhip_sound_limit(None, C.byref(q), C.byref(out)) == l.zlhip_sound_limit_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_peak(None, C.byref(p), C.byref(pout)) == l.zlhip_sound_peak_batch(None, C.byref(p), 1, C.byref(pout)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_limit_batch(None, C.byref(q), 1, C.byref(out)) == l.zlhip_group_sound_peak_batch(None, C.byref(p), 1, C.byref(pout)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_limit_timings(None, None, None) == l.zlhip_debug_peak_chunks(None, 0, None, 0, None) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_limit_resolve(48000.0, None) == l.zlhip_peak_resolve(48000.0, 1, None) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * C.sizeof(out) and bytes(pout) == b"\x5a" * C.sizeof(pout)
    assert l.zlhip_abi_version() == 3


def test_limit_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_peak_request", _abi.PeakRequest), ("zlhip_peak", _abi.Peak), ("zlhip_peak_chunk", _abi.PeakChunk), ("zlhip_limit_request", _abi.LimitRequest), ("zlhip_limit", _abi.Limit))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    body += 'printf("%d ",ZLHIP_LIMIT_TRUE_PEAK);'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-1] == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:5] == [16, 24, 16, 24, 40] and got[-1] == _abi.LIMIT_TRUE_PEAK == lr.TRUE_PEAK
    assert [f for f, _ in _abi.Limit._fields_ if f != "reserved"] == list(lr.RESULT_FIELDS)


def test_limit_kernels_have_no_scratch_memory(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_limit_kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resources of zl_limit.hip's kernels"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    detect = [r for n, r in rows.items() if "zl_k_limit_detect" in n]
    render = [r for n, r in rows.items() if "zl_k_limit_render" in n]
    assert len(detect) == 1 and len(render) == 1 and len(rows) == 2, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    # detect: v planar over a chunk and its taps, and sixteen words for the reduction; render: v, ips, r, mr transposed, eight words
    # (plus what the arrays' alignment adds: below 128 bytes)
    assert 0 <= detect[0]["lds"] - (2 * (1024 + 63) * 4 + 64) < 128 and detect[0]["vgprs"] <= 48 and detect[0]["waves"] >= 8, rows
    assert 0 <= render[0]["lds"] - (2 * 2624 + 2561 + 2560 + 1600 + 8) * 4 < 128 and render[0]["vgprs"] <= 64 and render[0]["waves"] >= 3, rows


# ---- the walk under the sanitizers ------------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/limit_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with AddressSanitizer
    and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment loads
    in front of it."""
    exe = str(tmp_path / "limit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "limit_check.cpp"), "-o", exe])
    for args in (["1", "12"], ["2", "12"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "limit check ok" in rc.stdout
