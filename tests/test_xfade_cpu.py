"""Loop crossfade, CPU tier: the host build of libzl_amd/csrc/zl_xfade.h (tests/cpu_harness/xfade_host.cpp walks a call the way the
kernels do, workgroup by workgroup and group by group, with the header's own arithmetic) against the numpy / Python-integer restatement
(tests/xfade_ref.py) with == on every float of every extent, on the three integers, on correlation, rho and both weights of every
frame, every float of an extent written exactly once and no read outside the buffer the harness was given; the resolve at every limit
from both sides; what the definition does to sound, on the restatement alone; the library's host-only calls, the struct layouts, the
new kernels' resources; the walk under the sanitizers (tests/cpp/xfade_check.cpp).  tests/test_xfade_gpu.py holds the kernels
themselves to the restatement on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import xfade_cases as xc
import xfade_ref as xr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
f32, u32 = np.float32, np.uint32

_h = None
_z = None


def harness():
    global _h
    if _h is None:
        l = C.CDLL(build.build_xfade_harness())
        l.zlxf_resolve.restype = C.c_int
        l.zlxf_resolve.argtypes = [C.c_double, C.c_int32, C.POINTER(_abi.XfadeRequest)]
        l.zlxf_finish.restype = None
        l.zlxf_finish.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.zlxf_design.restype = None
        l.zlxf_design.argtypes = [C.c_int32, C.c_double, C.c_void_p]
        l.zlxf_extent_floats.restype = C.c_int64
        l.zlxf_extent_floats.argtypes = [C.c_int64, C.c_int32]
        l.zlxf_call.restype = C.c_int32
        l.zlxf_call.argtypes = [C.c_int32] + [C.c_void_p] * 12
        _h = l
    return _h


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def run_call(cases, rate=SR, short=None, lacking=()):
    """one harness call over the cases.  short: {case index: floats the accessor is told the source holds}; lacking: the cases whose
    original lacks ZL_SOUND_FINITE.  Returns (status, results, extents, writes, weights, verdicts, walk)"""
    n = len(cases)
    reqs = (_abi.XfadeRequest * n)(*[_abi.XfadeRequest(0, c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"]) for c in cases])
    srcs = [np.ascontiguousarray(c["x"].T.reshape(-1)) for c in cases]
    floats = [int(harness().zlxf_extent_floats(c["x"].shape[1], c["x"].shape[0])) for c in cases]
    dst = [np.full(k, np.nan, f32) for k in floats]
    writes = [np.zeros(k, np.int32) for k in floats]
    weights = [np.full((max(1, xr.resolve(rate, c["x"].shape[1], c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"]) or 1), 2), np.nan, f32) for c in cases]
    ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    nsrc = (C.c_int64 * n)(*[(short or {}).get(i, s.size) for i, s in enumerate(srcs)])
    length = (C.c_int32 * n)(*[c["x"].shape[1] for c in cases])
    chans = (C.c_int32 * n)(*[c["x"].shape[0] for c in cases])
    rates = (C.c_double * n)(*[rate] * n)
    out = (_abi.Xfade * n)()
    verdicts = (C.c_uint32 * n)(*[1 if i in lacking else 0 for i in range(n)])
    walk = (C.c_int64 * 4)()
    pSrc, pDst, pWrites, pWeights = ptrs(srcs), ptrs(dst), ptrs(writes), ptrs(weights)
    rc = harness().zlxf_call(n, C.addressof(reqs), C.addressof(pSrc), C.addressof(nsrc), C.addressof(length), C.addressof(chans), C.addressof(rates),
                             C.addressof(pDst), C.addressof(pWrites), C.addressof(out), C.addressof(pWeights), C.addressof(verdicts), C.addressof(walk))
    res = [{k: getattr(out[i], k) for k, _ in _abi.Xfade._fields_ if k != "reserved"} for i in range(n)]
    return rc, res, dst, writes, weights, list(verdicts), tuple(walk)


def same_result(got, want):
    return all(got[k] == want[k] for k in xr.RESULT_INTS) and got["correlation"] == want["correlation"] and got["rho"] == want["rho"]


# ---- the header against the restatement ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return xc.grid()


def test_the_grid_covers_what_it_is_meant_to(grid):
    ds, da, at0, last, adjoin = xc.facts(grid)
    assert ds == {(1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 2)} and da == ds
    assert at0 >= 32 and last >= 64 and adjoin >= 16
    applied = [bool(xr.resolve(SR, c["x"].shape[1], c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"])) for c in grid]
    half = applied.index(False, 1)
    assert not applied[0] and not applied[-1] and not applied[half] and not applied[half + 1] and applied.count(False) == 4
    assert {xr.resolve(SR, c["x"].shape[1], c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"]) for c in grid} == {0} | set(xc.FADES)
    assert min(c["x"].shape[1] for c in grid) == 2 and max(c["x"].shape[1] for c in grid) == 70000


def test_harness_matches_the_restatement_on_every_bit(grid):
    rc, res, dst, writes, weights, verdicts, walk = run_call(grid)
    assert rc == len(grid) - 4
    assert walk[3] == 0, "a read outside a clip's own floats"
    groups = 0
    for i, c in enumerate(grid):
        want, ext = xc.want(c)
        assert same_result(res[i], want), (i, res[i], want)
        if not want["applied"]:
            assert not writes[i].any() and np.isnan(dst[i]).all()
            continue
        X = want["fade_frames"]
        assert np.array_equal(weights[i].view(u32), xr.design(X, want["rho"]).view(u32)), i
        assert np.all(writes[i] == 1), (i, np.flatnonzero(writes[i] != 1)[:8])
        assert dst[i].size == ext.size and np.array_equal(dst[i].view(u32), ext.view(u32)), (i, np.flatnonzero(dst[i].view(u32) != ext.view(u32))[:8])
        assert verdicts[i] == 0
        groups += ext.size // 4
    assert walk[2] >= 137 + rc - 1 and walk[0] <= groups and walk[1] < walk[0]


def test_a_call_of_nothing_to_fade_touches_nothing():
    cases = [c for c in xc.grid() if not xr.resolve(SR, c["x"].shape[1], c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"])]
    rc, res, dst, writes, _, _, walk = run_call(cases)
    assert rc == 0 and walk == (0, 0, 0, 0) and all(not w.any() for w in writes)
    assert all(v == 0 for r in res for v in r.values())


def test_the_harness_refuses_a_read_outside_the_buffer_it_was_given():
    """the refusal is the accessor's, not the masks': told that the buffer is one float shorter than the clip whose loop ends at its last
    frame, the same walk is refused the reads of that float -- the measuring pass's, the render's -- and the NaN shows in the output"""
    c = dict(x=xc.clip(np.random.default_rng(4), 1, 300), start_frame=100, stop_frame=300, fade_frames=50, curve=xr.LINEAR)
    rc, _, dst, writes, _, verdicts, walk = run_call([c])
    assert rc == 1 and walk[3] == 0 and verdicts == [0]
    rc, _, dst, writes, _, verdicts, walk = run_call([c], short={0: 299})
    assert rc == 1 and walk[3] == 2 and np.all(writes[0] == 1)
    assert np.isnan(dst[0][299]) and verdicts == [1] and not np.isnan(dst[0][:299]).any()


def test_the_verdict(grid):
    """an inf in A, a NaN in B, two samples near FLT_MAX that overflow at mid-fade under the equal-power curve; a clip whose original
    lacks the flag keeps its word; the restatement says the same"""
    base = xc.clip(np.random.default_rng(6), 2, 400)
    cases = []
    for k in range(5):
        x = base.copy()
        if k == 1:
            x[1, 290] = np.inf
        if k == 2:
            x[0, 90] = np.nan
        if k >= 3:
            x[0, 275] = x[0, 75] = 3e38
        cases.append(dict(x=x, start_frame=100, stop_frame=300, fade_frames=50, curve=xr.LINEAR if k == 4 else xr.EQUAL_POWER))
    rc, res, dst, _, _, verdicts, walk = run_call(cases + [cases[0]], lacking=(5,))
    assert rc == 6 and walk[3] == 0
    assert verdicts == [0, 1, 1, 1, 0, 1]
    for i, c in enumerate(cases):
        want, ext = xc.want(c)
        y = ext[:800].reshape(400, 2).T
        assert xr.all_finite(y, 100, 300, 50) == (verdicts[i] == 0)
        assert np.array_equal(dst[i].view(u32), ext.view(u32))


# ---- resolve --------------------------------------------------------------------------------------------------------------------------
def resolve_both(rate, length, s, e, X, curve):
    """the header's, the library's and the restatement's answer; they agree"""
    outs = []
    for fn in (harness().zlxf_resolve, zlhip().zlhip_xfade_resolve):
        q = _abi.XfadeRequest(7, s, e, X, curve)
        rc = fn(rate, length, C.byref(q))
        assert (q.id, q.start_frame, q.stop_frame, q.curve) == (7, s, e, curve)
        outs.append(q.fade_frames if rc == 0 else None)
        if rc != 0:
            assert q.fade_frames == X
    ref = xr.resolve(rate, length, s, e, X, curve)
    assert outs[0] == outs[1] == ref, (outs, ref)
    return ref


def test_resolve_at_every_limit(built):
    n = 400000
    # the accepting and the refusing side of every limit
    assert resolve_both(SR, n, 100, 300, 100, 0) == 100 and resolve_both(SR, n, 100, 300, 101, 0) is None            # X <= s
    assert resolve_both(SR, n, 300, 400, 100, 0) == 100 and resolve_both(SR, n, 300, 400, 101, 0) is None            # X <= e - s
    assert resolve_both(SR, n, 100000, 300000, 65536, 0) == 65536 and resolve_both(SR, n, 100000, 300000, 65537, 0) is None
    assert resolve_both(SR, n, 100, 300, 1, 0) == 1 and resolve_both(SR, n, 100, 300, -1, 0) is None
    assert resolve_both(SR, n, 100, n, 50, 2) == 50 and resolve_both(SR, n, 100, n + 1, 50, 2) is None                # e <= length
    assert resolve_both(SR, n, 100, 101, 1, 1) == 1 and resolve_both(SR, n, 100, 100, 1, 1) is None                    # s < e
    assert resolve_both(SR, n, -1, 100, 0, 0) is None
    assert resolve_both(SR, n, 100, 300, 50, 3) is None and resolve_both(SR, n, 100, 300, 50, -1) is None
    assert resolve_both(0.0, n, 100, 300, 50, 0) is None and resolve_both(float("nan"), n, 100, 300, 50, 0) is None
    # a loop from frame 0 has no lead-in: nothing to fade, no error
    assert resolve_both(SR, n, 0, 300, 0, 0) == 0
    assert resolve_both(SR, n, 0, 300, 1, 0) is None
    # the default: 20 ms, cut to the lead-in, the loop and the limit
    for rate, frames in ((22050.0, 441), (44100.0, 882), (48000.0, 960), (96000.0, 1920)):
        assert resolve_both(rate, n, 5000, 50000, 0, 0) == frames
        assert resolve_both(rate, n, 300, 50000, 0, 0) == 300 and resolve_both(rate, n, 5000, 5200, 0, 0) == 200
    assert resolve_both(768000.0 * 8, n, 200000, 400000, 0, 0) == 65536
    assert zlhip().zlhip_xfade_resolve(SR, n, None) == _abi.ZLHIP_ERR_INVALID


def test_design_and_finish_match_the_restatement(built):
    for X, rho in ((1, 0.0), (2, 1.0), (5, 0.3), (960, 0.0), (960, 1.0), (960, 0.4711), (65536, 0.033)):
        ref = xr.design(X, rho)
        for fn in (harness().zlxf_design, zlhip().zlhip_xfade_design):
            ab = np.full((X, 2), np.nan, f32)
            fn(X, rho, ab.ctypes.data)
            assert np.array_equal(ab.view(u32), ref.view(u32)), (X, rho)
        assert ref[-1, 0] == 0.0 and ref[-1, 1] == 1.0
        a, b = ref[:, 0].astype(np.float64), ref[:, 1].astype(np.float64)
        assert np.all(np.abs(a * a + b * b + 2.0 * rho * a * b - 1.0) <= 4e-7)
    assert np.array_equal(xr.design(8, 1.0)[:, 0], ((8 - np.arange(1, 9)) / 8.0).astype(f32))       # rho = 1: the linear fade
    ab = np.zeros((4, 2), f32)
    z = zlhip()
    assert z.zlhip_xfade_design(0, 0.5, ab.ctypes.data) == z.zlhip_xfade_design(65537, 0.5, ab.ctypes.data) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_xfade_design(4, -0.1, ab.ctypes.data) == z.zlhip_xfade_design(4, 1.1, ab.ctypes.data) == z.zlhip_xfade_design(4, float("nan"), ab.ctypes.data) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_xfade_design(4, 0.5, None) == _abi.ZLHIP_ERR_INVALID and not ab.any()
    for ints in ((0, 0, 5), (5, 0, 0), (10, 10, 10), (-10, 10, 10), (3, 10, 7), (-2 ** 48, 2 ** 48, 2 ** 48), (123456789, 987654321, 555555555)):
        c, r = C.c_double(9.0), C.c_double(9.0)
        harness().zlxf_finish(*ints, C.byref(c), C.byref(r))
        assert (c.value, r.value) == xr.finish(*ints), ints


# ---- what it does to sound (the restatement alone) ------------------------------------------------------------------------------------
X0, S0 = 960, 6000


def level_change(x, s, e, curve):
    """(mean square of the fade region against the 4 X frames in front of it in dB, rho) of the crossfaded clip"""
    res, y = xr.crossfade(x, SR, s, e, X0, curve)
    return xr.ms_db(y, e - X0, e) - xr.ms_db(y, e - 5 * X0, e - X0), res["rho"]


def test_noise_keeps_its_level_under_auto_and_loses_it_under_linear():
    """20 seeds of stereo white noise.  Observed: AUTO -0.22 .. +0.20 dB with the measured rho at most 0.056; LINEAR -2.05 .. -1.52 dB"""
    auto, lin, rhos = [], [], []
    for seed in range(20):
        x = xr.noise(seed, 2, 24000)
        d, rho = level_change(x, S0, 18000, xr.AUTO)
        auto.append(d); rhos.append(rho)
        lin.append(level_change(x, S0, 18000, xr.LINEAR)[0])
    print("noise: auto %.2f .. %.2f dB, rho <= %.3f, linear %.2f .. %.2f dB" % (min(auto), max(auto), max(rhos), min(lin), max(lin)))
    assert all(abs(d) <= 0.5 for d in auto), auto
    assert all(d < -1.2 for d in lin), lin


@pytest.mark.parametrize("period,e", [(100.0, 18000), (218.4, S0 + 1092 * 11)])
def test_a_tone_looped_over_whole_periods_keeps_its_level_under_auto_and_gains_under_equal_power(period, e):
    """observed: AUTO +0.02 / -0.09 dB with rho = 1; EQUAL_POWER +1.97 / +1.90 dB"""
    x = xr.tone(period, 2, 24000)
    d, rho = level_change(x, S0, e, xr.AUTO)
    up = level_change(x, S0, e, xr.EQUAL_POWER)[0]
    print("tone %.1f: auto %.2f dB, rho %.4f, equal power %.2f dB" % (period, d, rho, up))
    assert abs(d) <= 0.5 and rho > 0.999
    assert up > 1.5


def test_tone_plus_noise_keeps_its_level_under_auto_alone():
    """a mono tone plus noise at three ratios (rho about 0.9, 0.5, 0.2: the tone's share of the power).  Observed: rho 0.90, 0.51,
    0.17; AUTO -0.06, +0.16, -0.10 dB; LINEAR misses by up to 1.56 dB, EQUAL_POWER by up to 1.75 dB"""
    worst = 0.0
    for k, (noise_level, about) in enumerate(((0.079, 0.9), (0.237, 0.5), (0.474, 0.2))):
        x = (xr.tone(100.0, 1, 24000) + xr.noise(100 + k, 1, 24000, noise_level)).astype(f32)
        d, rho = level_change(x, S0, 18000, xr.AUTO)
        fixed = [level_change(x, S0, 18000, c)[0] for c in (xr.LINEAR, xr.EQUAL_POWER)]
        print("tone + noise: rho %.3f, auto %.2f dB, linear %.2f dB, equal power %.2f dB" % (rho, d, fixed[0], fixed[1]))
        assert abs(rho - about) <= 0.1, rho
        assert abs(d) <= 0.5, d
        worst = max(worst, max(abs(v) for v in fixed))
    assert worst > 1.0, worst


def test_a_decaying_pad_wraps_without_a_step():
    """e^(-t / 40000), period 218.4, looped over 220 periods: the wrap step |y[s] - y[e - 1]| falls from 0.078 to 0.0036 (level 0.3, the loop
    from frame 4000), where the median step of the samples around the start is 0.0026; asserted: no more than 3 times that median"""
    n, s = 56000, 4000
    e = s + int(round(218.4 * 220))
    x = xr.tone(218.4, 1, n, level=0.3, decay=40000.0)
    res, y = xr.crossfade(x, SR, s, e, X0, xr.AUTO)
    before = abs(float(x[0, s]) - float(x[0, e - 1]))
    after = abs(float(y[0, s]) - float(y[0, e - 1]))
    around = np.abs(np.diff(y[0, s - 50:s + 50].astype(np.float64)))
    median = float(np.median(around))
    print("pad: wrap step %.4f -> %.4f, median step around the start %.4f, rho %.3f" % (before, after, median, res["rho"]))
    assert before > 10 * after
    assert after <= 3 * median


@pytest.mark.parametrize("curve", [xr.AUTO, xr.LINEAR, xr.EQUAL_POWER])
def test_the_loops_last_frame_becomes_the_frame_in_front_of_its_start(curve):
    """y[e - 1] == x[s - 1] bit for bit: a = 0 and b = 1 there, and 0 x + 1 x' is x' for finite x and x' other than -0 (which the sum with
    the +0 product returns as +0): plain noise"""
    for ch, seed in ((1, 1), (2, 2)):
        x = np.random.default_rng(seed).uniform(-1.0, 1.0, (ch, 5000)).astype(f32)
        for s, e, X in ((1000, 4000, 0), (1, 2, 1), (77, 4999, 77), (960, 1920, 960)):
            _, y = xr.crossfade(x, SR, s, e, X, curve)
            assert np.array_equal(y[:, e - 1].view(u32), x[:, s - 1].view(u32)), (ch, s, e, X)
            Xr = xr.resolve(SR, 5000, s, e, X, curve)
            keep = np.ones(5000, bool); keep[e - Xr:e] = False
            assert np.array_equal(y[:, keep].view(u32), x[:, keep].view(u32))


# ---- the C-ABI without a GPU, the layouts, the kernels' resources ---------------------------------------------------------------------
def test_without_a_gpu_the_calls_answer_invalid(built):
    l = zlhip()
    q = _abi.XfadeRequest(0, 100, 300, 0, 0)
    out = _abi.Xfade()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert l.zlhip_sound_loop_crossfade(None, C.byref(q), C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_loop_crossfade_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_loop_crossfade_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_xfade_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    lz = C.CDLL(build.build_engine())
    for name, args in (("libzl_hotpath_clip_crossfade_loop", [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
                       ("libzl_hotpath_clips_seal_loops", [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p])):
        getattr(lz, name).restype = C.c_int
        getattr(lz, name).argtypes = args
    n = C.c_int(-7)
    assert lz.libzl_hotpath_clip_crossfade_loop(None, 0.0, 0, C.byref(n), None) == _abi.ZLHIP_ERR_INVALID and n.value == -7
    assert lz.libzl_hotpath_clips_seal_loops(None, 2, 0.0, 0.0, 0.0, 0, None) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_abi_version() == 3


def test_xfade_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_xfade_request", _abi.XfadeRequest), ("zlhip_xfade", _abi.Xfade))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    body += 'printf("%d %d %d ",ZLHIP_XFADE_AUTO,ZLHIP_XFADE_LINEAR,ZLHIP_XFADE_EQUAL_POWER);'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-3] == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:2] == [20, 64] and got[-3:] == [_abi.XFADE_AUTO, _abi.XFADE_LINEAR, _abi.XFADE_EQUAL_POWER] == [xr.AUTO, xr.LINEAR, xr.EQUAL_POWER]
    assert got[2:-3] == list(range(0, 20, 4)) + list(range(0, 24, 4)) + [24, 32, 40, 48, 56]


def test_xfade_kernels_have_no_scratch_memory_and_the_render_kernel_no_lds(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_xfade_kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resources of zl_xfade.hip's kernels"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    measure = [r for n, r in rows.items() if "zl_k_xfade_measure" in n]
    render = [r for n, r in rows.items() if "zl_k_xfade_render" in n]
    assert len(measure) == 1 and len(render) == 1 and len(rows) == 2, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    assert render[0]["lds"] == 0 and render[0]["vgprs"] <= 32 and render[0]["waves"] >= 8, rows
    assert measure[0]["lds"] == 2 * 4 * 1024 + 3 * 4 * 8, rows        # two chunks of int32, twelve words for the reduction


# ---- the walk under the sanitizers ------------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/xfade_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with AddressSanitizer
    and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment loads
    in front of it."""
    exe = str(tmp_path / "xfade_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "xfade_check.cpp"), "-o", exe])
    for args in (["1", "40"], ["2", "40"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "xfade check ok" in rc.stdout
