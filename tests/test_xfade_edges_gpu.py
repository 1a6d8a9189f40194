"""Loop crossfade, GPU tier, the engine around the call: what it refuses (with `out` untouched and every clip as it was), an arena that
cannot hold the call, the buffers' first allocation, a grown arena, the resident real-time kernel, the crossfade next to the rate
conversion and the re-render, the process's resources, the engine group and the libzl-named layer.  Extents and results are compared as
tests/test_xfade_gpu.py compares them (tests/xfade_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_ref as lr
import xfade_cases as xc
import xfade_ref as xr
from xfade_cases import SR, check_call, dirty, mismatch, upload

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def case(x, s, e, X=0, curve=xr.AUTO):
    return dict(x=x, start_frame=s, stop_frame=e, fade_frames=X, curve=curve)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_every_clip_and_out_as_they_were(built):
    from libzl_amd import _abi
    INV, CAP, STATE = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY, _abi.ZLHIP_ERR_STATE
    rng = np.random.default_rng(41)
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        a, b = xc.clip(rng, 2, 4000), xc.clip(rng, 1, 5000)
        big = xc.clip(rng, 2, 70000)                               # 560 KB: a second extent of it does not fit the arena (1 MiB)
        ia, ib, ibig = upload(s, a), upload(s, b), upload(s, big)
        exts = [s.clip_extent(i) for i in (ia, ib, ibig)]
        R = _abi.XfadeRequest

        def call(reqs, count=None):
            arr = (R * max(1, len(reqs)))(*[R(*r) for r in reqs])
            out = (_abi.Xfade * max(1, len(reqs)))()
            C.memset(out, 0x5A, C.sizeof(out))
            rc = lib.zlhip_sound_loop_crossfade_batch(e, arr, len(reqs) if count is None else count, out)
            return rc, bytes(out) == b"\x5a" * C.sizeof(out)

        def unchanged():
            return all(same(s.clip_extent(i), x) for i, x in zip((ia, ib, ibig), exts))

        good = (ia, 1000, 3000, 0, 0)
        assert s.clip_loop_crossfade(ib, 0, 3000)["applied"] == 0  # (nothing to fade: no buffers either)
        mem = s.memory_bytes()
        bad = [(ia, 1000, 4001, 0, 0), (ia, 1000, 1000, 0, 0), (ia, -1, 3000, 0, 0), (ia, 1000, 3000, 1001, 0), (ia, 1500, 2000, 501, 0), (ia, 1000, 3000, -1, 0),
               (ia, 1000, 3000, 10, 3), (ia, 0, 3000, 1, 0), (31, 1000, 3000, 0, 0), (-1, 1000, 3000, 0, 0), (99, 1000, 3000, 0, 0)]
        for r in bad:
            assert call([r]) == (INV, True), r
            assert call([(ib, 2000, 4000, 0, 0), r]) == (INV, True), r    # one bad request fails the call
        assert b"sound_loop_crossfade" in lib.zlhip_last_error(e)
        assert call([good, good]) == (INV, True) and call([good, (ib, 2000, 4000, 0, 0), (ia, 500, 900, 0, 0)]) == (INV, True)       # duplicates
        assert call([good], count=-1) == (INV, True) and call([], count=0) == (0, True)
        assert lib.zlhip_sound_loop_crossfade_batch(e, None, 1, None) == INV and lib.zlhip_sound_loop_crossfade(None, None, None) == INV
        assert unchanged() and s.memory_bytes() == mem
        # a clip that plays a re-render
        s.rerender_clip(ib, gain_db=-6.0)
        bre, mem = s.clip_extent(ib), s.memory_bytes()
        assert call([good, (ib, 2000, 4000, 0, 0)]) == (STATE, True) and call([(ib, 2000, 4000, 0, 0)]) == (STATE, True)
        assert same(s.clip_extent(ib), bre) and same(s.clip_extent(ia), exts[0]) and s.memory_bytes() == mem
        assert call([(ib, 0, 4000, 0, 0)])[0] == 0                 # nothing to fade: not judged
        s.rerender_clip(ib)
        assert unchanged()
        # an arena that cannot hold the call: the small clip's extent fits, the big one's does not -- neither is faded
        mem = s.memory_bytes()
        assert call([good, (ibig, 20000, 60000, 0, 0)]) == (CAP, True)
        assert unchanged() and s.memory_bytes() == mem
        # after the errors the call still works
        bad_, outs = check_call(s, [case(a, 1000, 3000), case(b, 2000, 4000, 100, xr.LINEAR)], [ia, ib])
        assert not bad_, bad_
        assert same(s.clip_extent(ibig), exts[2])


# ---- the buffers ----------------------------------------------------------------------------------------------------------------------
def test_an_engine_that_never_asks_allocates_nothing(built):
    with make() as s:
        rng = np.random.default_rng(42)
        xs = [xc.clip(rng, 2, 6000) for _ in range(3)]
        ids = [upload(s, x) for x in xs]
        total0, _ = s.memory_bytes()
        s.clip_loudness(ids[0])
        total1, _ = s.memory_bytes()
        assert total1 > total0
        assert s.clip_loop_crossfade(ids[0], 0, 3000)["applied"] == 0
        assert s.memory_bytes()[0] == total1                       # nothing to fade: no buffers
        assert s.clip_loop_crossfade(ids[0], 2000, 5000)["applied"] == 1
        total2, _ = s.memory_bytes()
        assert total2 > total1
        s.clip_loop_crossfade_batch([(ids[1], 1000, 3000, 500), (ids[2], 700, 1400, 0, 2)]); s.clip_loop_crossfade(ids[0], 100, 200, 0, 1)       # fit the first call's buffers
        assert s.memory_bytes()[0] == total2


def test_a_clip_in_a_grown_arena(built):
    arena = 1 << 20
    with make(max_sounds=16, sound_arena_bytes=arena) as s:
        rng = np.random.default_rng(43)
        xs = [xc.clip(rng, 1 + i % 2, 60000 + 1001 * i) for i in range(6)]
        ids = [upload(s, x) for x in xs]
        assert s.memory_bytes()[1] >= 2 * arena                    # the arena grew
        cases = [case(x, 960 + 7 * i, x.shape[1] - (0 if i % 2 else 13), 0 if i % 3 else 960, i % 3) for i, x in enumerate(xs)]
        bad, outs = check_call(s, cases, ids)                      # (the new extents grow it further: sources and destinations in different segments)
        assert not bad, bad
        assert all(o["applied"] == 1 for o in outs)


def test_the_resources_are_balanced_after_destroy(built):
    from libzl_amd.engine import live_resources
    before = live_resources()
    with make() as s:
        s.set_profiling(True)
        x = xc.clip(np.random.default_rng(44), 2, 5000)
        cid = upload(s, x)
        got = s.clip_loop_crossfade(cid, 1000, 4000)
        assert mismatch(s, cid, case(x, 1000, 4000), got) is None
        m, r = s.xfade_timings()
        assert m > 0.0 and r > 0.0
        assert live_resources() != before
    assert live_resources() == before


# ---- next to the resident real-time kernel ----------------------------------------------------------------------------------------------
@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_three_clips_in_one_call_between_real_time_cycles_cost_one_restart(built, rt_env):
    from scenario import engine_cmd, play_cmd
    from libzl_amd.engine import synthetic_clocks
    rng = np.random.default_rng(45)
    with make() as s:
        xs = [xc.clip(rng, 2, 3000) for _ in range(3)]
        ids = [upload(s, x) for x in xs]
        clocks = synthetic_clocks(8, 256, SR)
        starts = []
        for k in range(8):
            if k == 4:
                cases = [case(x, 1000, 2500, 300 + i) for i, x in enumerate(xs)]
                bad, _ = check_call(s, cases, ids)                  # three clips, one call
                assert not bad, bad
                p = s.default_clip_params(3000 / SR)
                p.length_seconds = 0.015625
                p.length_in_beats = 0.04
                s.set_clip_params(ids[0], p)
                s.handle_clip_command(engine_cmd(**play_cmd(ids[0], midi_channel=-2, loop=True, note=60, volume=0.8)), 0)
            L, R = s.process(256, clocks[k])
            starts.append(s.rt_stats()[0])
            if k == 4:
                first = np.stack([L[0], R[0]])
        assert starts == [1, 1, 1, 1, 2, 2, 2, 2], starts
        assert s.rt_stats() == (2, 8) and len(np.unique(first[0])) > 200


# ---- next to the rate conversion and the re-render --------------------------------------------------------------------------------------
def test_a_crossfade_after_a_rate_conversion_and_a_gain_after_the_crossfade(built):
    """the conversion leaves the data on the device only: the crossfade works on the converted frames (read back before it) at the new
    rate's default; a gain re-render afterwards starts from the faded data and keeps the seam; a pitch render is refused nothing, but the
    crossfade of a clip that plays a re-render is"""
    from libzl_amd import ZlHipError
    rng = np.random.default_rng(46)
    with make() as s:
        x = xc.clip(rng, 2, 8820)
        cid = upload(s, x, 44100.0)
        c0 = case(x, 2000, 8000)
        got = s.clip_loop_crossfade(cid, 2000, 8000)
        assert got["fade_frames"] == 882 and mismatch(s, cid, c0, got, rate=44100.0) is None
        s.convert_clips([cid], SR)
        L, R = s.read_clip(cid)
        now = np.stack([L, R])
        assert s.clip_info(cid)["sample_rate"] == SR and abs(now.shape[1] - 9600) <= 1
        c1 = case(now, 3000, 9000)
        got = s.clip_loop_crossfade(cid, 3000, 9000)
        assert got["fade_frames"] == 960 and mismatch(s, cid, c1, got) is None
        _, faded = xr.crossfade(now, SR, 3000, 9000, 0, xr.AUTO, ints=(got["sab"], got["saa"], got["sbb"]))
        s.rerender_clip(cid, gain_db=-6.0)
        g = f32(10.0 ** (-6.0 / 20.0))
        L, R = s.read_clip(cid)
        assert np.allclose(np.stack([L, R]), faded * g, rtol=1e-6, atol=1e-9)
        with pytest.raises(ZlHipError, match=r"\(-5\)"):
            s.clip_loop_crossfade(cid, 3000, 9000)
        s.rerender_clip(cid)                                       # the identity: the crossfaded original plays again
        L, R = s.read_clip(cid)
        assert same(np.stack([L, R]), faded)


# ---- the group, the libzl-named layer ---------------------------------------------------------------------------------------------------
def test_group_crossfades_on_every_member(built):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    rng = np.random.default_rng(47)
    with SamplerSynthGroup([0, 0], 4, 8, max_frames=256, max_batch_blocks=8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        cases = [case(xc.clip(rng, 2, 3000), 1000, 2900, 0, xr.AUTO), case(xc.clip(rng, 1, 700), 257, 700, 257, xr.EQUAL_POWER), case(xc.clip(rng, 2, 300), 0, 200)]
        ids = [upload(g, c["x"]) for c in cases]
        outs = g.clip_loop_crossfade_batch([(cid, c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"]) for cid, c in zip(ids, cases)])
        assert [o["applied"] for o in outs] == [1, 1, 0]
        for r in range(2):
            for cid, c, got in zip(ids, cases, outs):
                n = C.c_size_t(0)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, None, 0, C.byref(n)) == 0
                ext = np.empty(n.value, f32)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, ext.ctypes.data, ext.size, None) == 0
                if got["applied"]:
                    assert mismatch(g, cid, c, got, extent=ext) is None, (r, cid)
                else:
                    assert same(ext[:c["x"].size], np.ascontiguousarray(c["x"].T).reshape(-1))
        assert g.clip_loop_crossfade(ids[1], 257, 700, 100, xr.LINEAR)["rho"] == 1.0
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_loop_crossfade_batch([(ids[0], 1000, 2900), (ids[0], 1000, 2900)])


def test_libzl_clip_crossfade_loop_and_clips_seal_loops(built, tmp_path):
    """libzl_hotpath_clip_crossfade_loop on a loaded clip: the frames are the ones the voice derives from the clip's seconds, the data
    equals the restatement's; a re-rendered clip is refused; libzl_hotpath_clips_seal_loops on a bank of 4 makes two device calls (one
    loop search, one crossfade: the crossfade's buffers are the only ones that may grow) and reports bit 0 = snapped, bit 1 = faded"""
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        e = zl.libzl_hotpath_engine()
        tones = [lr.tone(218.4, 1, 24000, seed=51), lr.tone(133.7, 1, 24000, seed=52), lr.tone(97.3, 1, 24000, seed=53), lr.tone(171.9, 1, 24000, seed=54), lr.tone(150.0, 1, 24000, seed=55)]
        clips = []
        for k, src in enumerate(tones):
            path = str(tmp_path / ("t%d.wav" % k)).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, None, src.shape[1], SR, 32) == 0
            clips.append(zl.ClipAudioSource_new(path, False))
            assert clips[-1]
            zl.ClipAudioSource_setStartPosition(clips[-1], C.c_float(0.1))
            zl.ClipAudioSource_setLength(clips[-1], C.c_float(0.25), 120)      # 0.125 s: the loop is about [4800, 10800)

        def params(clip):
            p = _abi.ClipParams()
            assert zl.libzl_hotpath_clip_params(clip, C.byref(p)) == 0
            return p

        def frames(clip):
            p = params(clip)
            return lr.frame_of(p.start_position_seconds, SR), lr.stop_of(p.start_position_seconds, p.length_seconds, SR)

        def extent(clip):
            cid = zl.ClipAudioSource_engineClip(clip)
            n = C.c_size_t(0)
            assert zl.zlhip_debug_sound_extent(e, cid, None, 0, C.byref(n)) == 0
            ext = np.empty(n.value, f32)
            assert zl.zlhip_debug_sound_extent(e, cid, ext.ctypes.data, ext.size, None) == 0
            return ext

        # one clip
        a = clips[4]
        s0, e0 = frames(a)
        p0 = bytes(params(a))
        n, corr = C.c_int(-7), C.c_double(-7.0)
        assert zl.libzl_hotpath_clip_crossfade_loop(None, C.c_float(0.0), 0, C.byref(n), C.byref(corr)) < 0
        assert zl.libzl_hotpath_clip_crossfade_loop(a, C.c_float(-1.0), 0, C.byref(n), C.byref(corr)) < 0
        assert zl.libzl_hotpath_clip_crossfade_loop(a, C.c_float(0.0), 3, C.byref(n), C.byref(corr)) < 0 and (n.value, corr.value) == (-7, -7.0)
        assert zl.libzl_hotpath_clip_crossfade_loop(a, C.c_float(10.0), xr.AUTO, C.byref(n), C.byref(corr)) == 1
        assert n.value == 480 and bytes(params(a)) == p0
        res, y = xr.crossfade(tones[4], SR, s0, e0, 480, xr.AUTO)
        assert corr.value == res["correlation"]
        assert same(extent(a), xr.extent(y))
        # a clip that plays a re-render is refused: crossfade first, level afterwards
        zl.ClipAudioSource_setGain(a, C.c_float(-3.0))
        info = _abi.SoundInfo()
        assert zl.zlhip_sound_info_get(e, zl.ClipAudioSource_engineClip(a), C.byref(info)) == 0 and info.rendered == 1
        assert zl.libzl_hotpath_clip_crossfade_loop(a, C.c_float(10.0), xr.AUTO, None, None) == _abi.ZLHIP_ERR_STATE
        # a bank of 4 (and a NULL): snapped and faded
        bank = clips[:4]
        before = [frames(c) for c in bank]
        wants = [lr.loop(t, SR, s, e_) for t, (s, e_) in zip(tones, before)]
        assert all(w["found"] == 1 and w["improvement_db"] >= 20.0 for w in wants)
        arr = (C.c_void_p * 5)(bank[0], bank[1], None, bank[2], bank[3])
        results = (C.c_int * 5)(-1, -1, -1, -1, -1)
        assert zl.libzl_hotpath_clips_seal_loops(arr, 5, C.c_float(0.0), C.c_float(20.0), C.c_float(0.0), xr.AUTO, results) == 4
        assert list(results) == [3, 3, 0, 3, 3]
        for c, t, w in zip(bank, tones, wants):
            assert frames(c) == (w["start_frame"], w["stop_frame"])
            _, y = xr.crossfade(t, SR, w["start_frame"], w["stop_frame"], 0, xr.AUTO)
            assert same(extent(c), xr.extent(y))
        # again with a bar no seam passes: nothing moves, every loop is faded once more (bit 1 alone)
        assert zl.libzl_hotpath_clips_seal_loops(arr, 5, C.c_float(0.0), C.c_float(200.0), C.c_float(5.0), xr.LINEAR, results) == 4
        assert list(results) == [2, 2, 0, 2, 2]
        assert zl.libzl_hotpath_clips_seal_loops((C.c_void_p * 2)(bank[0], bank[0]), 2, C.c_float(0.0), C.c_float(20.0), C.c_float(0.0), 0, None) < 0
        assert zl.libzl_hotpath_clips_seal_loops(arr, 5, C.c_float(0.0), C.c_float(20.0), C.c_float(0.0), 7, None) < 0
        for clip in clips:
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
