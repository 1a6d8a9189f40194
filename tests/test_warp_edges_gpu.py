"""Warp, GPU tier, the engine around the call: what it refuses (with `out` untouched, every clip and zlhip_memory_bytes as they were), an
arena that cannot hold the call, the buffers' first allocation, a grown arena, a re-render after a warp, the process's resources, the
engine group and the libzl-named layer.  Extents, offsets and results are compared as tests/test_warp_gpu.py compares them
(tests/warp_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import warp_cases as wc
import warp_ref as wr
from warp_cases import check_call, mismatch, upload

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
R1 = 1000.0


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def test_errors_leave_every_clip_out_and_the_memory_as_they_were(built):
    from libzl_amd import _abi
    INV, CAP, STATE = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY, _abi.ZLHIP_ERR_STATE
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        a, b = wc.clip(1, 2, 400), wc.clip(2, 1, 500)
        big = wc.clip(3, 2, 70000)                                 # 560 KB: a second extent of it does not fit the arena (1 MiB)
        ia, ib, ibig = upload(s, a, R1), upload(s, b, R1), upload(s, big, R1)
        ids = (ia, ib, ibig)
        exts = [s.clip_extent(i) for i in ids]

        def call(reqs, count=None):
            keep = [np.ascontiguousarray(np.asarray(an, np.int32).reshape(-1, 2)) for _, an in reqs]
            arr = (_abi.WarpRequest * max(1, len(reqs)))(*[_abi.WarpRequest(cid, k.shape[0], C.cast(k.ctypes.data, C.POINTER(_abi.WarpAnchor))) for (cid, _), k in zip(reqs, keep)])
            out = (_abi.Warp * max(1, len(reqs)))()
            C.memset(out, 0x5A, C.sizeof(out))
            rc = lib.zlhip_sound_warp_batch(e, arr, len(reqs) if count is None else count, out)
            return rc, bytes(out) == b"\x5a" * C.sizeof(out)

        def unchanged():
            return all(wc.same_bits(s.clip_extent(i), x) for i, x in zip(ids, exts))

        good = (ia, [(0, 0), (200, 260), (400, 440)])
        other = (ib, [(0, 0), (500, 600)])
        assert s.clip_warp(ib, [(0, 0), (250, 250), (500, 500)])["applied"] == 0     # (the identity: no buffers either)
        mem = s.memory_bytes()
        bad = [(ia, [(0, 0), (400, 99)]), (ia, [(0, 0), (100, 401), (400, 800)]), (ia, [(0, 0), (92, 200), (400, 508)]), (ia, [(0, 0), (399, 500)]),
               (ia, [(0, 1), (400, 500)]), (ia, [(0, 0), (200, 250), (200, 260), (400, 500)]), (ia, [(0, 0), (200, 250), (300, 250), (400, 500)]),
               (ia, [(0, 0)]), (31, good[1]), (-1, good[1]), (99, good[1])]
        for r in bad:
            assert call([r]) == (INV, True), r
            assert call([other, r]) == (INV, True), r              # one bad request fails the call
        assert b"sound_warp" in lib.zlhip_last_error(e)
        assert call([good, good]) == (INV, True) and call([good, other, (ia, [(0, 0), (400, 500)])]) == (INV, True)       # duplicates
        assert call([good], count=-1) == (INV, True) and call([], count=0) == (0, True)
        assert lib.zlhip_sound_warp_batch(e, None, 1, None) == INV and lib.zlhip_sound_warp(None, None, None) == INV
        q = _abi.WarpRequest(ia, 2, None)
        assert lib.zlhip_sound_warp(e, C.byref(q), C.byref(_abi.Warp())) == INV
        assert unchanged() and s.memory_bytes() == mem
        # a clip that plays a re-render
        s.rerender_clip(ib, gain_db=-6.0)
        bre, mem = s.clip_extent(ib), s.memory_bytes()
        assert call([good, other]) == (STATE, True) and call([other]) == (STATE, True)
        assert wc.same_bits(s.clip_extent(ib), bre) and wc.same_bits(s.clip_extent(ia), exts[0]) and s.memory_bytes() == mem
        assert call([(ib, [(0, 0), (500, 500)])])[0] == 0          # the identity: not judged
        s.rerender_clip(ib)
        assert unchanged()
        # an arena that cannot hold the call: the small clip's extent fits, the big one's does not -- neither is warped
        mem = s.memory_bytes()
        assert call([good, (ibig, [(0, 0), (70000, 71000)])]) == (CAP, True)
        assert unchanged() and s.memory_bytes() == mem
        assert s.warp_offsets(ia).size == 0
        # after the errors the call still works
        cases = [dict(tag="after-a", rate=R1, x=a, anchors=good[1]), dict(tag="after-b", rate=R1, x=b, anchors=other[1])]
        bad_, outs = check_call(s, cases, [ia, ib])
        assert not bad_, bad_
        assert wc.same_bits(s.clip_extent(ibig), exts[2])
        with pytest.raises(Exception):
            s.warp_offsets(31)


def test_an_engine_that_never_asks_allocates_nothing(built):
    with make() as s:
        xs = [wc.clip(40 + i, 2, 600) for i in range(3)]
        ids = [upload(s, x, R1) for x in xs]
        total0, _ = s.memory_bytes()
        s.clip_loudness(ids[0])
        total1, _ = s.memory_bytes()
        assert total1 > total0
        assert s.clip_warp(ids[0], [(0, 0), (300, 300), (600, 600)])["applied"] == 0
        assert s.memory_bytes()[0] == total1                       # the identity: no buffers
        assert s.clip_warp(ids[0], [(0, 0), (300, 360), (600, 640)])["applied"] == 1
        total2, _ = s.memory_bytes()
        assert total2 > total1
        s.clip_warp_batch([(ids[1], [(0, 0), (600, 500)]), (ids[2], [(0, 0), (200, 260), (400, 460), (600, 600)])])      # fits the first call's buffers
        s.clip_warp(ids[0], [(0, 0), (640, 700)])
        assert s.memory_bytes()[0] == total2


def test_clips_in_a_grown_arena(built):
    arena = 1 << 20
    with make(max_sounds=16, sound_arena_bytes=arena) as s:
        cases = [wc.case("grown%d" % i, 8000, 1 + i % 2, [(30000 + 501 * i, 33000), (30000, 28000 + 77 * i)], seed=50 + i) for i in range(6)]
        ids = [upload(s, c["x"], c["rate"]) for c in cases]
        assert s.memory_bytes()[1] >= 2 * arena                    # the arena grew
        bad, outs = check_call(s, cases, ids)                      # (the new extents grow it further: sources and destinations in different segments)
        assert not bad, bad
        assert all(o["applied"] == 1 for o in outs)


def test_the_resources_are_balanced_after_destroy_and_the_timings_are_there(built):
    from libzl_amd.engine import live_resources
    before = live_resources()
    with make() as s:
        s.set_profiling(True)
        c = wc.case("timed", 1000, 2, [(300, 360), (300, 280)])
        cid = upload(s, c["x"], c["rate"])
        got = s.clip_warp(cid, c["anchors"])
        assert mismatch(s, cid, c, got) is None
        a, b = s.warp_timings()
        assert a > 0.0 and b > 0.0
        assert live_resources() != before
    assert live_resources() == before


def test_a_rerender_after_a_warp_starts_from_the_warped_data(built):
    """warp first, then tune and level: the re-render equals the restatement's re-render (tests/stretch_ref.py) of the restatement's
    warp; the identity re-render plays the warped original again; a warp under a re-render is refused"""
    import stretch_ref
    from libzl_amd import ZlHipError
    c = wc.case("then-rerender", 8000, 2, [(3000, 3400), (3000, 2700)], seed=61)
    y = wc.want(c)[1]
    with make() as s:
        cid = upload(s, c["x"], c["rate"])
        got = s.clip_warp(cid, c["anchors"])
        assert mismatch(s, cid, c, got) is None
        s.rerender_clip(cid, gain_db=-3.0, pitch=2.0, speed=1.25)
        ref, roffs = stretch_ref.render(y, 8000.0, -3.0, 2.0, 1.25)
        L, R = s.read_clip(cid)
        assert wc.same_bits(np.stack([L, R]), ref) and np.array_equal(s.rerender_offsets(cid), roffs)
        with pytest.raises(ZlHipError, match=r"\(-5\)"):
            s.clip_warp(cid, [(0, 0), (y.shape[1], y.shape[1] + 500)])
        s.rerender_clip(cid)
        L, R = s.read_clip(cid)
        assert wc.same_bits(np.stack([L, R]), y)
        # and a second warp, of the warped data
        c2 = dict(tag="warp-twice", rate=8000.0, x=np.array(y), anchors=[(0, 0), (y.shape[1], y.shape[1] - 400)])
        got = s.clip_warp(cid, c2["anchors"])
        assert mismatch(s, cid, c2, got) is None


def test_group_warps_on_every_member(built):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    with SamplerSynthGroup([0, 0], 4, 8, max_frames=256, max_batch_blocks=8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        cases = [wc.case("group-a", 1000, 2, [(100, 130), (50, 50), (120, 90)]), wc.case("group-b", 1000, 1, [(240, 60)]), wc.case("group-c", 1000, 2, [(64, 64)])]
        ids = [upload(g, c["x"], c["rate"]) for c in cases]
        outs = g.clip_warp_batch([(cid, c["anchors"]) for cid, c in zip(ids, cases)])
        assert [o["applied"] for o in outs] == [1, 1, 0]
        for r in range(2):
            for cid, c, got in zip(ids, cases, outs):
                n = C.c_size_t(0)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, None, 0, C.byref(n)) == 0
                ext = np.empty(n.value, f32)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, ext.ctypes.data, ext.size, None) == 0
                k = C.c_int32(0)
                assert g._lib.zlhip_debug_warp_offsets(g.member(r), cid, None, 0, C.byref(k)) == 0
                offs = np.zeros(max(1, k.value), np.int32)
                assert g._lib.zlhip_debug_warp_offsets(g.member(r), cid, offs.ctypes.data, offs.size, C.byref(k)) == 0
                assert mismatch(g, cid, c, got, extent=ext, offsets=offs[:k.value] if got["applied"] else None) is None, (r, cid)
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_warp_batch([(ids[0], cases[0]["anchors"]), (ids[0], cases[0]["anchors"])])


def test_libzl_clip_warp_to_grid(built, tmp_path):
    """libzl_hotpath_clip_warp_to_grid on a jittered click loop at the session's tempo (120 bpm, the scheduler's default): it returns 1,
    the clip's data equals the restatement's warp by the restatement's plan over the restatement's onsets, the onsets found afterwards
    by zlhip_sound_onsets equal the restatement's onsets of that data, and new_length_frames is right; a clip that plays a re-render is
    refused; strength 0 at the session's tempo is nothing to do, and so is a clip without a tempo where the tempo is to be detected"""
    import onset_ref
    from libzl_amd import _abi, libzl
    SR = 48000.0
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        lib = _abi.load()
        eng = C.c_void_p(zl.libzl_hotpath_engine())
        rng = np.random.default_rng(71)
        length = 96000                                             # 2 s: four beats at 120 bpm, a hit every half beat, up to 25 ms off
        x = rng.uniform(-0.002, 0.002, (1, length)).astype(f32)
        for k, j in zip(range(1, 8), (700, -900, 1100, -400, 1200, -1000, 600)):
            t = k * 12000 + j
            x[0, t:t + 400] += (0.8 * np.exp(-np.arange(400) / 60.0) * np.sin(2 * np.pi * np.arange(400) / 31.0)).astype(f32)
        path = str(tmp_path / "clicks.wav").encode()
        assert zl.libzl_wav_write(path, x[0].ctypes.data, None, length, SR, 32) == 0
        c = zl.ClipAudioSource_new(path, False)
        assert c
        cid = zl.ClipAudioSource_engineClip(c)

        def played():
            n = C.c_int32(0)
            assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(n)) >= 0
            L = np.empty(n.value, f32)
            assert lib.zlhip_sound_read(eng, cid, L.ctypes.data, None, n.value, C.byref(n)) >= 1
            return L[None, :]

        def device_onsets():
            q = _abi.OnsetRequest(cid, 0, played().shape[1], 0, 0, 0, 0, 0)
            out = (_abi.Onset * 128)()
            n = C.c_int32(0)
            assert lib.zlhip_sound_onsets(eng, C.byref(q), out, 128, C.byref(n)) == 0
            return [(out[i].frame, out[i].strength) for i in range(n.value)]

        d = onset_ref.resolve(SR)
        on = onset_ref.onsets(x, 0, None, d["hop"], d["gate"], d["threshold"], d["min_gap"], d["max_onsets"])[0]
        assert [tuple(int(v) for v in r) for r in on] == device_onsets() and len(on) >= 5
        frames = sorted(int(v) for v in on[:, 0])
        moved, newlen = C.c_int(-7), C.c_int(-7)
        fn = zl.libzl_hotpath_clip_warp_to_grid
        assert fn(None, C.c_float(120.0), 2, C.c_float(1.0), C.byref(moved), C.byref(newlen)) < 0
        assert fn(c, C.c_float(120.0), 0, C.c_float(1.0), C.byref(moved), C.byref(newlen)) < 0
        assert fn(c, C.c_float(120.0), 2, C.c_float(1.5), C.byref(moved), C.byref(newlen)) < 0 and (moved.value, newlen.value) == (-7, -7)
        assert fn(c, C.c_float(120.0), 2, C.c_float(0.0), C.byref(moved), C.byref(newlen)) == 0 and (moved.value, newlen.value) == (0, length)
        assert wc.same_bits(played(), x)
        anchors, dropped = wr.plan(SR, length, frames, 120.0, 120.0, 2, 1.0, 0)
        summary, y, offs, _ = wr.warp(x, SR, anchors)
        assert summary["applied"] == 1 and len(anchors) >= 6
        assert fn(c, C.c_float(120.0), 2, C.c_float(1.0), C.byref(moved), C.byref(newlen)) == 1
        assert (moved.value, newlen.value) == (len(anchors) - 2, y.shape[1]) and y.shape[1] == length
        assert wc.same_bits(played(), y)
        on2 = onset_ref.onsets(y, 0, None, d["hop"], d["gate"], d["threshold"], d["min_gap"], d["max_onsets"])[0]
        assert [tuple(int(v) for v in r) for r in on2] == device_onsets()
        # a clip that plays a re-render is refused: warp first, then tune and level
        zl.ClipAudioSource_setGain(c, C.c_float(-3.0))
        assert fn(c, C.c_float(120.0), 2, C.c_float(1.0), None, None) == _abi.ZLHIP_ERR_STATE
        zl.ClipAudioSource_destroy(c)
        # src_bpm 0 detects: silence has no tempo, which returns 0 and changes nothing
        quiet = np.zeros(48000, f32)
        path = str(tmp_path / "quiet.wav").encode()
        assert zl.libzl_wav_write(path, quiet.ctypes.data, None, quiet.size, SR, 32) == 0
        c = zl.ClipAudioSource_new(path, False)
        assert c
        cid = zl.ClipAudioSource_engineClip(c)
        moved, newlen = C.c_int(-7), C.c_int(-7)
        assert fn(c, C.c_float(0.0), 2, C.c_float(1.0), C.byref(moved), C.byref(newlen)) == 0 and (moved.value, newlen.value) == (-7, -7)
        assert wc.same_bits(played(), quiet[None, :])
        zl.ClipAudioSource_destroy(c)
    finally:
        zl.shutdownJuce()
