"""Clip edit, GPU tier: the kernels of libzl_amd/csrc/zl_edit.hip against the numpy restatement (tests/edit_ref.py).  Every extent is
read back whole (zlhip_debug_sound_extent) from a small arena that held noise and compared == with the restatement; then the single
call and an edit of an edited clip, the finite flag, a loud neighbour, every refusal, the scan that a call without TRIM does not
launch, a voice rendered over a reversed and cropped clip against the oracle's run over the restatement's data, the group, and the
libzl-named layer."""
import ctypes as C
import os

import numpy as np
import pytest

import edit_cases as ec
import edit_ref as er
import loop_ref as lr
from edit_cases import SR, check_call, dirty, mismatch, upload

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def case(x, **q):
    return dict(tag="", x=x, q=er.request(**q))


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
def test_the_grid_in_one_call(built):
    """tests/edit_cases.py::grid (tests/test_edit_cpu.py asserts what it covers): every case in ONE call, identity and silent requests
    first, last and twice in a row; then every clip's info and that the clips with nothing to change are untouched"""
    cases = ec.grid()
    with make(max_sounds=512, sound_arena_bytes=32 << 20) as s:
        dirty(s, 3 << 20)
        ids = [upload(s, c["x"]) for c in cases]
        wants = [ec.want(c)[0] for c in cases]
        before = {i: s.clip_extent(cid) for i, (cid, w) in enumerate(zip(ids, wants)) if not w["applied"]}
        assert len(before) >= 6
        bad, outs = check_call(s, cases, ids)
        assert not bad, (len(bad), bad[:3])
        assert [i for i, o in enumerate(outs) if not o["applied"]] == sorted(before)
        for i, ext in before.items():
            assert same(s.clip_extent(ids[i]), ext), (i, cases[i]["tag"])
        for cid, c, w in zip(ids, cases, wants):
            assert s.clip_info(cid) == {"length": w["length"], "channels": c["x"].shape[0], "sample_rate": SR, "finite": bool(np.isfinite(c["x"]).all()), "rendered": False}, c["tag"]
        # the extents' tails are the kernel's zeros, not the arena's noise
        for cid, c, w in zip(ids, cases, wants):
            if w["applied"]:
                ext = s.clip_extent(cid)
                data = w["length"] * c["x"].shape[0]
                assert ext.size > data and not ext[data:].any(), c["tag"]


def test_the_single_call_and_a_second_edit_of_the_same_clip(built):
    with make() as s:
        dirty(s, 100000)
        rng = np.random.default_rng(31)
        x = ec.quiet(rng, 2, 5000)
        x[:, 1203:3777] = ec.clip(rng, 2, 3777 - 1203)
        x[0, 1203] = x[1, 3776] = 0.5
        c = case(x, flags=er.TRIM, pre_roll_frames=100, hold_frames=50, fade_in_frames=64, fade_out_frames=300, curve=er.SMOOTH)
        cid = upload(s, x)
        got = s.clip_edit(cid, flags=er.TRIM, pre_roll_frames=100, hold_frames=50, fade_in_frames=64, fade_out_frames=300, curve=er.SMOOTH)
        assert (got["applied"], got["first_frame"], got["num_frames"], got["first_loud"], got["last_loud"]) == (1, 1103, 3777 + 50 - 1103, 1203, 3776)
        assert mismatch(s, cid, c, got) is None
        # again, on the edited data: a crop from an odd frame, reversed
        L, R = s.read_clip(cid)
        c2 = case(np.stack([L, R]), first_frame=333, num_frames=1001, flags=er.REVERSE, fade_in_frames=7, curve=er.SQRT)
        got = s.clip_edit(cid, 333, 1001, er.REVERSE, fade_in_frames=7, curve=er.SQRT)
        assert got["length"] == 1001 and got["reversed"] == 1 and mismatch(s, cid, c2, got) is None
        assert s.clip_info(cid)["length"] == 1001
        # reversed twice: the data it had
        y = s.clip_extent(cid)
        s.clip_edit(cid, flags=er.REVERSE)
        assert not same(s.clip_extent(cid), y)
        s.clip_edit(cid, flags=er.REVERSE)
        assert same(s.clip_extent(cid), y)


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def test_the_finite_flag(built):
    """a finite clip keeps the flag through a crop with fades (3e38 inside a fade among them: a weight is at most 1).  A clip with an inf
    lacks the flag from its upload on and never gains it: not with the inf inside a fade (where the verdict is set as well -- weight 0
    included, 0 inf is a NaN), not with the inf only copied, and not with the inf cropped away, where every written sample is finite"""
    from libzl_amd import _abi
    rng = np.random.default_rng(34)
    base = rng.uniform(-1.0, 1.0, (2, 400)).astype(f32)
    big = base.copy(); big[0, 105] = 3e38; big[1, 50] = 3e38       # finite: the flag is set; 3e38 times a weight below 1 stays finite
    cases, had, expect = [], [], []
    for k, (frame, q) in enumerate(((None, {}), (105, {}), (299, {}), (150, {}), (50, {}), (297, dict(flags=er.REVERSE)))):
        x = base.copy()
        if frame is not None:
            x[1, frame] = np.inf
        cases.append(case(x, first_frame=100, num_frames=200, fade_in_frames=10, fade_out_frames=10, curve=er.SQRT, **q))
        had.append(frame is None); expect.append(frame is None)
    cases.append(case(big, first_frame=100, num_frames=200, fade_in_frames=10, fade_out_frames=10)); had.append(True); expect.append(True)
    with make() as s:
        dirty(s, 100000)
        ids = [s.register_clip_pcm(np.ascontiguousarray(c["x"].T), _abi.PCM_F32, 2, SR) for c in cases]
        assert [s.clip_info(i)["finite"] for i in ids] == had
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
        assert [s.clip_info(i)["finite"] for i in ids] == expect
        # (cases 3 and 4: the inf is copied or cropped away, the written faded samples are finite -- and the clip still does not gain the flag)
        for c in cases[3:5]:
            res, y = er.edit(c["x"], c["q"])
            assert er.faded_finite(y, 10, 10)
        # a clip from 16-bit PCM has the flag without a check at upload; a reversed crop with a fade keeps it
        pcm = (base.T * 30000.0).astype(np.int16)
        cid = s.register_clip_pcm(np.ascontiguousarray(pcm), _abi.PCM_S16, 2, SR)
        assert s.clip_info(cid)["finite"]
        assert s.clip_edit(cid, 10, 300, er.REVERSE, fade_in_frames=20)["applied"] == 1
        assert s.clip_info(cid)["finite"]


# ---- a neighbour does not leak --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two at +-7.9 in a small arena that held noise, trimmed over its whole data: a neighbour's float in the scan's
    head or tail group would be a loud frame, one in the copy would change the extent"""
    with make(max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(35)
        dirty(s, 200000)
        for n in (3333, 2 * er.CHUNK + 1, 131):
            loud = [np.repeat(rng.choice(np.array([-7.9, 7.9], f32), (1, m)), ch, axis=0) for m in (3001, 3003)]
            q0 = ec.quiet(rng, ch, n)
            q1 = q0.copy(); q1[ch - 1, n // 3] = 0.5; q1[0, n // 2] = -0.5
            for quiet in (q0, q1):
                ids = [upload(s, x) for x in (loud[0], quiet, loud[1])]
                cases = [case(quiet, flags=er.TRIM | er.REVERSE), case(loud[0], flags=er.TRIM), case(loud[1], flags=er.TRIM, fade_out_frames=3)]
                before = [s.clip_extent(i) for i in ids]
                bad, outs = check_call(s, cases, [ids[1], ids[0], ids[2]])
                assert not bad, bad
                assert same(s.clip_extent(ids[0]), before[0]) and (quiet is q1 or same(s.clip_extent(ids[1]), before[1]))     # untouched: bit-identical
                assert (outs[0]["silent"], outs[0]["first_loud"], outs[0]["last_loud"]) == ((1, -1, -1) if quiet is q0 else (0, n // 3, n // 2))
                assert (outs[1]["first_loud"], outs[1]["last_loud"], outs[1]["applied"]) == (0, 3000, 0)
                for cid in ids:
                    s.unregister_clip(cid)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_every_clip_and_out_as_they_were(built):
    from libzl_amd import _abi
    INV, CAP, STATE = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY, _abi.ZLHIP_ERR_STATE
    rng = np.random.default_rng(41)
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        a, b = ec.clip(rng, 2, 4000), ec.clip(rng, 1, 5000)
        big = ec.clip(rng, 2, 70000)                               # 560 KB: a second extent of it does not fit the arena (1 MiB)
        big[:, :3] = 0.0                                           # (a trim cuts three frames: the new extent is as large, to within them)
        ia, ib, ibig = upload(s, a), upload(s, b), upload(s, big)
        exts = [s.clip_extent(i) for i in (ia, ib, ibig)]
        R = _abi.EditRequest

        def req(cid, **q):
            q = er.request(**q)
            return R(cid, *(int(q[k]) for k in er.REQUEST_KEYS[:-1]), float(q["threshold"]))

        def call(reqs, count=None):
            arr = (R * max(1, len(reqs)))(*reqs)
            out = (_abi.Edit * max(1, len(reqs)))()
            C.memset(out, 0x5A, C.sizeof(out))
            rc = lib.zlhip_sound_edit_batch(e, arr, len(reqs) if count is None else count, out)
            return rc, bytes(out) == b"\x5a" * C.sizeof(out)

        def unchanged():
            return all(same(s.clip_extent(i), x) for i, x in zip((ia, ib, ibig), exts))

        good = req(ia, first_frame=1000, num_frames=2000, flags=er.TRIM | er.REVERSE)
        other = req(ib, first_frame=17, flags=er.TRIM)
        assert s.clip_edit(ib)["applied"] == 0                     # (the identity: no buffers either)
        mem = s.memory_bytes()
        bad = [req(ia, first_frame=1000, num_frames=3001), req(ia, first_frame=4000), req(ia, first_frame=-1, num_frames=10), req(ia, num_frames=-1), req(ia, flags=4),
               req(ia, curve=3), req(ia, fade_in_frames=-1), req(ia, fade_out_frames=-1), req(ia, flags=1, pre_roll_frames=-1), req(ia, flags=1, hold_frames=-1),
               req(ia, flags=1, threshold=-1.0), req(ia, flags=1, threshold=float("inf")), req(ia, flags=1, threshold=float("nan")),
               req(31, flags=2), req(-1, flags=2), req(99, flags=2)]
        for r in bad:
            assert call([r]) == (INV, True), bytes(r)
            assert call([other, r]) == (INV, True), bytes(r)       # one bad request fails the call
        assert b"sound_edit" in lib.zlhip_last_error(e)
        assert call([good, good]) == (INV, True) and call([good, other, req(ia, flags=2)]) == (INV, True)       # duplicates
        assert call([good], count=-1) == (INV, True) and call([], count=0) == (0, True)
        assert lib.zlhip_sound_edit_batch(e, None, 1, None) == INV and lib.zlhip_sound_edit(None, None, None) == INV
        assert unchanged() and s.memory_bytes() == mem
        # a clip that plays a re-render
        s.rerender_clip(ib, gain_db=-6.0)
        bre, mem = s.clip_extent(ib), s.memory_bytes()
        assert call([good, other]) == (STATE, True) and call([req(ib, flags=2)]) == (STATE, True)
        assert b"re-render" in lib.zlhip_last_error(e)
        assert same(s.clip_extent(ib), bre) and same(s.clip_extent(ia), exts[0]) and s.memory_bytes() == mem
        assert call([req(ib)])[0] == 0                             # the identity: not judged
        s.rerender_clip(ib)
        assert unchanged()
        # an arena that cannot hold the call, decided behind the scan: the small clip's extent fits, the big one's does not -- neither changes
        assert call([good, req(ibig, flags=er.TRIM)]) == (CAP, True)
        assert unchanged()
        assert call([req(ibig, flags=er.REVERSE), good]) == (CAP, True)
        assert unchanged()
        # after the errors the call still works, and a trim that makes the big clip small enough fits
        bad_, outs = check_call(s, [case(a, first_frame=1000, num_frames=2000, flags=er.TRIM | er.REVERSE), case(b, first_frame=17, flags=er.TRIM),
                                    case(big, first_frame=100, num_frames=30000, flags=er.TRIM)], [ia, ib, ibig])
        assert not bad_, bad_
        assert [o["applied"] for o in outs] == [1, 1, 1]


# ---- the scan is launched only for TRIM -------------------------------------------------------------------------------------------------
def test_a_call_without_trim_makes_no_scan_launch(built):
    with make() as s:
        s.set_profiling(True)
        rng = np.random.default_rng(42)
        ids = [upload(s, ec.clip(rng, 2, 20000)) for _ in range(3)]
        assert s.clip_edit(ids[0], 100, 15000, er.REVERSE, fade_in_frames=100)["applied"] == 1
        scan, render = s.edit_timings()
        assert scan == 0.0 and render > 0.0
        assert s.clip_edit(ids[1], 100, 15000, er.TRIM, fade_in_frames=100)["applied"] == 1
        scan, render = s.edit_timings()
        assert scan > 0.0 and render > 0.0
        assert s.clip_edit(ids[2], 7, 0, 0)["applied"] == 1
        scan, render = s.edit_timings()
        assert scan == 0.0 and render > 0.0
        s.set_profiling(False)
        assert s.clip_edit(ids[2], 7, 0, er.TRIM)["applied"] == 1
        assert s.edit_timings() == (scan, render)                  # (the times of the last profiled call stay)


# ---- playback -------------------------------------------------------------------------------------------------------------------------
EDIT = dict(first_frame=501, num_frames=5000, flags=er.REVERSE, fade_in_frames=100, fade_out_frames=50, curve=er.SQRT)


def playback_scene(y, note, nblocks=24):
    """one looping voice over a free-running loop of some 2300 frames from frame 1440 of clip y (planar)"""
    from scenario import Scene, play_cmd
    sc = Scene(num_buses=1, voices_per_bus=2, fs=SR, mode=0, mix_group=0, nframes=256, nblocks=nblocks, bpm=120)
    sc.sounds.append((y[0].copy(), y[1].copy() if y.shape[0] == 2 else None, SR))

    def setup(lib, clip):
        lib.zlo_clip_set_start_position(clip, C.c_float(0.030005))
        lib.zlo_clip_set_length(clip, C.c_float(0.1), 120)           # no whole number of beats: the free-running loop branch
    sc.clip_setup[0] = setup
    sc.events[0] = [("cmd", play_cmd(0, midi_channel=-2, loop=True, note=note, volume=0.8), 0)]
    return sc


def play_edited(x, note, resident=False):
    """(the engine's audio of the scene over clip x cropped and reversed on the device, the oracle's audio over the restatement's data)"""
    from oracle import zl_oracle as zo
    from scenario import engine_cmd, run_oracle, snapshot_clip
    from libzl_amd.engine import synthetic_clocks
    c = case(x, **EDIT)
    res, y = er.edit(x, c["q"])
    sc = playback_scene(y, note)
    ref = zo.OracleSynth(1, 1, SR, 0, max_sounds=8)
    assert ref.register_clip(*sc.sounds[0]) == 0
    sc.clip_setup[0](ref.lib, ref.clips[0])
    p = snapshot_clip(ref.clips[0])                                 # the parameters of a clip over the edited data: the caller moves them
    s0, e0 = lr.frame_of(p.start_position_seconds, SR), lr.stop_of(p.start_position_seconds, p.length_seconds, SR)
    assert s0 == 1440 and 2000 <= e0 - s0 <= 2500 and e0 < y.shape[1]
    with make(num_buses=1, voices_per_bus=2, max_batch_blocks=sc.nblocks) as s:
        cid = upload(s, x)
        got = s.clip_edit(cid, **EDIT)
        assert got["applied"] == 1 and got["length"] == 5000 and mismatch(s, cid, c, got) is None
        s.set_clip_params(cid, p)
        s.handle_clip_command(engine_cmd(**sc.events[0][0][1]), 0)
        if resident:
            out = np.zeros((1, 2, sc.nblocks * 256), f32)
            clocks = synthetic_clocks(sc.nblocks, 256, SR)
            for k in range(sc.nblocks):
                L, R = s.process(256, clocks[k])
                out[:, 0, k * 256:(k + 1) * 256] = L
                out[:, 1, k * 256:(k + 1) * 256] = R
            assert s.rt_stats()[1] == sc.nblocks
        else:
            s.render_batch(sc.nblocks, 256, synthetic_clocks(sc.nblocks, 256, SR))
            out = np.array(s.read_bus(), copy=True)
    ref_bus, _, _ = run_oracle(sc)
    return out, ref_bus


def signal(seed):
    t = np.arange(6000, dtype=np.float64)
    v = 0.3 * np.sin(2.0 * np.pi * t / 218.4) * np.exp(-t / 3000.0)
    return (np.stack([v, 0.9 * v]) + np.random.default_rng(seed).standard_normal((2, 6000)) * 0.01).astype(f32)


@pytest.mark.parametrize("note", [60, 67], ids=["on-grid", "pitched"])
def test_a_voice_over_a_reversed_and_cropped_clip_equals_the_oracle_over_the_restatement(built, note):
    out, ref_bus = play_edited(signal(36), note)
    assert out.shape == ref_bus.shape and len(np.unique(out[0, 0])) > 1000
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_a_voice_through_the_resident_kernel_equals_the_oracle(built, rt_env):
    out, ref_bus = play_edited(signal(37), 60, resident=True)
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


# ---- the group, the libzl-named layer ---------------------------------------------------------------------------------------------------
def test_group_edits_on_every_member(built):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    rng = np.random.default_rng(47)
    with SamplerSynthGroup([0, 0], 4, 8, max_frames=256, max_batch_blocks=8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        q = ec.quiet(rng, 2, 3000); q[1, 700] = 0.5; q[0, 2100] = -0.5
        cases = [case(q, flags=er.TRIM, pre_roll_frames=11, hold_frames=5, fade_out_frames=40), case(ec.clip(rng, 1, 700), first_frame=257, flags=er.REVERSE, fade_in_frames=9, curve=er.SMOOTH),
                 case(ec.clip(rng, 2, 300))]
        ids = [upload(g, c["x"]) for c in cases]
        outs = g.clip_edit_batch([dict(clip=cid, **c["q"]) for cid, c in zip(ids, cases)])
        assert [o["applied"] for o in outs] == [1, 1, 0]
        for r in range(2):
            for cid, c, got in zip(ids, cases, outs):
                n = C.c_size_t(0)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, None, 0, C.byref(n)) == 0
                ext = np.empty(n.value, f32)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, ext.ctypes.data, ext.size, None) == 0
                want, wext = ec.want(c)
                assert all(got[k] == want[k] for k in er.RESULT_FIELDS), (r, cid, got, want)
                assert ec.same_bits(ext, wext) is None, (r, cid)
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_edit_batch([dict(clip=ids[0], flags=2), dict(clip=ids[0], flags=2)])


def test_libzl_trim_crop_and_reverse(built, tmp_path):
    """the three calls of the libzl-named layer on loaded clips: the data equals the restatement's, and the clip's seconds have moved so
    that the frames a voice derives from them are the intended ones; a re-rendered clip is refused; a bank is trimmed in one call"""
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        e = zl.libzl_hotpath_engine()
        rng = np.random.default_rng(51)

        def recording(n, lo, hi):
            x = np.zeros((1, n), f32)
            x[0, lo:hi] = rng.uniform(0.01, 0.5, hi - lo).astype(f32)
            return x

        srcs = [recording(24000, 5003, 15001), ec.clip(rng, 1, 24000), ec.clip(rng, 1, 24000), recording(9000, 100, 8000), np.zeros((1, 5000), f32),
                recording(9000, 0, 9000), recording(7000, 3000, 4000)]
        srcs[5][0, 0] = srcs[5][0, -1] = 0.5                       # loud from its first to its last frame: nothing to cut
        clips = []
        for k, src in enumerate(srcs):
            path = str(tmp_path / ("t%d.wav" % k)).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, None, src.shape[1], SR, 32) == 0
            clips.append(zl.ClipAudioSource_new(path, False))
            assert clips[-1]
        for c in clips[:3]:
            zl.ClipAudioSource_setStartPosition(c, C.c_float(0.15))
            zl.ClipAudioSource_setLength(c, C.c_float(0.25), 120)      # 0.125 s: the region is about [7200, 13200)

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

        # trim: 10 ms of pre-roll, 20 ms of hold
        t = clips[0]
        s0, e0 = frames(t)
        assert 7199 <= s0 <= 7200 and 13199 <= e0 <= 13201
        removed, length = C.c_int(-7), C.c_int(-7)
        assert zl.libzl_hotpath_clip_trim_silence(None, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), C.byref(removed), C.byref(length)) < 0
        assert zl.libzl_hotpath_clip_trim_silence(t, C.c_float(0.0), C.c_float(-1.0), C.c_float(0.0), C.byref(removed), C.byref(length)) < 0
        assert zl.libzl_hotpath_clip_trim_silence(t, C.c_float(float("nan")), C.c_float(0.0), C.c_float(0.0), C.byref(removed), C.byref(length)) < 0
        assert (removed.value, length.value) == (-7, -7)
        assert zl.libzl_hotpath_clip_trim_silence(t, C.c_float(0.0), C.c_float(10.0), C.c_float(20.0), C.byref(removed), C.byref(length)) == 1
        res, y = er.edit(srcs[0], er.request(flags=er.TRIM, pre_roll_frames=480, hold_frames=960))
        assert (res["first_loud"], res["last_loud"]) == (5003, 15000)
        assert (removed.value, length.value) == (5003 - 480, 15001 + 960 - (5003 - 480)) == (res["first_frame"], res["length"])
        assert same(extent(t), er.extent(y))
        assert frames(t) == (s0 - removed.value, e0 - removed.value)
        assert params(t).duration_seconds == f32(length.value / SR)
        assert zl.libzl_hotpath_clip_trim_silence(t, C.c_float(0.0), C.c_float(10.0), C.c_float(20.0), C.byref(removed), C.byref(length)) == 0      # tight already
        assert (removed.value, length.value) == (0, res["length"]) and same(extent(t), er.extent(y))
        # crop to the region, 5 ms in, 10 ms out
        c = clips[1]
        s0, e0 = frames(c)
        n = C.c_int(-7)
        assert zl.libzl_hotpath_clip_crop(c, C.c_float(5.0), C.c_float(10.0), 7, C.byref(n)) < 0 and n.value == -7
        assert zl.libzl_hotpath_clip_crop(c, C.c_float(-5.0), C.c_float(10.0), 0, C.byref(n)) < 0 and n.value == -7
        assert zl.libzl_hotpath_clip_crop(c, C.c_float(5.0), C.c_float(10.0), er.SQRT, C.byref(n)) == 1
        res, y = er.edit(srcs[1], er.request(first_frame=s0, num_frames=e0 - s0, fade_in_frames=240, fade_out_frames=480, curve=er.SQRT))
        assert n.value == e0 - s0 == res["length"] and same(extent(c), er.extent(y))
        p = params(c)
        assert p.start_position_seconds == 0.0 and frames(c) == (0, n.value) and p.duration_seconds == f32(n.value / SR)
        assert zl.libzl_hotpath_clip_crop(c, C.c_float(0.0), C.c_float(0.0), 0, C.byref(n)) == 0 and same(extent(c), er.extent(y))      # the whole data, no fade
        # reverse: the same region, backwards
        r = clips[2]
        s0, e0 = frames(r)
        assert zl.libzl_hotpath_clip_reverse(r) == 1
        assert same(extent(r), er.extent(srcs[2][:, ::-1]))
        assert frames(r) == (24000 - e0, 24000 - s0) and params(r).duration_seconds == f32(24000 / SR)
        assert zl.libzl_hotpath_clip_reverse(r) == 1
        assert same(extent(r), er.extent(srcs[2])) and frames(r) == (s0, e0)
        # a clip that plays a re-render is refused: edit first, level afterwards
        zl.ClipAudioSource_setGain(r, C.c_float(-3.0))
        info = _abi.SoundInfo()
        assert zl.zlhip_sound_info_get(e, zl.ClipAudioSource_engineClip(r), C.byref(info)) == 0 and info.rendered == 1
        assert zl.libzl_hotpath_clip_reverse(r) == _abi.ZLHIP_ERR_STATE
        assert zl.libzl_hotpath_clip_crop(r, C.c_float(0.0), C.c_float(0.0), 0, None) == _abi.ZLHIP_ERR_STATE
        assert zl.libzl_hotpath_clip_trim_silence(r, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), None, None) == _abi.ZLHIP_ERR_STATE
        # a bank (a NULL, a silent clip, a tight one, the re-rendered one): one call; -20 dB
        bank = [clips[3], None, clips[4], clips[5], r, clips[6]]
        arr = (C.c_void_p * 6)(*bank)
        applied = (C.c_int * 6)(*[-1] * 6)
        kept = extent(r)
        assert zl.libzl_hotpath_clips_trim(arr, 6, C.c_float(-20.0), C.c_float(1.0), C.c_float(2.0), applied) == 2
        assert list(applied) == [1, 0, 0, 0, 0, 1]
        for k in (3, 6):
            res, y = er.edit(srcs[k], er.request(flags=er.TRIM, pre_roll_frames=48, hold_frames=96, threshold=float(f32(10.0 ** (-20.0 / 20.0)))))
            assert res["applied"] and same(extent(clips[k]), er.extent(y))
            assert frames(clips[k]) == (0, res["length"]) and params(clips[k]).duration_seconds == f32(res["length"] / SR)
        assert same(extent(clips[4]), er.extent(srcs[4])) and same(extent(r), kept)
        assert zl.libzl_hotpath_clips_trim((C.c_void_p * 2)(clips[3], clips[3]), 2, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), None) < 0
        assert zl.libzl_hotpath_clips_trim(arr, -1, C.c_float(0.0), C.c_float(0.0), C.c_float(0.0), None) < 0
        for clip in clips:
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
