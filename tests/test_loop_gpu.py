"""Loop finder, GPU tier: the kernels of libzl_amd/csrc/zl_loop.hip against the numpy / Python-integer restatement (tests/loop_ref.py):
every cost of the matrix, every item record and every integer of the result bit for bit, the three dB fields within 1e-9 (two log10
implementations, each good to an ulp of a value below 12, times 10: six orders below that).  Clips of at most 24000 frames."""
import ctypes as C

import numpy as np
import pytest

import loop_ref as lr
from loop_checks import SR, check_batch as _check_batch, same as _same, upload as _upload
from scenario import Scene, play_cmd, run_backend, run_oracle

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=64, sound_arena_bytes=16 << 20)
    yield s
    s.close()


def test_the_grid_equals_the_restatement_in_one_call(syn):
    """tests/loop_ref.py's grid (the CPU tier holds the host harness to the same cases) in ONE clip_loop_batch call"""
    cases = lr.grid()
    ids = [_upload(syn, x) for _, x, _ in cases]
    try:
        reqs = [dict(q, clip=cid) for cid, (_, _, q) in zip(ids, cases)]
        bad, outs = _check_batch(syn, reqs, {cid: x for cid, (_, x, _) in zip(ids, cases)})
        assert not bad, (len(bad), bad[:3])
        by = {what: o for (what, _, _), o in zip(cases, outs)}
        assert by["full scale"]["shift"] == 6 and by["short clip"]["found"] == 0 and by["64x64 ch2"]["starts"] == by["64x64 ch2"]["ends"] == 64
        assert sum(o["found"] for o in outs) == len(outs) - 2
    finally:
        for cid in ids:
            syn.unregister_clip(cid)


def test_a_call_above_the_cost_matrix_keeps_items_and_result_only(syn):
    """Rs = Re = 600: 1201 x 1201 candidate pairs, more than 2^20 -- the pairs kernel stores no costs (loop_costs: ZLHIP_ERR_STATE), 361
    items with partial tiles on both sides"""
    from libzl_amd import ZlHipError
    src = lr.tone(218.4, 2, 24000, seed=7)
    cid = _upload(syn, src)
    try:
        r = dict(clip=cid, start_frame=6000, stop_frame=18011, start_search=600, stop_search=600, window=256)
        bad, outs = _check_batch(syn, [r], {cid: src}, costs=False)
        assert not bad, bad
        assert outs[0]["starts"] == 1201 and outs[0]["pairs"] == 1201 * 1201 and len(syn.loop_items(0)) == 19 * 19
        n = (outs[0]["stop_frame"] - outs[0]["start_frame"]) / 218.4
        assert abs(n - round(n)) <= 0.02 and outs[0]["improvement_db"] >= 20.0, outs[0]
        with pytest.raises(ZlHipError, match=r"\(-5\)"):
            syn.loop_costs(0)
        # a small call afterwards keeps its costs again
        bad, _ = _check_batch(syn, [dict(r, start_search=20, stop_search=70)], {cid: src})
        assert not bad, bad
    finally:
        syn.unregister_clip(cid)


def test_a_mixed_batch_with_nothing_found_in_the_middle(syn):
    a, b, short = lr.tone(100.0, 1, 9000, seed=1), lr.tone(61.7, 2, 7001, seed=2), lr.tone(50.0, 2, 150, seed=3)
    ia, ib, ic = _upload(syn, a), _upload(syn, b), _upload(syn, short)
    try:
        reqs = [dict(clip=ia, start_frame=2001, stop_frame=7000, start_search=100, stop_search=90, window=128),
                dict(clip=ic, start_frame=0, stop_frame=150),                                                   # shorter than the window: no candidates
                dict(clip=ib, start_frame=1003, stop_frame=6000, start_search=-1, stop_search=150, window=32),
                dict(clip=ia, start_frame=3000, stop_frame=3100, start_search=30, stop_search=30, window=16, min_length=500),     # no admissible pair
                dict(clip=ib, start_frame=77, stop_frame=6960, window=64, min_length=3)]                         # the defaults' 480 frames, clipped at both edges
        bad, outs = _check_batch(syn, reqs, {ia: a, ib: b, ic: short})
        assert not bad, bad
        assert [o["found"] for o in outs] == [1, 0, 1, 0, 1] and outs[2]["starts"] == 1 and outs[4]["nominal_valid"] == 1
        assert all(v == 0 for v in outs[1].values()) and all(v == 0 for v in outs[3].values())
        assert syn.loop_items(1) == [] and len(syn.loop_items(3)) == 1 and syn.loop_costs(1).shape == (0, 0)
    finally:
        for c in (ia, ib, ic):
            syn.unregister_clip(c)


def test_errors_leave_out_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = lr.tone(100.0, 2, 24000, seed=8)
    cid = _upload(syn, src)
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    R, T = _abi.LoopRequest, _abi.Loop
    out = (T * 40)()
    C.memset(out, 0x5A, C.sizeof(out))
    INV = _abi.ZLHIP_ERR_INVALID

    def untouched():
        return bytes(out) == b"\x5a" * C.sizeof(out)

    def single(*a):
        r = R(*a)
        rc = lib.zlhip_sound_loop(e, C.byref(r), out)
        assert untouched(), a
        return rc

    def batch(reqs, nreq=None):
        arr = (R * max(1, len(reqs)))(*reqs)
        rc = lib.zlhip_sound_loop_batch(e, arr, len(reqs) if nreq is None else nreq, out)
        assert untouched()
        return rc

    ok = (cid, 6000, 18000, 100, 100, 256, 256)
    assert single(63, *ok[1:]) == INV and single(-1, *ok[1:]) == INV and single(64, *ok[1:]) == INV and single(gone, *ok[1:]) == INV
    for s0, e0 in ((-1, 18000), (6000, 6000), (6000, 5999), (6000, 24001), (24000, 24001)):
        assert single(cid, s0, e0, *ok[3:]) == INV, (s0, e0)
    for rs, re in ((2048, 100), (100, 2048), (-2, 100), (100, -2)):
        assert single(cid, 6000, 18000, rs, re, 256, 256) == INV, (rs, re)
    for w in (8, 24, 1040, -256):
        assert single(cid, 6000, 18000, 100, 100, w, 256) == INV, w
    assert single(cid, 6000, 18000, 100, 100, 256, -1) == INV
    wide = R(cid, 6000, 18000, 2047, 2047, 16, 1)                  # 4095 x 4095 candidates: 64 x 64 = 4096 items each
    assert batch([wide] * 17) == INV                               # 69632 work items in one call
    assert batch([R(*ok)], nreq=-1) == INV
    assert batch([R(*ok), R(gone, *ok[1:])]) == INV                # one bad request fails the whole call
    assert b"sound_loop" in lib.zlhip_last_error(e)
    assert lib.zlhip_sound_loop_batch(e, None, 1, out) == INV and lib.zlhip_sound_loop_batch(e, (R * 1)(R(*ok)), 1, None) == INV
    n = C.c_int32(-77)
    assert lib.zlhip_debug_loop_items(e, 99, None, 0, C.byref(n)) == INV and lib.zlhip_debug_loop_costs(e, 99, None, 0, C.byref(n), C.byref(n)) == INV and n.value == -77
    # the limits themselves are fine
    assert batch([], nreq=0) == 0
    assert lib.zlhip_sound_loop_batch(e, (R * 2)(R(*ok), R(cid, 0, 24000, -1, -1, 1024, 1)), 2, out) == 0
    want = lr.loop(src, SR, *ok[1:])
    assert _same({k: getattr(out[0], k) for k, _ in T._fields_}, want) and out[0].found == 1 and out[1].found == 0 and bytes(out)[2 * 80:] == b"\x5a" * (38 * 80)
    c = np.zeros(4, np.uint32)
    a, b = C.c_int32(0), C.c_int32(0)
    assert lib.zlhip_debug_loop_costs(e, 0, c.ctypes.data, 4, C.byref(a), C.byref(b)) == _abi.ZLHIP_ERR_CAPACITY and (a.value, b.value) == (201, 201) and not c.any()
    rec = (_abi.LoopItem * 1)()
    assert lib.zlhip_debug_loop_items(e, 0, C.addressof(rec), 1, C.byref(a)) == _abi.ZLHIP_ERR_CAPACITY and a.value == 16
    syn.unregister_clip(cid)


def test_group_loop_equals_the_single_engine(syn):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    src = lr.tone(130.0, 2, 20000, seed=6)
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        cid, gid = _upload(syn, src), _upload(g, src)
        for args in ((5000, 15000), (5003, 15000, 70, -1, 64, 100)):
            a = g.clip_loop(gid, *args)
            assert a == syn.clip_loop(cid, *args) and a["found"] == 1
        assert _same(a, lr.loop(src, SR, 5003, 15000, 70, -1, 64, 100))
        syn.unregister_clip(cid)
        a, b = g.clip_loop_batch([(gid, 5000, 15000, 30, 30), (gid, 0, 100, -1, -1)])
        assert a["found"] == 1 and b["found"] == 0
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_loop_batch([(gid, 5000, 15000, 0, 0, 24)])


def test_libzl_clip_find_and_snap_loop(built, tmp_path):
    """libzl_hotpath_clip_find_loop / _snap_loop / clips_snap_loops on tones: the published parameters map to the found frames through the
    voice's two formulas, a snap below the bar changes nothing, and a looping voice rendered across two laps with the published
    parameters equals the oracle run with the same parameters bit for bit"""
    from libzl_amd import SamplerSynth, _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        tone = lr.tone(218.4, 1, 24000, seed=11)
        other = lr.tone(133.7, 1, 24000, seed=12)
        clips = []
        for name, src in (("a", tone), ("b", tone), ("c", other)):
            path = str(tmp_path / (name + ".wav")).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, None, src.shape[1], SR, 32) == 0
            clips.append(zl.ClipAudioSource_new(path, False))
            assert clips[-1]
            zl.ClipAudioSource_setStartPosition(clips[-1], C.c_float(0.1))
            zl.ClipAudioSource_setLength(clips[-1], C.c_float(0.25), 120)      # 0.125 s: the nominal loop is about [4800, 10800)
        a, b, c = clips

        def params(clip):
            p = _abi.ClipParams()
            assert zl.libzl_hotpath_clip_params(clip, C.byref(p)) == 0
            return p

        p0 = params(a)
        s0, e0 = lr.frame_of(p0.start_position_seconds, SR), lr.stop_of(p0.start_position_seconds, p0.length_seconds, SR)
        assert s0 == 4800 and e0 in (10799, 10800)                 # (0.1f + 0.125f is a float of its own)
        want = lr.loop(tone, SR, s0, e0)
        assert want["found"] == 1 and want["improvement_db"] >= 20.0
        s, e, seam, nominal = C.c_int(-1), C.c_int(-1), C.c_double(-1.0), C.c_double(-1.0)
        assert zl.libzl_hotpath_clip_find_loop(None, 0.0, 0, C.byref(s), C.byref(e), C.byref(seam), C.byref(nominal)) < 0
        assert zl.libzl_hotpath_clip_find_loop(a, -1.0, 0, C.byref(s), C.byref(e), C.byref(seam), C.byref(nominal)) < 0
        assert zl.libzl_hotpath_clip_find_loop(a, 0.0, 24, C.byref(s), C.byref(e), C.byref(seam), C.byref(nominal)) < 0 and (s.value, e.value, seam.value) == (-1, -1, -1.0)
        assert zl.libzl_hotpath_clip_find_loop(a, 0.0, 0, C.byref(s), C.byref(e), C.byref(seam), C.byref(nominal)) == 1
        assert (s.value, e.value) == (want["start_frame"], want["stop_frame"]) and abs(seam.value - want["seam_db"]) <= 1e-9 and abs(nominal.value - want["nominal_db"]) <= 1e-9
        narrow = lr.loop(tone, SR, s0, e0, 96, 96, 64)
        assert zl.libzl_hotpath_clip_find_loop(a, 2.0, 64, C.byref(s), C.byref(e), None, None) == 1 and (s.value, e.value) == (narrow["start_frame"], narrow["stop_frame"])
        assert bytes(params(a)) == bytes(p0)                       # finding changes nothing

        # a snap below the bar changes nothing
        s, e = C.c_int(-1), C.c_int(-1)
        assert zl.libzl_hotpath_clip_snap_loop(a, 0.0, 200.0, C.byref(s), C.byref(e)) == 0 and (s.value, e.value) == (-1, -1) and bytes(params(a)) == bytes(p0)
        assert zl.libzl_hotpath_clip_snap_loop(a, 0.0, float("nan"), C.byref(s), C.byref(e)) < 0 and zl.libzl_hotpath_clip_snap_loop(None, 0.0, 0.0, C.byref(s), C.byref(e)) < 0
        # the snap: the published parameters map to the found frames through the voice's formulas; everything else stays
        assert zl.libzl_hotpath_clip_snap_loop(a, 0.0, 20.0, C.byref(s), C.byref(e)) == 1 and (s.value, e.value) == (want["start_frame"], want["stop_frame"])
        p1 = params(a)
        assert lr.frame_of(p1.start_position_seconds, SR) == s.value and lr.stop_of(p1.start_position_seconds, p1.length_seconds, SR) == e.value
        assert p1.length_in_beats == p0.length_in_beats and list(p1.slice_positions) == list(p0.slice_positions) and p1.root_note == p0.root_note
        # the bank call: b moves to the same points as a did, a NULL stays, c finds its own
        arr = (C.c_void_p * 3)(b, None, c)
        applied = (C.c_int * 3)(-1, -1, -1)
        assert zl.libzl_hotpath_clips_snap_loops(arr, 3, 0.0, 20.0, applied) == 2 and list(applied) == [1, 0, 1]
        assert bytes(params(b)) == bytes(p1)
        pc = params(c)
        wc = lr.loop(other, SR, s0, e0)
        assert wc["improvement_db"] >= 20.0
        assert (lr.frame_of(pc.start_position_seconds, SR), lr.stop_of(pc.start_position_seconds, pc.length_seconds, SR)) == (wc["start_frame"], wc["stop_frame"])
        assert zl.libzl_hotpath_clips_snap_loops((C.c_void_p * 2)(a, a), 2, 0.0, 20.0, None) < 0         # a clip twice
        for clip in clips:
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()

    # a looping voice across two laps of the snapped loop, against the oracle with the same parameters
    lap = e.value - s.value
    sc = Scene(num_buses=1, voices_per_bus=2, fs=SR, nframes=256, nblocks=(2 * lap + 1200) // 256 + 1)
    sc.sounds.append((tone[0], None, SR))

    def setup(lib, clip):
        clip.startPositionInSeconds = p1.start_position_seconds
        clip.lengthInSeconds = p1.length_seconds
        clip.lengthInBeats = p1.length_in_beats
    sc.clip_setup[0] = setup
    sc.events[0] = [("cmd", play_cmd(0, midi_channel=-2, loop=True, note=60, volume=1.0), 0)]
    ref, orep, _ = run_oracle(sc)
    out, rep, syn2, _ = run_backend(sc, SamplerSynth, batch=16)
    syn2.close()
    assert np.array_equal(ref.view(np.int32), out.view(np.int32)) and np.abs(out).max() > 0.05
    assert all(orep[v].valid == rep[v].valid and orep[v].gain == rep[v].gain and orep[v].progress == rep[v].progress for v in range(2)) and any(rep[v].valid for v in range(2))
    # the seam the voice crossed is the one that was found: frame `lap` of the output continues from the loop's start
    heard = out[0, 0]
    jump = np.abs(np.diff(heard[lap - 300:lap + 300])).max()
    assert jump <= 1.5 * np.abs(np.diff(heard[400:lap - 400])).max(), jump
