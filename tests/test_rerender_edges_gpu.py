"""Clip re-render on the device, what only the device runs (zl_k_stretch_seek, zl_k_stretch_synth of libzl_amd/csrc/zl_stretch.hip;
DESIGN.md section 8).  tests/test_rerender_gpu.py walks the speed x pitch grid at 44100, 48000 and 96000 Hz; here: the limits of the
geometry (the 16-frame overlap, a segment shorter than its cross-fade, seek windows below one wave and below one pass, an overlap the
multiple-of-8 rule shortens, W + O = 4608 -- the LDS staging at its limit -- and the rates just outside, which are rejected), a clip
at the rails under a 512-frame overlap (the int32 pair sums at their bound), one segment and whole numbers of segments, renders
that end at and one frame past a synthesis workgroup, ties between candidates in different lanes, waves and passes, a seek decided
by the last frame a candidate reads, the 8 zero frames behind a render in an arena that held noise, and a voice playing a render to
its end.  Everything is held to the numpy restatement (tests/stretch_ref.py) bit for bit, data and seek offsets; no tolerances."""
import ctypes as C

import numpy as np
import pytest

import stretch_ref as sr_
from oracle import zl_oracle as zo
from rerender_cases import (LAST_FRAME_CASES, PAD, TIE_SPEED, dirty, edge_cases, edge_id, edge_reference, extent_of, holds_ties,
                            last_frame_source, reference, same_bits, source, tie_cases, tie_source)
from scenario import engine_cmd, oracle_cmd, play_cmd, snapshot_clip

pytestmark = pytest.mark.gpu
EDGE = edge_cases()


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


def _planar(L, R):
    return np.stack([L, R]) if R is not None else L[None, :]


def _upload(syn, src, sr):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def first_difference(got, ref):
    if got.shape != ref.shape:
        return got.shape, ref.shape
    d = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=0))
    return d[:6], d.size


def holds(syn, cid, ref, roffs, tag):
    """the clip's playback data and the seek offsets of its last render against the restatement"""
    out = _planar(*syn.read_clip(cid))
    assert same_bits(out, ref), (tag, first_difference(out, ref))
    offs = syn.rerender_offsets(cid).astype(np.int64)
    assert np.array_equal(offs, roffs), (tag, offs[:12], roffs[:12])


def extent_holds(syn, cid, planar, tag):
    """the first (N + 8) ch floats of the clip's extent: its frames, then 8 zero frames (the floats between there and the 16-byte
    boundary are nobody's: nothing writes them and nothing reads them)"""
    want = extent_of(planar)
    got = syn.clip_extent(cid)
    assert got.size >= want.size and not want[planar.size:].any()
    assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32)), (tag, np.flatnonzero(got[:want.size] != want)[:8])


# ---- the edge grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGE, ids=[edge_id(c) for c in EDGE])
def test_an_edge_case_equals_the_restatement(syn, case):
    sr, ch, speed, pitch, gain, length, kind = case
    src, ref, roffs = edge_reference(case)
    cid = _upload(syn, src, sr)
    try:
        syn.rerender_clip(cid, gain_db=gain, pitch=pitch, speed=speed)
        holds(syn, cid, ref, roffs, case)
        if kind == "rail" or sr == 204800.0:
            assert roffs.any()                                     # (the scores differ: the seek has something to decide)
    finally:
        syn.unregister_clip(cid)


def test_all_edge_cases_in_one_call(syn):
    """one seek launch and one synthesis launch for all of them: windows from 6 to 4096 candidates side by side, jobs with one
    segment (no seek at all) between jobs with five, the synthesis grid sized by the 204800 Hz clip at speed 0.25"""
    refs = [edge_reference(c) for c in EDGE]
    assert max(r[1].shape[1] for r in refs) == 72000 and min(r[2].size for r in refs) == 1
    ids = [_upload(syn, r[0], c[0]) for c, r in zip(EDGE, refs)]
    try:
        syn.rerender_clips(ids, [c[4] for c in EDGE], [c[3] for c in EDGE], [c[2] for c in EDGE])
        for cid, c, (src, ref, roffs) in zip(ids, EDGE, refs):
            holds(syn, cid, ref, roffs, c)
    finally:
        for cid in ids:
            syn.unregister_clip(cid)


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,ch,period", tie_cases(), ids=[f"{int(c[0])}-{c[1]}ch-P{c[2]}" for c in tie_cases()])
def test_tying_candidates_resolve_to_the_smallest_offset(syn, sr, ch, period):
    """a clip of period P: the candidates o, o + P, o + 2 P ... of a window inside the clip have the same score to the bit, and they
    sit in different lanes of a wave (P = 37), in the same lane of neighbouring waves (64), in one thread on successive passes (512).
    The argmax must carry the smaller-offset rule through the shuffles, the eight waves and the passes"""
    src, ref, roffs = reference(("tie", ch, period), lambda: tie_source(sr, ch, period), sr, 0.0, 0.0, TIE_SPEED)
    holds_ties(sr, period, roffs)
    cid = _upload(syn, src, sr)
    try:
        syn.rerender_clip(cid, speed=TIE_SPEED)
        holds(syn, cid, ref, roffs, (sr, ch, period))
    finally:
        syn.unregister_clip(cid)


@pytest.mark.parametrize("sr,pitch,speed", LAST_FRAME_CASES)
@pytest.mark.parametrize("ch", [1, 2])
def test_the_last_frame_a_candidate_reads_decides_a_seek(syn, sr, pitch, speed, ch):
    """silence but for two frames: segment 2's only non-zero score is candidate W - 1's, from the product of its last frame -- frame
    W + O - 2 of the staged window, at 204800 Hz frame 4606 of the 4608 the LDS holds"""
    src, ref, roffs = reference(("last", ch), lambda: last_frame_source(sr, ch, pitch, speed), sr, 0.0, pitch, speed)
    assert roffs[1] == 0 and roffs[2] == sr_.geometry(sr, src.shape[1], 0.0, pitch, speed)["W"] - 1
    cid = _upload(syn, src, sr)
    try:
        syn.rerender_clip(cid, pitch=pitch, speed=speed)
        holds(syn, cid, ref, roffs, (sr, ch))
    finally:
        syn.unregister_clip(cid)


# ---- rejection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("sr,length,refused,taken", [
    (204850.0, 40000, dict(speed=0.5), [dict(speed=2.0, pitch=12.0), dict(speed=2.0, pitch=0.0)]),      # W = 4097; tau == 1; W = 3072
    (400.0, 300, dict(speed=4.0), [dict(speed=4.0, pitch=24.0), dict(speed=1.25, pitch=0.0)]),          # S = 16 = O; tau == 1; S = 26
], ids=["204850", "400"])
def test_a_rate_the_stretch_cannot_take_is_refused_and_the_clip_left_alone(syn, sr, length, refused, taken, ch):
    from libzl_amd import ZlHipError
    with pytest.raises(ValueError):
        sr_.geometry(sr, length, 0.0, refused.get("pitch", 0.0), refused["speed"])
    src = source(sr, ch, length, seed=length + ch)
    other = source(48000.0, ch, 5000, seed=3)
    cid, oid = _upload(syn, src, sr), _upload(syn, other, 48000.0)
    try:
        mem = syn.memory_bytes()
        for call in (lambda: syn.rerender_clip(cid, **refused),
                     # in a batch, behind a clip the call could take: all or nothing
                     lambda: syn.rerender_clips([oid, cid], 0.0, [3.0, refused.get("pitch", 0.0)], [1.25, refused["speed"]])):
            with pytest.raises(ZlHipError, match="sample rate"):
                call()
            assert same_bits(_planar(*syn.read_clip(cid)), src) and same_bits(_planar(*syn.read_clip(oid)), other)
            assert syn.memory_bytes() == mem
            assert not syn.clip_info(cid)["rendered"] and not syn.clip_info(oid)["rendered"]
            assert syn.rerender_offsets(cid).size == 0
        for params in taken:
            ref, roffs = sr_.render(src, sr, 0.0, params["pitch"], params["speed"])
            syn.rerender_clip(cid, **params)
            holds(syn, cid, ref, roffs, (sr, ch, params))
            assert syn.clip_info(cid)["rendered"]
        # refused again while it plays a render: the render stays
        with pytest.raises(ZlHipError, match="sample rate"):
            syn.rerender_clip(cid, **refused)
        holds(syn, cid, ref, roffs, (sr, ch, "after the refusal"))
        syn.rerender_clip(cid)
        assert same_bits(_planar(*syn.read_clip(cid)), src) and syn.memory_bytes() == mem
    finally:
        syn.unregister_clip(cid)
        syn.unregister_clip(oid)


# ---- the zero frames behind a render --------------------------------------------------------------------------------------------------
def _small(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=4, max_frames=256, max_batch_blocks=16, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def test_the_zero_frames_behind_a_render_in_an_arena_that_held_noise(built):
    """zl_k_stretch_synth writes N + 8 frames; a voice reads up to two frames past the end.  Renders whose N + 8 frames end at and one
    frame past a synthesis workgroup, and one four-segment stretch, mono and stereo each.  Then a shorter render and back to
    identity: the original's extent is as it was and so is the arena"""
    tail = [c for c in EDGE if (c[2], c[3]) == (1.0, 3.0)] + [c for c in EDGE if c[0] == 47250.0]
    assert sorted((c[5] + PAD, c[1]) for c in tail[:8]) == [(n, ch) for n in (256, 257, 512, 513) for ch in (1, 2)] and len(tail) == 10
    with _small() as s:
        dirty(s, 400000)                                           # (everything below takes under 100 K floats)
        for case in tail:
            sr, ch, speed, pitch, gain, length, kind = case
            src, ref, roffs = edge_reference(case)
            cid = _upload(s, src, sr)
            arena = s.memory_bytes()[1]
            extent_holds(s, cid, src, (case, "uploaded"))
            s.rerender_clip(cid, gain_db=gain, pitch=pitch, speed=speed)
            holds(s, cid, ref, roffs, case)
            assert ref.shape[1] == s.clip_length(cid)
            extent_holds(s, cid, ref, (case, "rendered"))
            short, soffs = sr_.render(src, sr, gain, pitch, 2.0)
            s.rerender_clip(cid, gain_db=gain, pitch=pitch, speed=2.0)
            holds(s, cid, short, soffs, (case, "shorter"))
            extent_holds(s, cid, short, (case, "shorter"))
            s.rerender_clip(cid)
            assert same_bits(_planar(*s.read_clip(cid)), src)
            extent_holds(s, cid, src, (case, "back to identity"))
            assert s.memory_bytes()[1] == arena
        assert s.memory_bytes()[1] == 4 << 20                      # (it never grew: every extent lay on the noise)


# ---- playback over the tail ------------------------------------------------------------------------------------------------------------
def test_a_voice_plays_a_render_to_its_end_like_the_oracle(built):
    """Hermite mode reads x[pos - 1 .. pos + 2]: near the end of the clip the device reads the zero frames behind the render, which lie
    on noise here.  One unlooped voice over a render of 700 frames, five blocks of 256: the buses equal the oracle's bit for bit
    through the block in which the voice ends, and after it"""
    from libzl_amd.engine import synthetic_clocks
    sr, N, mode = 48000.0, 256, 4
    src = source(sr, 2, 700, seed=41)
    ref, _ = sr_.render(src, sr, 3.0, 3.0, 1.0)                    # (speed 1: the render is as long as the clip's parameters say)
    assert ref.shape == (2, 700)
    osyn = zo.OracleSynth(2, 4, 48000.0, mode)
    with _small(mode=mode) as syn:
        dirty(syn, 20000)
        oid = osyn.register_clip(src[0], src[1], sr)
        cid = syn.register_clip(src[0], src[1], sr)
        osyn.lib.zlo_clip_set_pan(C.byref(osyn.clips[oid]), C.c_float(0.3))
        syn.set_clip_params(cid, snapshot_clip(osyn.clips[oid]))
        syn.rerender_clip(cid, gain_db=3.0, pitch=3.0, speed=1.0)
        extent_holds(syn, cid, ref, "rendered")
        # the oracle's sound plays the restated render
        L, R = np.ascontiguousarray(ref[0]), np.ascontiguousarray(ref[1])
        osyn._buffers += [L, R]
        snd = osyn.sounds[oid]
        snd.L, snd.R, snd.length = L.ctypes.data_as(C.POINTER(C.c_float)), R.ctypes.data_as(C.POINTER(C.c_float)), 700
        osyn.handle_clip_command(oracle_cmd(**play_cmd(oid, midi_channel=-2, loop=False, note=60, volume=0.8)), 0)
        syn.handle_clip_command(engine_cmd(**play_cmd(cid, midi_channel=-2, loop=False, note=60, volume=0.8)), 0)
        playing = []
        for k0, n in ((0, 2), (2, 1), (3, 2)):
            clk = synthetic_clocks(n, N, 48000.0, start_block=k0)
            bus, orep = osyn.render_batch(n, N, clk)
            syn.render_batch(n, N, clk)
            out = syn.read_bus()
            assert np.array_equal(out.view(np.int32), bus.view(np.int32)), (k0, np.abs(out - bus).max())
            assert np.abs(bus).max() > 0.0 or k0 == 3
            rep = syn.voice_reports()
            for v in range(8):
                assert (rep[v].valid, rep[v].gain, rep[v].progress) == (orep[v].valid, orep[v].gain, orep[v].progress), (k0, v)
            playing.append(any(bool(rep[v].playing) for v in range(8)))
            assert playing[-1] == any(bool(osyn.voices[v].isPlaying) for v in range(8)), k0
        assert playing == [True, False, False], playing           # the voice ends in the third block (frames 512 .. 767)
