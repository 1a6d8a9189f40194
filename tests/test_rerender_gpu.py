"""Clip re-render on the device (zlhip_sound_rerender / _batch, zlhip_sound_read): the rendered playback data and the seek offsets
against the numpy restatement (tests/stretch_ref.py) bit for bit; a batch against single calls; playback of a rendered clip and a
voice playing across the swap against the CPU oracle; the swap under the resident real-time kernel; the libzl setters.

The oracle's sound table is plain ctypes: a render is mirrored there by pointing the clip's sound entry at the restated data at the
same block boundary (its voices keep their state and read the new data from their next block, SamplerSynthVoice.cpp:186-191) --
the construction the engine's swap is checked against."""
import ctypes as C

import numpy as np
import pytest

import stretch_ref as sr_
from oracle import zl_oracle as zo
from rerender_cases import cases, same_bits, source
from scenario import engine_cmd, oracle_cmd, play_cmd, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32


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


GRID = cases()


def test_rerender_equals_the_restatement_over_the_grid(syn):
    bad = []
    for (sr, ch, speed, pitch, gain, length) in GRID:
        src = source(sr, ch, length, seed=length + 7 * ch)
        cid = _upload(syn, src, sr)
        syn.rerender_clip(cid, gain_db=gain, pitch=pitch, speed=speed)
        out = _planar(*syn.read_clip(cid))
        ref, roffs = sr_.render(src, sr, gain, pitch, speed)
        offs = syn.rerender_offsets(cid)
        if not (same_bits(out, ref) and np.array_equal(offs.astype(np.int64), roffs)):
            bad.append((sr, ch, speed, pitch, gain, length))
        syn.unregister_clip(cid)
    assert not bad, bad[:10]


@pytest.mark.parametrize("kind", ["zeros", "special"])
def test_all_zero_and_special_values(syn, kind):
    for ch in (1, 2):
        for speed, pitch, gain in [(1.25, 3.0, -6.0), (0.5, -12.0, 0.0), (2.0, 7.0, 3.0), (1.0, -5.0, 0.0), (0.8, 0.0, 3.0)]:
            src = source(48000.0, ch, 24000, seed=5, kind=kind)
            cid = _upload(syn, src, 48000.0)
            syn.rerender_clip(cid, gain_db=gain, pitch=pitch, speed=speed)
            out = _planar(*syn.read_clip(cid))
            ref, roffs = sr_.render(src, 48000.0, gain, pitch, speed)
            assert same_bits(out, ref), (ch, speed, pitch, gain)
            assert np.array_equal(syn.rerender_offsets(cid).astype(np.int64), roffs)
            syn.unregister_clip(cid)


def test_every_render_starts_from_the_original_and_identity_restores_it(syn):
    src = source(44100.0, 2, 30000, seed=3)
    cid = _upload(syn, src, 44100.0)
    total0, arena0 = syn.memory_bytes()
    syn.rerender_clip(cid, gain_db=3.0, pitch=7.0, speed=0.5)
    syn.rerender_clip(cid, gain_db=-6.0, pitch=-5.0, speed=1.25)
    ref, _ = sr_.render(src, 44100.0, -6.0, -5.0, 1.25)
    assert same_bits(_planar(*syn.read_clip(cid)), ref)
    syn.rerender_clip(cid)
    assert same_bits(_planar(*syn.read_clip(cid)), src)
    assert syn.memory_bytes()[1] == arena0
    from libzl_amd import ZlHipError
    for bad in (dict(speed=0.2), dict(speed=4.5), dict(pitch=25.0), dict(gain_db=float("inf")), dict(gain_db=float("nan"))):
        with pytest.raises(ZlHipError):
            syn.rerender_clip(cid, **bad)
    assert same_bits(_planar(*syn.read_clip(cid)), src)
    syn.unregister_clip(cid)


def test_a_full_arena_leaves_the_clip_as_it_was(built):
    from libzl_amd import SamplerSynth, ZlHipError
    with SamplerSynth(num_buses=1, voices_per_bus=1, sound_arena_bytes=1 << 20, sound_arena_max_bytes=1 << 20) as s:
        src = source(48000.0, 2, 60000, seed=4)                   # 0.48 MB of the 1 MB arena; the render at speed 0.5 needs 0.96 MB
        cid = _upload(s, src, 48000.0)
        with pytest.raises(ZlHipError, match="capacity"):
            s.rerender_clip(cid, speed=0.5)
        assert same_bits(_planar(*s.read_clip(cid)), src)
        s.rerender_clip(cid, speed=2.0)                           # (0.24 MB fits)
        assert _planar(*s.read_clip(cid)).shape == (2, 30000)


def test_a_batch_of_64_equals_64_single_calls(syn):
    rng = np.random.default_rng(17)
    params, srcs = [], []
    for i in range(64):
        sr = (44100.0, 48000.0, 96000.0)[i % 3]
        srcs.append((source(sr, 1 + i % 2, int(rng.integers(1, 40000)), seed=100 + i), sr))
        params.append((float(rng.choice([-6.0, 0.0, 3.0])), float(rng.choice([-12.0, -5.0, 0.0, 3.0, 7.0])), float(rng.choice([0.5, 0.8, 1.0, 1.25, 2.0]))))
    ids_b = [_upload(syn, s, sr) for s, sr in srcs]
    ids_s = [_upload(syn, s, sr) for s, sr in srcs]
    syn.rerender_clips(ids_b, [p[0] for p in params], [p[1] for p in params], [p[2] for p in params])
    for cid, p in zip(ids_s, params):
        syn.rerender_clip(cid, *p)
    for a, b in zip(ids_b, ids_s):
        assert same_bits(_planar(*syn.read_clip(a)), _planar(*syn.read_clip(b)))
        assert np.array_equal(syn.rerender_offsets(a), syn.rerender_offsets(b))
    for cid in ids_b + ids_s:
        syn.unregister_clip(cid)


# ---- playback -----------------------------------------------------------------------------------------------------------------

def _pair(mode, L, R, sr, nframes=256):
    from libzl_amd import SamplerSynth
    osyn = zo.OracleSynth(2, 4, 48000.0, mode)
    syn = SamplerSynth(num_buses=2, voices_per_bus=4, mode=mode, max_frames=nframes, max_batch_blocks=16)
    oid = osyn.register_clip(L, R, sr)
    cid = syn.register_clip(L, R, sr)
    assert oid == cid == 0
    osyn.lib.zlo_clip_set_pan(C.byref(osyn.clips[0]), C.c_float(0.3))
    syn.set_clip_params(0, snapshot_clip(osyn.clips[0]))
    for f, tick in ((play_cmd(0, midi_channel=-2, loop=True, note=60, volume=0.8), 0), (play_cmd(0, midi_channel=-1, loop=False, note=64, volume=0.6), 0)):
        osyn.handle_clip_command(oracle_cmd(**f), tick)
        syn.handle_clip_command(engine_cmd(**f), tick)
    return osyn, syn


def _oracle_swap(osyn, planar):
    """the oracle's sound 0 plays `planar` from its next block on"""
    L = np.ascontiguousarray(planar[0]); R = np.ascontiguousarray(planar[1]) if planar.shape[0] == 2 else None
    osyn._buffers += [L, R]
    s = osyn.sounds[0]
    s.L = L.ctypes.data_as(C.POINTER(C.c_float))
    s.R = R.ctypes.data_as(C.POINTER(C.c_float)) if R is not None else None
    s.length = L.shape[0]


@pytest.mark.parametrize("mode", [0, 4], ids=["linear", "hermite"])
@pytest.mark.parametrize("swap_block", [0, 5], ids=["render-then-play", "across-the-swap"])
def test_playback_of_a_rendered_clip_matches_the_oracle(mode, swap_block):
    from libzl_amd.engine import synthetic_clocks
    sr, N = 44100.0, 256
    src = source(sr, 2, 40000, seed=21)
    osyn, syn = _pair(mode, src[0], src[1], sr, N)
    ref, _ = sr_.render(src, sr, -6.0, 3.0, 1.25)
    try:
        for k0, n in ((0, swap_block), (swap_block, 12)):
            if k0 == swap_block:
                syn.rerender_clip(0, gain_db=-6.0, pitch=3.0, speed=1.25)
                _oracle_swap(osyn, ref)
            if n == 0:
                continue
            clk = synthetic_clocks(n, N, 48000.0, start_block=k0)
            bus, orep = osyn.render_batch(n, N, clk)
            syn.render_batch(n, N, clk)
            out = syn.read_bus()
            assert np.array_equal(out.view(np.int32), bus.view(np.int32)), (k0, np.abs(out - bus).max())
            rep = syn.voice_reports()
            for v in range(8):
                assert (rep[v].valid, rep[v].gain, rep[v].progress) == (orep[v].valid, orep[v].gain, orep[v].progress), (k0, v)
                if rep[v].playing:
                    assert rep[v].source_sample_position == osyn.voices[v].sourceSamplePosition, (k0, v)
    finally:
        syn.close()


def test_swap_under_the_resident_kernel_and_back_to_identity():
    from libzl_amd.engine import synthetic_clocks
    sr, N = 48000.0, 128
    src = source(sr, 2, 30000, seed=33)
    osyn, syn = _pair(0, src[0], src[1], sr, N)
    ref, _ = sr_.render(src, sr, 3.0, -5.0, 0.8)
    try:
        _, arena0 = syn.memory_bytes()
        outs = []
        for k in range(30):
            if k == 10:
                syn.rerender_clip(0, gain_db=3.0, pitch=-5.0, speed=0.8)
                _oracle_swap(osyn, ref)
            if k == 20:
                syn.rerender_clip(0)
                _oracle_swap(osyn, src)
                assert syn.memory_bytes()[1] == arena0
            clk = synthetic_clocks(1, N, 48000.0, start_block=k)
            L, R = syn.process(N, clk[0])
            bus, _ = osyn.render_batch(1, N, clk)
            assert np.array_equal(L.view(np.int32), bus[:, 0].view(np.int32)) and np.array_equal(R.view(np.int32), bus[:, 1].view(np.int32)), k
            outs.append(L.copy())
        starts, cycles = syn.rt_stats()
        assert cycles == 30 and starts >= 1
        assert not np.array_equal(outs[12], outs[2])
    finally:
        syn.close()


# ---- the libzl layer ----------------------------------------------------------------------------------------------------------

def _bus_spectrum_peak(zl, nblocks, N=256):
    from libzl_amd.engine import synthetic_clocks
    outL = np.zeros((12, N), f32); outR = np.zeros((12, N), f32)
    acc = []
    for k in range(nblocks):
        clk = synthetic_clocks(1, N, 48000.0, start_block=_bus_spectrum_peak.block)
        _bus_spectrum_peak.block += 1
        assert zl.libzl_hotpath_process(N, clk, outL.ctypes.data, outR.ctypes.data) == 0
        acc.append(outL[0].copy())
    y = np.concatenate(acc).astype(np.float64)
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    return np.argmax(spec) * 48000.0 / len(y), spec.max(), 48000.0 / len(y)


_bus_spectrum_peak.block = 0


def test_libzl_set_pitch_and_gain_are_audible(built):
    from libzl_amd import libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        sr = 48000.0
        sine = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(int(2 * sr)) / sr)).astype(f32)
        c = zl.ClipAudioSource_newFromBuffer(sine.ctypes.data, None, len(sine), sr, b"sine")
        assert c
        # a loop of 3.99 beats at 120 bpm (1.995 s of the 2 s clip): not a whole number of beats, so the voice loops on its position
        zl.ClipAudioSource_setLength(c, 3.99, 120)
        zl.ClipAudioSource_play(c, True)
        _bus_spectrum_peak(zl, 4)
        hz0, mag0, bin_ = _bus_spectrum_peak(zl, 64)
        assert abs(hz0 - 440.0) <= 2 * bin_, hz0
        zl.ClipAudioSource_setPitch(c, 12.0)
        _bus_spectrum_peak(zl, 4)
        hz1, mag1, _ = _bus_spectrum_peak(zl, 64)
        assert abs(hz1 - 880.0) <= 2 * bin_, hz1
        zl.ClipAudioSource_setPitch(c, 0.0)
        zl.ClipAudioSource_setGain(c, -6.0)
        _bus_spectrum_peak(zl, 4)
        hz2, mag2, _ = _bus_spectrum_peak(zl, 64)
        assert abs(hz2 - 440.0) <= 2 * bin_, hz2
        assert abs(mag2 / mag0 - 10 ** (-6.0 / 20.0)) < 0.05 * 10 ** (-6.0 / 20.0), mag2 / mag0
        zl.ClipAudioSource_setSpeedRatio(c, 9.0)                   # clamped to 4
        eng = zl.libzl_hotpath_engine()
        from libzl_amd import _abi
        lib = _abi.load()
        n = C.c_int32(0)
        assert lib.zlhip_sound_read(C.c_void_p(eng), zl.ClipAudioSource_engineClip(c), None, None, 0, C.byref(n)) == 1
        assert n.value == len(sine) // 4
        zl.ClipAudioSource_destroy(c)
    finally:
        zl.shutdownJuce()
