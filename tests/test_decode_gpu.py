"""Clips from raw PCM on the device (zlhip_sound_upload_pcm / _batch, include/zlhip.h): what the engine plays after the upload against
the numpy restatement (tests/decode_ref.py), bit for bit -- over formats, channel counts and lengths at every alignment, with a large
and a tiny staging buffer, from pageable and page-locked memory, special values, the zero frames behind a clip, the finite flag,
whole scenes against the oracle, errors that leave the engine as it was -- and the call's place next to the resident real-time kernel,
in the engine group and behind the libzl-named layer."""
import ctypes as C
import os

import numpy as np
import pytest

import decode_ref as dr
from scenario import Scene, compare_runs, engine_cmd, play_cmd, rand_source, random_scene, run_backend, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32

CHANNELS = (1, 2, 3, 5)
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=512, sound_arena_bytes=64 << 20)
    yield s
    s.close()


@pytest.fixture(scope="module")
def grid():
    """every (format, channels, length) of the grid, once: [(raw bytes, fmt, channels, length, planar reference)]"""
    out = []
    for fmt in dr.FORMATS:
        rng = np.random.default_rng(1000 + fmt)
        for ch in CHANNELS:
            for n in LENGTHS:
                raw = dr.random_raw(rng, fmt, ch, n)
                out.append((raw, fmt, ch, n, dr.decode(raw, fmt, ch)))
    return out


def read_sound(lib, engine, cid):
    """zlhip_sound_read on a bare engine handle -> planar [channels][length]"""
    n = C.c_int32(0)
    ch = lib.zlhip_sound_read(engine, cid, None, None, 0, C.byref(n))
    assert ch in (1, 2)
    L, R = np.zeros(n.value, f32), np.zeros(n.value, f32)
    assert lib.zlhip_sound_read(engine, cid, L.ctypes.data, R.ctypes.data if ch == 2 else None, n.value, None) == ch
    return np.stack([L, R]) if ch == 2 else L[None, :]


def check_grid(syn, grid, frames_of=lambda raw: raw):
    keep = [frames_of(g[0]) for g in grid]
    ids = syn.register_clips_pcm([(k, g[1], g[2], 44100.0 + i) for i, (k, g) in enumerate(zip(keep, grid))])
    try:
        assert ids == sorted(ids) and len(set(ids)) == len(grid)
        bad = []
        for cid, (raw, fmt, ch, n, ref) in zip(ids, grid):
            got = read_sound(syn._lib, syn._e, cid)
            if got.shape != ref.shape or not dr.same(got, ref, fmt):
                bad.append((dr.NAMES[fmt], ch, n))
        assert not bad, bad[:10]
    finally:
        for cid in ids:
            if cid >= 0:
                syn.unregister_clip(cid)


def test_grid_in_one_batch_equals_the_restatement(syn, grid):
    check_grid(syn, grid)


def test_grid_through_a_4096_byte_stage(syn, grid, monkeypatch):
    """many passes, clips cut inside (4099 frames of any format do not fit 4096 bytes)"""
    monkeypatch.setenv("ZL_PCM_STAGE_BYTES", "4096")
    check_grid(syn, grid)


def test_grid_from_page_locked_memory(syn, grid):
    from libzl_amd.engine import pinned_array

    def pinned(raw):
        b = dr.raw_bytes(raw)
        p = pinned_array(syn._lib, (b.size,), np.uint8)
        p[:] = b
        return p
    check_grid(syn, grid, pinned)


F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], u32)
F64_SPECIAL = np.concatenate([
    np.array([0.0, -0.0, 2.0 ** -140, -2.0 ** -140, 2.0 ** -149, 2.0 ** -150, -2.0 ** -150, 2.0 ** -150 * 1.5, 2.0 ** -126, 2.0 ** -127,
              1e300, -1e300, np.finfo(np.float64).max, -np.finfo(np.float64).max, float(np.finfo(f32).max), 2.0 ** 128, 2.0 ** 128 * (1 - 2.0 ** -25),
              1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 - 2.0 ** -25, np.inf, -np.inf, 1.0, -1.0, 0.1], np.float64),
    np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF4000000000000], np.uint64).view(np.float64)])


def test_special_values_through_f32_and_f64(syn):
    """F32: every word comes back with its own bits.  F64: (float)d with denormal results kept, overflow to inf, NaNs by sign."""
    rng = np.random.default_rng(5)
    srcs = []
    for ch in (1, 2, 3):
        a = rng.permutation(np.tile(F32_SPECIAL, 40))[:(700 // ch) * ch].view(f32)
        b = rng.permutation(np.tile(F64_SPECIAL, 30))[:(800 // ch) * ch]
        srcs += [(a, dr.F32, ch), (b, dr.F64, ch)]
    ids = syn.register_clips_pcm([(x, fmt, ch, 48000.0) for x, fmt, ch in srcs])
    for cid, (x, fmt, ch) in zip(ids, srcs):
        got, ref = read_sound(syn._lib, syn._e, cid), dr.decode(x, fmt, ch)
        assert dr.same(got, ref, fmt), (dr.NAMES[fmt], ch)
        if fmt == dr.F32 and ch == 1:
            assert np.array_equal(got[0].view(u32), x.view(u32))   # no float operation touched them
        syn.unregister_clip(cid)
    # by value, one at a time in their listed order
    cid = syn.register_clip_pcm(F64_SPECIAL, dr.F64, 1, 48000.0)
    got = read_sound(syn._lib, syn._e, cid)[0]
    syn.unregister_clip(cid)
    bits = got.view(u32)
    assert bits[2] == 1 << 9 and bits[3] == 0x80000000 | 1 << 9 and bits[4] == 1 and bits[5] == 0      # 2^-140 stays denormal; 2^-150 ties to zero
    assert np.isposinf(got[10]) and np.isneginf(got[11]) and bits[14] == 0x7F7FFFFF and np.isposinf(got[15])
    assert np.isnan(got[-4:]).all() and list(bits[-4:] >> 31) == [0, 1, 0, 1]


def _past_the_end_scene(planes, neighbour):
    """the shape of the golden g7_past_the_end_q10: a loop longer than its file and a one-shot that runs off the end of clip 0"""
    sc = Scene(num_buses=1, voices_per_bus=4, fs=48000.0, mode=0, nframes=128, nblocks=12)
    sc.sounds = [(planes[0], planes[1], 48000.0), (neighbour[0], neighbour[1], 48000.0)]

    def setup(lib, clip):
        clip.lengthInBeats = 0.25
        clip.lengthInSeconds = float(f32(0.03))                    # 1440 frames of a 500-frame file
        lib.zlo_clip_set_volume_absolute(clip, C.c_float(0.8))
        lib.zlo_clip_set_pan(clip, C.c_float(0.25))
        clip.adsr.p.attack, clip.adsr.p.decay, clip.adsr.p.sustain, clip.adsr.p.release = (0.0, 0.1, 1.0, 0.0)
    sc.clip_setup[0] = setup
    sc.events[0] = [("cmd", play_cmd(0, loop=False, note=57, volume=0.9), 0), ("cmd", play_cmd(0, midi_channel=-2, loop=True, note=60, volume=0.7), 0),
                    ("cmd", play_cmd(0, loop=False, note=60, volume=0.5), 0)]
    return sc


def test_the_pad_behind_a_clip_is_zero_and_the_neighbour_is_untouched(built):
    """a clip of all 1.0, a neighbour behind it; the first is released and a shorter S16 clip lands in the freed extent: its zero
    frames lie where 1.0 was.  Voices played past the new clip's end read them: a stale 1.0 differs from the oracle."""
    from libzl_amd import SamplerSynth
    rng = np.random.default_rng(77)
    ones = np.ones((600, 2), f32)
    nb_raw = dr.random_raw(rng, dr.S24, 2, 700)
    nb = dr.decode(nb_raw, dr.S24, 2)
    raw = dr.random_raw(rng, dr.S16, 2, 500)
    planes = dr.decode(raw, dr.S16, 2)
    sc = _past_the_end_scene(planes, nb)

    class Loader(SamplerSynth):
        def register_clip(self, left, right, sample_rate):
            if np.array_equal(left, planes[0]):
                a = self.register_clip_pcm(ones, dr.F32, 2, sample_rate)
                b = self.register_clip_pcm(nb_raw, dr.S24, 2, sample_rate)
                assert (a, b) == (0, 1)
                self.unregister_clip(a)
                c = self.register_clip_pcm(raw, dr.S16, 2, sample_rate)
                assert c == 0                                      # the freed slot, and (first fit) the freed extent
                assert dr.same(np.stack(self.read_clip(c)), planes, dr.S16)
                return c
            assert dr.same(np.stack(self.read_clip(1)), nb, dr.S24)                   # the neighbour, after the upload in front of it
            return 1

    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    bus, rep, s, _ = run_backend(sc, Loader, batch=4)
    try:
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, 4)
        assert np.abs(bus[:, :, 600:]).max() > 0.0                 # the loop goes on after the file's end
        assert dr.same(np.stack(s.read_clip(1)), nb, dr.S24)
    finally:
        s.close()


def _nan_aware_equal(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


@pytest.mark.parametrize("fmt", [dr.F32, dr.F64], ids=["f32_inf", "f64_1e300"])
def test_a_non_finite_source_does_not_get_the_finite_flag(built, fmt):
    """on-grid unit-step loops (note 60 at the engine's rate) of four clips, one of which holds an inf -- an F64 of 1e300 is one after
    the conversion.  With ZL_SOUND_FINITE wrongly set K2 would drop the second tap and with it the oracle's inf * 0 = NaN frames.
    Against the oracle NaN frames compare as NaN frames (an invalid operation's NaN has the platform's sign and payload, see
    tests/test_k2_ongrid.py); against the same engine with the clip loaded through zlhip_sound_upload every bit agrees."""
    from libzl_amd import SamplerSynth
    rng = np.random.default_rng(31 + fmt)
    dtype = f32 if fmt == dr.F32 else np.float64
    raws = []
    for i in range(4):
        x = rng.uniform(-1.0, 1.0, (3000 + 101 * i, 2)).astype(dtype)
        if i == 1:
            x[700, 0] = np.inf if fmt == dr.F32 else 1e300
            x[1500, 1] = -np.inf if fmt == dr.F32 else -1e300
        raws.append(x)
    planes = [dr.decode(x, fmt, 2) for x in raws]
    assert [dr.finite(p) for p in planes] == [True, False, True, True]
    sc = Scene(num_buses=1, voices_per_bus=4, fs=48000.0, mode=0, nframes=256, nblocks=40)
    for i, p in enumerate(planes):
        sc.sounds.append((p[0], p[1], 48000.0))

        def setup(lib, clip, i=i):
            lib.zlo_clip_set_length(clip, C.c_float(0.1 + 0.02 * i), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(0.5 + 0.1 * i))
            lib.zlo_clip_set_pan(clip, C.c_float(-0.3 + 0.2 * i))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=-2, loop=True, note=60, volume=0.8), 0) for i in range(4)]

    class Loader(SamplerSynth):
        def register_clip(self, left, right, sample_rate):
            i = next(k for k, p in enumerate(planes) if p[0] is left or np.array_equal(p[0].view(u32), left.view(u32)))
            return self.register_clip_pcm(raws[i], fmt, 2, sample_rate)

    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    assert np.isnan(ref_bus).any()
    bus, rep, s, _ = run_backend(sc, Loader)
    s.close()
    plain, _, s2, _ = run_backend(sc, SamplerSynth)
    s2.close()
    assert _nan_aware_equal(ref_bus, bus)
    assert np.array_equal(bus.view(np.int32), plain.view(np.int32))


def test_a_scene_loaded_as_s16_and_s24_equals_the_oracle(built):
    from libzl_amd import SamplerSynth
    sc = random_scene(9102, num_buses=3, voices_per_bus=8, nclips=10, nframes=128, nblocks=24)
    rng = np.random.default_rng(4)
    raws = []
    for i, (L, R, sr) in enumerate(sc.sounds):
        ch, fmt = (2 if R is not None else 1), (dr.S16 if i % 2 else dr.S24)
        raw = dr.random_raw(rng, fmt, ch, L.shape[0])
        p = dr.decode(raw, fmt, ch)
        raws.append((raw, fmt, ch))
        sc.sounds[i] = (p[0], p[1] if ch == 2 else None, sr)

    class Loader(SamplerSynth):
        def register_clip(self, left, right, sample_rate):
            i = next(k for k, s in enumerate(sc.sounds) if s[0] is left)
            return self.register_clip_pcm(*raws[i], sample_rate)

    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    bus, rep, s, _ = run_backend(sc, Loader, batch=8)
    s.close()
    compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, 24)


def test_a_failing_batch_leaves_the_engine_as_it_was(built):
    from libzl_amd import SamplerSynth, _abi
    INV, CAP = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY
    arena = 1 << 20
    with SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=8, sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        x = np.random.default_rng(1).integers(-30000, 30000, (1000, 2)).astype(np.int16)
        first = s.register_clip_pcm(x, dr.S16, 2, 48000.0)         # (the stage exists from here on)
        assert first == 0
        mem = s.memory_bytes()
        P = _abi.PcmSource
        good = P(x.ctypes.data, 1000, 2, dr.S16, 0, 48000.0)

        def batch(*srcs, count=None):
            arr = (P * max(1, len(srcs)))(*srcs)
            ids = (C.c_int32 * max(1, len(srcs)))(*[77] * max(1, len(srcs)))
            rc = lib.zlhip_sound_upload_pcm_batch(e, arr, len(srcs) if count is None else count, ids)
            return rc, list(ids)[:len(srcs)]

        bads = [P(None, 1000, 2, dr.S16, 0, 48000.0), P(x.ctypes.data, 1000, 2, 0, 0, 48000.0), P(x.ctypes.data, 1000, 2, 7, 0, 48000.0),
                P(x.ctypes.data, 1000, 0, dr.S16, 0, 48000.0), P(x.ctypes.data, 10, 65, dr.S16, 0, 48000.0), P(x.ctypes.data, 0, 2, dr.S16, 0, 48000.0),
                P(x.ctypes.data, -3, 2, dr.S16, 0, 48000.0), P(x.ctypes.data, 1000, 2, dr.S16, 0, 0.0), P(x.ctypes.data, 1000, 2, dr.S16, 0, -1.0),
                P(x.ctypes.data, 1000, 2, dr.S16, 1, 48000.0)]
        for k, b in enumerate(bads):
            for srcs in ((good, b, good), (b,), (good, good, b)):
                rc, ids = batch(*srcs)
                assert rc == INV and ids == [-1] * len(srcs), (k, rc, ids)
        assert b"sound_upload_pcm" in lib.zlhip_last_error(e)
        assert batch(good, count=-1)[0] == INV
        assert lib.zlhip_sound_upload_pcm_batch(e, None, 0, None) == 0                 # nothing to do
        out = C.c_int32(5)
        assert lib.zlhip_sound_upload_pcm(e, x.ctypes.data, 9, 2, 1000, 48000.0, C.byref(out)) == INV and out.value == -1
        # more clips than free slots (7 are free)
        rc, ids = batch(*[good] * 8)
        assert rc == CAP and ids == [-1] * 8
        # more samples than the fixed arena holds: the first two fit, the third does not
        big = np.zeros((60000, 2), f32)                            # 480 KB each
        bigsrc = P(big.ctypes.data, 60000, 2, dr.F32, 0, 48000.0)
        rc, ids = batch(bigsrc, good, bigsrc, bigsrc)
        assert rc == CAP and ids == [-1] * 4
        assert s.memory_bytes() == mem
        # the engine is as it was: the next uploads get the ids and the room they would have got
        y = np.random.default_rng(2).uniform(-1, 1, 1000).astype(f32)
        assert s.register_clip(y, None, 48000.0) == 1
        rc, ids = batch(bigsrc, good, bigsrc)
        assert rc == 0 and ids == [2, 3, 4]
        assert dr.same(np.stack(s.read_clip(3)), dr.decode(x, dr.S16, 2), dr.S16) and dr.same(np.stack(s.read_clip(0)), dr.decode(x, dr.S16, 2), dr.S16)
        assert np.array_equal(s.read_clip(1)[0], y) and not np.stack(s.read_clip(4)).any()
        assert s.memory_bytes() == mem


@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_an_upload_between_real_time_cycles(built, rt_env):
    """three clips go up in ONE batch call between two zlhip_render cycles: the resident kernel leaves once and is started once more
    (not once per clip), the clips play from the next cycle on, every cycle is the oracle's bit for bit"""
    from libzl_amd import SamplerSynth
    from oracle import zl_oracle as zo
    sc = random_scene(517, num_buses=12, voices_per_bus=8, nclips=8, mode=0, nframes=128, nblocks=24, events=False)
    rng = np.random.default_rng(6)
    base, at = len(sc.sounds), 10
    extra = []
    for i, (fmt, ch) in enumerate([(dr.S16, 2), (dr.S24, 1), (dr.F32, 2)]):
        raw = dr.random_raw(rng, fmt, ch, 5000 + 37 * i)
        p = dr.decode(raw, fmt, ch)
        extra.append((raw, fmt, ch, 48000.0))
        sc.sounds.append((p[0], p[1] if ch == 2 else None, 48000.0))

        def setup(lib, clip, i=i):
            lib.zlo_clip_set_length(clip, C.c_float(0.05 + 0.01 * i), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(0.6))
        sc.clip_setup[base + i] = setup
    sc.events[at] = [("cmd", play_cmd(base + i, midi_channel=i - 2, loop=True, note=60 + i, volume=0.7), 0) for i in range(3)]
    ref_bus, _, _ = run_oracle(sc)
    ref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    syn = SamplerSynth(num_buses=sc.num_buses, voices_per_bus=sc.voices_per_bus, mode=sc.mode, playback_sample_rate=sc.fs,
                       max_frames=128, max_batch_blocks=4, max_sounds=16, sound_arena_bytes=4 << 20)
    try:
        for i, (L, R, sr) in enumerate(sc.sounds):
            assert ref.register_clip(L, R, sr) == i
            if i in sc.clip_setup:
                sc.clip_setup[i](ref.lib, ref.clips[i])
            if i < base:
                assert syn.register_clip(L, R, sr) == i
                syn.set_clip_params(i, snapshot_clip(ref.clips[i]))
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts = []
        for k in range(sc.nblocks):
            if k == at:
                assert syn.register_clips_pcm(extra) == [base, base + 1, base + 2]
                for i in range(3):
                    syn.set_clip_params(base + i, snapshot_clip(ref.clips[base + i]))
            for ev in sc.events.get(k, []):
                assert ev[0] == "cmd"
                syn.handle_clip_command(engine_cmd(**ev[1]), ev[2])
            L, R = syn.process(N, sc.make_clocks(k, 1)[0])
            out[:, 0, k * N:(k + 1) * N] = L
            out[:, 1, k * N:(k + 1) * N] = R
            starts.append(syn.rt_stats()[0])
        assert starts[0] == 1 and starts[at - 1] == 1 and starts[at] == 2 and starts[-1] == 2, starts
        assert syn.rt_stats() == (2, sc.nblocks)
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
        assert np.abs(out[:, :, at * N:] - 0).max() > 0
    finally:
        syn.close()


def test_group_broadcast_in_one_call(built):
    from libzl_amd import SamplerSynthGroup
    rng = np.random.default_rng(8)
    srcs = [(dr.random_raw(rng, fmt, ch, n), fmt, ch, 44100.0) for fmt, ch, n in
            [(dr.S16, 2, 4099), (dr.S24, 1, 257), (dr.U8, 3, 1000), (dr.F64, 2, 63), (dr.S32, 5, 9), (dr.F32, 1, 1)]]
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        y = rng.uniform(-1, 1, 100).astype(f32)
        assert g.register_clip(y, None, 48000.0) == 0
        ids = g.register_clips_pcm(srcs)
        assert ids == [1, 2, 3, 4, 5, 6]                           # the same on both members
        for r in range(2):
            for cid, (raw, fmt, ch, _) in zip(ids, srcs):
                assert dr.same(read_sound(g._lib, g.member(r), cid), dr.decode(raw, fmt, ch), fmt), (r, cid)
        assert g.clip_length(1) == 4099
        from libzl_amd import ZlHipError
        with pytest.raises(ZlHipError, match="member 0"):
            g.register_clips_pcm([(srcs[0][0], dr.S16, 2, 0.0)])
        assert g.register_clip(y, None, 48000.0) == 7              # the failed call took no slot on any member


def _wavs(tmp_path):
    rng = np.random.default_rng(11)
    out = []
    for i, (fmt, ch) in enumerate([(dr.U8, 1), (dr.S16, 2), (dr.S16, 3), (dr.S24, 1), (dr.S24, 3), (dr.S32, 2), (dr.F32, 2), (dr.F64, 1), (dr.F64, 3)]):
        n = 1001 + 13 * i
        raw = dr.random_raw(rng, fmt, ch, n)
        path = str(tmp_path / f"{dr.NAMES[fmt]}_{ch}.wav")
        dr.write_wav(path, raw, fmt, ch, 44100 if i % 2 else 48000, extensible=(fmt, ch) == (dr.S24, 3))
        out.append((path, dr.decode(raw, fmt, ch), fmt))
    return out


def test_libzl_layer_loads_files_on_the_device(built, tmp_path, monkeypatch):
    """ClipAudioSource_new with ZL_PCM_DECODE unset (the data chunk decoded on the device) and = 0 (libzl_wav_read on the host): the
    same playback data, the restatement's; a bank through libzl_hotpath_clips_new with one missing file among good ones"""
    from libzl_amd import libzl
    zl = libzl.load()
    wavs = _wavs(tmp_path)
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        e = zl.libzl_hotpath_engine()
        seen = {}
        for route in (None, "0"):
            if route is None:
                monkeypatch.delenv("ZL_PCM_DECODE", raising=False)
            else:
                monkeypatch.setenv("ZL_PCM_DECODE", route)
            for path, ref, fmt in wavs:
                c = zl.ClipAudioSource_new(path.encode(), False)
                assert c, path
                got = read_sound(zl, e, zl.ClipAudioSource_engineClip(c))
                assert dr.same(got, ref, fmt), (route, path)
                seen.setdefault(path, []).append(got.view(u32).copy())
        for path, both in seen.items():
            assert np.array_equal(both[0], both[1]), path
        monkeypatch.delenv("ZL_PCM_DECODE", raising=False)
        paths = [w[0] for w in wavs[:4]] + [str(tmp_path / "missing.wav")] + [w[0] for w in wavs[4:]]
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        out = (C.c_void_p * len(paths))()
        assert zl.libzl_hotpath_clips_new(arr, len(paths), out) == len(wavs)
        assert out[4] is None
        k = 0
        for i, p in enumerate(paths):
            if i == 4:
                continue
            assert out[i], p
            assert dr.same(read_sound(zl, e, zl.ClipAudioSource_engineClip(out[i])), wavs[k][1], wavs[k][2]), p
            k += 1
        eng = [zl.ClipAudioSource_engineClip(out[i]) for i in range(len(paths)) if i != 4]
        assert eng == list(range(eng[0], eng[0] + len(eng)))       # one batch: consecutive slots in request order
    finally:
        zl.shutdownJuce()
