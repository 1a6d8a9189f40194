"""Sample-rate conversion on the device (zlhip_sound_convert_rate / _batch, include/zlhip.h): what the engine holds after the call
against the numpy restatement (tests/resample_ref.py) fed the library's own table, bit for bit -- mixed rates, mono and stereo and
lengths in one batch, the zero frames behind every extent, the neighbours in the arena -- then what it plays (the table swap, the host
mirror's rate, the finite flag), errors that leave every clip as it was, the call's place next to the resident real-time kernel, in the
engine group and behind the libzl-named layer.  Small engines: 2 buses x 8 voices, 256-frame blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as rr

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
FT = 48000


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


@pytest.fixture(scope="module")
def syn(built):
    s = make()
    yield s
    s.close()


_tables = {}


def table(fs, ft=FT):
    """the LIBRARY's table of the ratio (zlhip_resample_design), [L, row] float32"""
    from libzl_amd import _abi
    if (fs, ft) not in _tables:
        lib = _abi.load()
        L, row = C.c_int32(0), C.c_int32(0)
        assert lib.zlhip_resample_design(fs, ft, C.byref(L), None, None, C.byref(row), None, 0) == 0
        t = np.zeros((L.value, row.value), f32)
        assert lib.zlhip_resample_design(fs, ft, None, None, None, None, t.ctypes.data, t.size) == 0
        _tables[(fs, ft)] = t
    return _tables[(fs, ft)]


def source(rng, n, ch):
    x = rng.uniform(-1.0, 1.0, (n, ch)).astype(f32)
    special = np.array([0.0, -0.0, 1e-39, -1e-39, 1.0, -1.0], f32)
    at = rng.integers(0, n, size=max(1, n // 7))
    x[at, rng.integers(0, ch, size=at.size)] = special[rng.integers(0, special.size, size=at.size)]
    return x


def upload(s, x, rate):
    return s.register_clip(x[:, 0].copy(), x[:, 1].copy() if x.shape[1] == 2 else None, float(rate))


def read(s, cid):
    """[length, channels]"""
    L, R = s.read_clip(cid)
    return np.stack([L, R], axis=1) if R is not None else L[:, None]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def expected(x, fs, ft=FT):
    return rr.convert(table(fs, ft), fs, ft, x)


def dirty(s, floats):
    """noise over the first `floats` floats of a fresh arena, released again: what is allocated next lies on it, so that a float of an
    extent that nobody writes does not read as zero by luck"""
    x = np.random.default_rng(99).uniform(1.0, 2.0, floats - 8).astype(f32)
    cid = s.register_clip(x, None, float(FT))
    s.unregister_clip(cid)


def uploaded_extent_is(s, cid, x):
    """the extent of a clip that zlhip_sound_upload wrote: its frames and the 8 zero frames behind them (that call does not write the
    floats between there and the 16-byte boundary, which nothing reads)"""
    n = (x.shape[0] + 8) * x.shape[1]
    return same(s.clip_extent(cid)[:n], rr.extent(x)[:n])


def set_loop(s, cid, frames, rate=float(FT)):
    """the clip's parameters with a loop of 750 frames (ClipAudioSource::setLength(0.04 beats, 120 bpm) = 1/64 s; `rate`: the engine's,
    where it is not 48000): with the default length -- the whole clip, no beat length -- a looping voice under a stopped SyncTimer
    holds its first frame"""
    p = s.default_clip_params(frames / rate)
    p.length_seconds = 0.015625
    p.length_in_beats = 0.04
    s.set_clip_params(cid, p)


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------
def test_a_mixed_batch_equals_the_restatement_bit_for_bit(syn):
    """one call: four source rates (a table each), one clip already at 48000 (skipped), mono and stereo, lengths 1, 65, 1000 and the
    one that gives 257 output frames (258 where the ratio skips 257).  The extents are read back whole (zlhip_debug_sound_extent) from
    an arena that held noise: the 8 frames behind every clip and the floats up to the 16-byte boundary are zero because the kernel
    wrote them"""
    dirty(syn, 200000)                                             # (the sources and their conversions take 40 K floats)
    rng = np.random.default_rng(21)
    cases = []
    for k, fs in enumerate((44100, 96000, 8000, 22050)):
        for m, n in enumerate((1, 65, 1000, rr.lengths_for(fs, FT, 257)[-1])):
            cases.append((fs, 1 + (k + m) % 2, n))
    cases.insert(5, (48000, 2, 300))
    srcs = [source(rng, n, ch) for fs, ch, n in cases]
    ids = [upload(syn, x, fs) for x, (fs, ch, n) in zip(srcs, cases)]
    before = syn.memory_bytes()
    syn.convert_clips(ids, FT)
    assert syn.memory_bytes()[0] > before[0]                       # the filter tables are counted
    for cid, x, (fs, ch, n) in zip(ids, srcs, cases):
        info = syn.clip_info(cid)
        if fs == FT:
            assert same(read(syn, cid), x) and info["length"] == n and info["sample_rate"] == FT
            continue
        ref = expected(x, fs)
        assert info == {"length": ref.shape[0], "channels": ch, "sample_rate": float(FT), "finite": True, "rendered": False}, (fs, ch, n, info)
        assert info["length"] == rr.out_frames(fs, FT, n)
        got = read(syn, cid)
        assert same(got, ref), (fs, ch, n, np.argwhere(got.view(u32) != ref.view(u32))[:6] if got.shape == ref.shape else got.shape)
        ext, want = syn.clip_extent(cid), rr.extent(ref)
        assert ext.size == want.size >= (ref.shape[0] + 8) * ch and not want[ref.shape[0] * ch:].any()
        assert same(ext, want), (fs, ch, n, np.flatnonzero(ext.view(u32) != want.view(u32))[:8])
    again = syn.memory_bytes()
    syn.convert_clips(ids, FT)                                     # every clip is at the rate: nothing to do, nothing allocated
    assert syn.memory_bytes() == again
    syn.convert_clips(ids[:3], None)                               # None / 0: the engine's own rate
    assert syn.memory_bytes() == again
    for cid in ids:
        syn.unregister_clip(cid)


def test_the_frames_behind_a_converted_clip_are_zero_and_the_neighbours_unharmed(built):
    """three clips adjacent in an arena that held noise; the middle one is converted into the room behind them, a fourth clip takes the
    room the middle one left and a fifth the room right behind the converted extent: the neighbours read back unchanged, extents
    included, and the converted extent ends in zeros.  Played once, unlooped, the converted clip renders what the restatement's output
    uploaded at 48000 renders"""
    from scenario import engine_cmd, play_cmd
    from libzl_amd.engine import synthetic_clocks
    rng = np.random.default_rng(22)
    with make() as s:
        dirty(s, 100000)
        a, b, c = (source(rng, n, 2) for n in (500, 441, 700))
        ia, ib, ic = upload(s, a, FT), upload(s, b, 44100), upload(s, c, FT)
        ea, ec = s.clip_extent(ia), s.clip_extent(ic)
        assert uploaded_extent_is(s, ia, a) and uploaded_extent_is(s, ic, c)
        s.convert_clips([ib])
        ref = expected(b, 44100)
        assert same(read(s, ib), ref) and same(s.clip_extent(ib), rr.extent(ref))
        d, g = source(rng, 441, 2), source(rng, 300, 2)
        idd = upload(s, d, FT)                                     # (first fit: the extent the middle clip left)
        ig = upload(s, g, FT)                                      # (right behind the converted extent)
        assert uploaded_extent_is(s, idd, d) and uploaded_extent_is(s, ig, g)
        assert same(s.clip_extent(ib), rr.extent(ref)) and same(s.clip_extent(ia), ea) and same(s.clip_extent(ic), ec)
        # play the converted clip once, unlooped, to its end and beyond, next to the restatement's output uploaded at 48000
        it = upload(s, ref, FT)
        for bus, cid in ((0, ib), (1, it)):
            s.handle_clip_command(engine_cmd(**play_cmd(cid, midi_channel=bus - 2, loop=False, note=60, volume=1.0)), 0)
        s.render_batch(4, 256, synthetic_clocks(4, 256, float(FT)))
        bus = s.read_bus()
        assert same(bus[0], bus[1]) and len(np.unique(bus[0][0, :480])) > 400   # (it moves through the clip)
        assert not bus[0][:, 768:].any()                           # (480 frames: silence long before the last block)


# ---- playback -------------------------------------------------------------------------------------------------------------------
def play_pair(s, converted, twin, blocks=8, loop=True, rate=float(FT)):
    """clip `converted` on bus 0, clip `twin` on bus 1, one voice each, the same command: (bus [2][2][frames], peaks, levels, reports);
    `rate`: the engine's, where it is not 48000"""
    from scenario import engine_cmd, play_cmd
    from libzl_amd.engine import synthetic_clocks
    for bus, cid in ((0, converted), (1, twin)):
        set_loop(s, cid, s.clip_info(cid)["length"], rate)
        assert s.handle_clip_command(engine_cmd(**play_cmd(cid, midi_channel=bus - 2, loop=loop, note=60, volume=0.8)), 0) == 1
    s.render_batch(blocks, 256, synthetic_clocks(blocks, 256, rate))
    bus = s.read_bus()
    peaks = s.block_peaks()
    lv = s.levels_tick()
    rep = s.voice_reports()
    fields = ("playing", "valid", "gain", "progress", "source_sample_position")
    reports = [[tuple(getattr(rep[b * 8 + v], f) for f in fields) for v in range(8)] for b in range(2)]
    levels = [tuple(getattr(lv[b], f) for f, _ in type(lv[b])._fields_) for b in range(2)]
    return bus, peaks, levels, reports


def test_a_converted_clip_plays_like_its_uploaded_twin(built):
    """a 44.1 kHz clip converted on the device, looped on one voice for 8 blocks, against the restatement's output uploaded at 48000 in
    the same engine: bus, levels and reports bit for bit (the table swap, the host mirror's rate -- a wrong one would step the voice at
    0.91875 -- and the flag).  1176 = 8 * 147 frames become 1280: both clips last 1/37.5 s exactly, the loop wraps once."""
    rng = np.random.default_rng(23)
    with make() as s:
        x = source(rng, 1176, 2)
        cid = upload(s, x, 44100)
        s.convert_clips([cid])
        ref = expected(x, 44100)
        assert ref.shape[0] == 1280
        twin = upload(s, ref, FT)
        assert s.clip_info(cid) == s.clip_info(twin)
        bus, peaks, levels, reports = play_pair(s, cid, twin)
        assert len(np.unique(bus[0][0])) > 700                      # (it moves through the loop: 750 frames)
        assert same(bus[0], bus[1])
        assert np.array_equal(peaks[:, 0], peaks[:, 1]) and levels[0] == levels[1] and reports[0] == reports[1]
        assert reports[0][0][0] == 1 and 0 < reports[0][0][4] < 751        # still looping, inside the loop


def nan_same(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(a[~an].view(u32), b[~bn].view(u32))


def test_a_non_finite_clip_converts_without_the_flag_and_still_plays(built):
    """an F32 clip with one +inf: finite == 0, so the clip plays on the two-tap path; it matches the uploaded twin.  NaN payloads
    differ between the host and the device: NaNs are compared as NaNs, every other sample bit for bit, and the stored clip beyond `half`
    input frames from the +inf bit for bit."""
    from libzl_amd import _abi
    rng = np.random.default_rng(24)
    with make() as s:
        x = source(rng, 1176, 2)
        x[600, 0] = np.inf
        cid = s.register_clip_pcm(np.ascontiguousarray(x), _abi.PCM_F32, 2, 44100.0)
        assert s.clip_info(cid)["finite"] is False
        s.convert_clips([cid])
        info = s.clip_info(cid)
        assert info["finite"] is False and info["length"] == 1280 and info["sample_rate"] == FT
        ref = expected(x, 44100)
        got = read(s, cid)
        far = np.abs((np.arange(1280, dtype=np.int64) * 147) // 160 - 600) > 32
        assert same(got[far], ref[far]) and same(got[:, 1], ref[:, 1]) and nan_same(got, ref)
        assert not np.isfinite(got[~far, 0]).all()
        twin = upload(s, ref, FT)
        assert s.clip_info(twin)["finite"] is False
        bus, peaks, levels, reports = play_pair(s, cid, twin)
        assert nan_same(bus[0], bus[1]) and np.isnan(bus[0]).any()
        assert reports[0] == reports[1] or all(nan_same(np.array(p, np.float64), np.array(q, np.float64)) for p, q in zip(reports[0], reports[1]))


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_every_clip_as_it_was(built):
    from libzl_amd import _abi
    INV, CAP, STATE = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY, _abi.ZLHIP_ERR_STATE
    rng = np.random.default_rng(25)
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        a, b, c = source(rng, 2000, 2), source(rng, 3000, 1), source(rng, 1500, 2)
        ia, ib = upload(s, a, 44100), upload(s, b, 22050)
        ic = upload(s, c, 47999)                                   # 47999 -> 48000: L = 48000, beyond the limits
        big = source(rng, 60000, 2)                                # 480 KB; converted 522 KB: the arena (1 MiB) cannot take it
        ibig = upload(s, big, 44100)

        def call(ids, rate=float(FT), count=None):
            arr = (C.c_int32 * max(1, len(ids)))(*ids)
            return lib.zlhip_sound_convert_rate_batch(e, arr, len(ids) if count is None else count, rate)

        s.convert_clips([ia])                                      # (the call's records and the 44.1 table exist from here on)
        s.rerender_clip(ia, gain_db=0.0, pitch=0.0, speed=1.0)
        a48 = expected(a, 44100)
        assert same(read(s, ia), a48)
        a = a48                                                    # what "unchanged" means for clip a from now on

        def unchanged():
            return (same(read(s, ia), a) and same(read(s, ib), b) and same(read(s, ic), c) and same(read(s, ibig), big)
                    and [s.clip_info(i)["sample_rate"] for i in (ia, ib, ic, ibig)] == [48000.0, 22050.0, 47999.0, 44100.0])

        mem = s.memory_bytes()
        # an invalid ratio in a batch, ids out of range, free or repeated, a bad count, a bad target
        for ids in ([ib, ic], [ic], [ib, 31], [ib, -1], [ib, ib], [ib, 99]):
            assert call(ids) == INV, ids
        assert b"sound_convert_rate" in lib.zlhip_last_error(e)
        assert call([ib], count=-1) == INV and call([ib], rate=48000.5) == INV and call([ib], rate=500.0) == INV
        assert lib.zlhip_sound_convert_rate(e, ic, 0.0) == INV
        assert call([], count=0) == 0
        assert unchanged() and s.memory_bytes() == mem
        assert call([ic], rate=47999.0) == 0                       # already at the target, whatever the target: skipped, not judged
        assert unchanged() and s.memory_bytes() == mem
        # a clip that plays a re-render
        s.rerender_clip(ib, gain_db=-6.0)
        bre = read(s, ib)
        assert s.clip_info(ib)["rendered"] is True
        mem = s.memory_bytes()                                     # (the re-render allocated its own records and the rendered extent)
        assert call([ia, ib], rate=44100.0) == STATE and call([ib]) == STATE
        assert s.memory_bytes() == mem
        assert same(read(s, ib), bre) and s.clip_info(ia)["sample_rate"] == FT and same(read(s, ia), a)
        s.rerender_clip(ib)                                        # back to the original
        assert unchanged()
        mem = s.memory_bytes()
        # an arena that cannot hold the call: the small clip of the call fits, the big one does not -- neither is converted, and the
        # table of the small clip's ratio (22050 -> 48000: new to this engine) that the call had made is freed again
        assert call([ib, ibig]) == CAP
        assert unchanged() and s.memory_bytes() == mem
        # after the errors: the call still works, and a re-render of a converted clip starts from the converted data
        s.convert_clips([ib])
        b48 = expected(b, 22050)
        assert same(read(s, ib), b48)
        s.rerender_clip(ib, gain_db=-6.0)
        g = f32(10.0 ** (-6.0 / 20.0))
        got = read(s, ib)
        assert got.shape == b48.shape and np.allclose(got, b48 * g, rtol=1e-6, atol=1e-9)
        assert s.clip_info(ib) == {"length": b48.shape[0], "channels": 1, "sample_rate": 48000.0, "finite": False, "rendered": True}
        s.rerender_clip(ib)
        assert same(read(s, ib), b48) and s.clip_info(ib)["finite"] is True


# ---- next to the resident real-time kernel --------------------------------------------------------------------------------------
@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_a_conversion_between_real_time_cycles_costs_one_restart(built, rt_env):
    from scenario import engine_cmd, play_cmd
    from libzl_amd.engine import synthetic_clocks
    rng = np.random.default_rng(26)
    with make() as s:
        xs = [source(rng, 1176, 2) for _ in range(3)]
        ids = [upload(s, x, 44100) for x in xs]
        clocks = synthetic_clocks(8, 256, float(FT))
        starts = []
        for k in range(8):
            if k == 4:
                s.convert_clips(ids)                               # three clips, one call
                set_loop(s, ids[0], 1280)
                s.handle_clip_command(engine_cmd(**play_cmd(ids[0], midi_channel=-2, loop=True, note=60, volume=0.8)), 0)
            L, R = s.process(256, clocks[k])
            starts.append(s.rt_stats()[0])
            if k == 4:
                first = np.stack([L[0], R[0]])
        assert starts == [1, 1, 1, 1, 2, 2, 2, 2], starts
        assert s.rt_stats() == (2, 8)
        ref = expected(xs[0], 44100)
        assert len(np.unique(first[0])) > 200 and [s.clip_info(i)["length"] for i in ids] == [1280] * 3
        assert same(read(s, ids[0]), ref)


# ---- the group, the libzl-named layer -------------------------------------------------------------------------------------------
def test_group_converts_on_every_member(built):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    rng = np.random.default_rng(27)
    with SamplerSynthGroup([0, 0], 4, 8, max_frames=256, max_batch_blocks=8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        xs = [(source(rng, 1000, 2), 44100), (source(rng, 257, 1), 96000), (source(rng, 300, 2), 48000)]
        ids = [g.register_clip(x[:, 0].copy(), x[:, 1].copy() if x.shape[1] == 2 else None, float(fs)) for x, fs in xs]
        g.convert_clips(ids)
        for r in range(2):
            for cid, (x, fs) in zip(ids, xs):
                n = C.c_int32(0)
                ch = g._lib.zlhip_sound_read(g.member(r), cid, None, None, 0, C.byref(n))
                L, R = np.zeros(n.value, f32), np.zeros(n.value, f32)
                assert g._lib.zlhip_sound_read(g.member(r), cid, L.ctypes.data, R.ctypes.data if ch == 2 else None, n.value, None) == ch
                got = np.stack([L, R], axis=1) if ch == 2 else L[:, None]
                assert same(got, expected(x, fs) if fs != FT else x), (r, cid)
        assert g.clip_info(ids[0]) == {"length": rr.out_frames(44100, FT, 1000), "channels": 2, "sample_rate": 48000.0, "finite": True, "rendered": False}
        with pytest.raises(ZlHipError, match="member 0"):
            g.convert_clips([ids[0], ids[0]])


def test_libzl_layer_converts_at_load_only_when_asked(built, tmp_path, monkeypatch):
    """a 44.1 kHz WAV: with ZL_LOAD_CONVERT unset the load is today's, bit for bit; with 1 the clip has the converted length, rate and
    data, and getDuration is unchanged; libzl_hotpath_clips_convert does the same to clips already loaded, in one call"""
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    rng = np.random.default_rng(28)
    paths, planes = [], []
    for i, ch in enumerate((2, 1, 2)):
        x = source(rng, 1176 + 147 * i, ch)
        p = str(tmp_path / f"clip{i}.wav")
        assert zl.libzl_wav_write(p.encode(), x[:, 0].copy().ctypes.data, x[:, 1].copy().ctypes.data if ch == 2 else None, x.shape[0], 44100.0, 32) == 0
        paths.append(p)
    odd = str(tmp_path / "odd.wav")                                # 47999 Hz: beyond the limits, stays as loaded
    y = source(rng, 500, 1)
    assert zl.libzl_wav_write(odd.encode(), y[:, 0].copy().ctypes.data, None, 500, 47999.0, 32) == 0

    def sound(e, c):
        cid = zl.ClipAudioSource_engineClip(c)
        n = C.c_int32(0)
        ch = zl.zlhip_sound_read(e, cid, None, None, 0, C.byref(n))
        L, R = np.zeros(n.value, f32), np.zeros(n.value, f32)
        assert zl.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data if ch == 2 else None, n.value, None) == ch
        info = _abi.SoundInfo()
        assert zl.zlhip_sound_info_get(e, cid, C.byref(info)) == 0
        return (np.stack([L, R], axis=1) if ch == 2 else L[:, None]), info

    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        e = zl.libzl_hotpath_engine()
        monkeypatch.delenv("ZL_LOAD_CONVERT", raising=False)
        plain = [zl.ClipAudioSource_new(p.encode(), False) for p in paths]
        loaded = []
        for c in plain:
            data, info = sound(e, c)
            assert info.sample_rate == 44100.0
            loaded.append((data, zl.ClipAudioSource_getDuration(c)))
        monkeypatch.setenv("ZL_LOAD_CONVERT", "0")
        for p, (data, _) in zip(paths, loaded):
            assert same(sound(e, zl.ClipAudioSource_new(p.encode(), False))[0], data)
        monkeypatch.setenv("ZL_LOAD_CONVERT", "1")
        for p, (data, dur) in zip(paths, loaded):
            c = zl.ClipAudioSource_new(p.encode(), False)
            got, info = sound(e, c)
            ref = expected(data, 44100)
            assert info.sample_rate == FT and info.length == ref.shape[0] and info.finite == 1 and same(got, ref)
            assert zl.ClipAudioSource_getDuration(c) == dur
        allp = paths + [odd]
        arr = (C.c_char_p * len(allp))(*[p.encode() for p in allp])
        out = (C.c_void_p * len(allp))()
        assert zl.libzl_hotpath_clips_new(arr, len(allp), out) == len(allp)
        for c, (data, dur) in zip(out[:3], loaded):
            got, info = sound(e, c)
            assert info.sample_rate == FT and same(got, expected(data, 44100)) and zl.ClipAudioSource_getDuration(c) == dur
        got, info = sound(e, out[3])
        assert info.sample_rate == 47999.0 and info.length == 500   # it does not fail the load: it plays pitched
        # clips already loaded, in one call: three convert, the odd one stays
        monkeypatch.delenv("ZL_LOAD_CONVERT", raising=False)
        more = [zl.ClipAudioSource_new(p.encode(), False) for p in allp]
        handles = (C.c_void_p * len(more))(*more)
        assert zl.libzl_hotpath_clips_convert(handles, len(more)) == 3
        for c, (data, dur) in zip(more[:3], loaded):
            assert same(sound(e, c)[0], expected(data, 44100)) and zl.ClipAudioSource_getDuration(c) == dur
        assert sound(e, more[3])[1].sample_rate == 47999.0
        assert zl.libzl_hotpath_clips_convert(handles, len(more)) == 3   # again: nothing left to do
    finally:
        zl.shutdownJuce()
