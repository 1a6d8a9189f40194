"""Waveform overviews on the device (zlhip_sound_overview / _batch, include/zlhip.h): the columns against the numpy restatement
(tests/overview_ref.py) bit for bit -- over lengths, channel counts, column counts and sub-ranges at every alignment, special
values, neighbouring clips, re-rendered clips, a grown arena, batches, errors -- and the call's place next to the resident
real-time kernel, in the engine group and behind the libzl-named layer."""
import os

import numpy as np
import pytest

import overview_ref as ov
import stretch_ref as sr_
from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32

LENGTHS = (1, 2, 3, 63, 64, 65, 255, 257, 1000, 4099, 70001)
COLUMNS = (1, 2, 3, 7, 64, 100, 4096)
KINDS = {"positive": (0.25, 1.0), "negative": (-1.0, -0.25), "both": (-1.0, 1.0)}


def _source(kind, ch, length):
    lo, hi = KINDS[kind]
    rng = np.random.default_rng(1000 * list(KINDS).index(kind) + 7 * length + ch)
    return rng.uniform(lo, hi, (ch, length)).astype(f32)


def _upload(syn, src, sr=48000.0):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


@pytest.fixture(scope="module")
def clips(syn):
    """every (kind, channels, length) of the grid, uploaded once: {key: (clip id, planar source)}"""
    table = {}
    for kind in KINDS:
        for ch in (1, 2):
            for length in LENGTHS:
                src = _source(kind, ch, length)
                table[(kind, ch, length)] = (_upload(syn, src), src)
    return table


@pytest.mark.parametrize("kind", list(KINDS))
def test_grid_full_range_equals_the_restatement(syn, clips, kind):
    """70001 frames in one column: many pieces into one word; 4096 columns over 3 frames: many columns per frame"""
    bad = []
    for ch in (1, 2):
        for length in LENGTHS:
            cid, src = clips[(kind, ch, length)]
            for columns in COLUMNS:
                out = syn.clip_overview(cid, columns)
                assert out.shape == (columns, 4) and out.dtype == f32
                if not ov.same_bits(out, ov.overview(src, columns)):
                    bad.append((ch, length, columns))
    assert not bad, bad[:10]


@pytest.mark.parametrize("kind", list(KINDS))
def test_grid_sub_ranges_equal_the_restatement(syn, clips, kind):
    """first frame 1, 2, 3, 5 and a last frame 1, 2, 3 short of the end: the head and tail of misaligned 16-byte groups are masked.
    A pad zero, or the frame next to the range, leaking into a column is a wrong minimum in the positive set and a wrong maximum in
    the negative one."""
    bad = []
    for ch in (1, 2):
        for length in LENGTHS:
            cid, src = clips[(kind, ch, length)]
            reqs = [(cid, columns, first, length - first - short) for first in (1, 2, 3, 5) for short in (1, 2, 3)
                    for columns in COLUMNS if length - first - short >= 1]
            if not reqs:
                continue
            outs = syn.clip_overviews(reqs)
            for (_, columns, first, n), out in zip(reqs, outs):
                if not ov.same_bits(out, ov.overview(src, columns, first, n)):
                    bad.append((ch, length, columns, first, n))
    assert not bad, bad[:10]


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], u32)


def test_special_values_come_back_with_their_own_bits(syn):
    """+-0, denormals, +-inf, NaNs of both signs: compared as uint32"""
    rng = np.random.default_rng(5)
    for ch in (1, 2):
        src = rng.permutation(np.tile(SPECIAL, 150))[:1100 * ch].reshape(ch, -1).view(f32)
        cid = _upload(syn, src)
        for columns, first, n in ((1, 0, 1100), (7, 1, 1097), (64, 3, 1001), (100, 0, 1100), (1100, 0, 1100), (4096, 2, 3), (16, 0, 16)):
            out = syn.clip_overview(cid, columns, first, n)
            ref = ov.overview(src, columns, first, n, loop=True)
            assert np.array_equal(out.view(u32), ref.view(u32)), (ch, columns, first, n)
        # one frame per column: every value is its own minimum and maximum -- -0 is not +0, a NaN keeps its payload
        one = syn.clip_overview(cid, 1100).view(u32)
        assert np.array_equal(one[:, 0], src[0].view(u32)) and np.array_equal(one[:, 1], src[0].view(u32))
        syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """three clips back to back in a fresh arena, disjoint value ranges: every overview stays inside its clip's own range"""
    from libzl_amd import SamplerSynth
    ranges = [(0.25, 0.5), (-0.5, -0.25), (0.6, 0.9)]
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=1 << 20) as s:
        rng = np.random.default_rng(9)
        srcs = [rng.uniform(lo, hi, (ch, n)).astype(f32) for (lo, hi), n in zip(ranges, (1001, 777, 1003))]
        ids = [_upload(s, x) for x in srcs]
        for cid, x, (lo, hi) in zip(ids, srcs, ranges):
            for columns in (1, 3, 64, 777, 4096):
                for first, n in ((0, None), (1, x.shape[1] - 2), (x.shape[1] - 5, 5)):
                    out = s.clip_overview(cid, columns, first, n)
                    assert out.min() >= f32(lo) and out.max() <= f32(hi), (cid, columns, first)
                    assert ov.same_bits(out, ov.overview(x, columns, first, n))


def test_overview_follows_the_rerender(syn):
    src = _source("both", 2, 30000)
    cid = _upload(syn, src, 44100.0)
    before = syn.clip_overview(cid, 100)
    syn.rerender_clip(cid, gain_db=-6.0, pitch=3.0, speed=1.25)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert played.shape[1] == 24000
    for columns, first, n in ((100, 0, None), (7, 3, 23990), (4096, 0, None), (1, 0, None)):
        assert ov.same_bits(syn.clip_overview(cid, columns, first, n), ov.overview(played, columns, first, n or played.shape[1] - first))
    assert not ov.same_bits(syn.clip_overview(cid, 100), before)
    from libzl_amd import ZlHipError
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_overview(cid, 10, 0, 30000)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert ov.same_bits(syn.clip_overview(cid, 100), before) and ov.same_bits(before, ov.overview(src, 100))
    assert ov.same_bits(syn.clip_overview(cid, 10, 0, 30000), ov.overview(src, 10))
    syn.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    """a small arena and uploads beyond it: the later clips lie in further segments, far from the first one in the address space"""
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [_source("both", 1 + i % 2, 60000 + 1001 * i) for i in range(8)]      # 0.24 - 0.54 MB each
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        outs = s.clip_overviews([(cid, 333, 1) for cid in ids])
        for x, out in zip(srcs, outs):
            assert ov.same_bits(out, ov.overview(x, 333, 1))
        assert ov.same_bits(s.clip_overview(ids[-1], 4096), ov.overview(srcs[-1], 4096))
        assert ov.same_bits(s.clip_overview(ids[-1], 1), ov.overview(srcs[-1], 1))


def test_a_batch_of_64_equals_64_single_calls(syn):
    rng = np.random.default_rng(23)
    srcs = [_source("both", 1 + i % 2, int(rng.integers(1, 20000))) for i in range(16)]
    ids = [_upload(syn, x) for x in srcs]
    reqs = []
    for i in range(64):
        k = i % 16
        length = srcs[k].shape[1]
        first = int(rng.integers(0, length))
        n = int(rng.integers(1, length - first + 1))
        reqs.append((ids[k], int(rng.choice([1, 2, 3, 7, 64, 100, 257, 4096])), first, n))
    lib, e = syn._lib, syn._e
    from libzl_amd import _abi
    arr = (_abi.OverviewRequest * 64)(*[_abi.OverviewRequest(c, f, n, cols) for c, cols, f, n in reqs])
    total = sum(r[1] for r in reqs)
    packed = np.full((total + 3, 4), f32(1234.5))                  # three sentinel columns behind the packed output
    assert lib.zlhip_sound_overview_batch(e, arr, 64, packed.ctypes.data, total * 4) == 0
    assert (packed[total:] == f32(1234.5)).all()
    at = 0
    for (cid, cols, first, n), k in zip(reqs, [i % 16 for i in range(64)]):
        single = syn.clip_overview(cid, cols, first, n)
        assert ov.same_bits(packed[at:at + cols], single), (cid, cols, first, n)      # no gaps: request i starts where i - 1 ended
        assert ov.same_bits(single, ov.overview(srcs[k], cols, first, n))
        at += cols
    assert at == total
    for cid in ids:
        syn.unregister_clip(cid)


def test_errors_leave_out_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = _source("both", 2, 1000)
    cid = _upload(syn, src)
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    out = np.full(4 * 262144 + 64, f32(-77.25))

    def single(*a):
        rc = lib.zlhip_sound_overview(e, *a, out.ctypes.data)
        assert (out == f32(-77.25)).all(), a
        return rc

    INV, CAP = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY
    assert single(255, 0, 10, 4) == INV                            # a slot that never held a sound
    assert single(-1, 0, 10, 4) == INV and single(256, 0, 10, 4) == INV
    assert single(gone, 0, 10, 4) == INV                           # a released id
    assert single(cid, 0, 1000, 0) == INV and single(cid, 0, 1000, 4097) == INV and single(cid, 0, 1000, -1) == INV
    assert single(cid, 1, 1000, 4) == INV and single(cid, 1000, 1, 4) == INV and single(cid, -1, 10, 4) == INV      # past the end / before the start
    assert single(cid, 0, 0, 4) == INV and single(cid, 0, -5, 4) == INV
    R = _abi.OverviewRequest
    many = (R * 65)(*[R(cid, 0, 1000, 4096)] * 64, R(cid, 0, 1000, 1))                # 262145 columns
    assert lib.zlhip_sound_overview_batch(e, many, 65, out.ctypes.data, out.size) == INV and (out == f32(-77.25)).all()
    two = (R * 2)(R(cid, 0, 1000, 10), R(cid, 0, 1000, 10))
    assert lib.zlhip_sound_overview_batch(e, two, 2, out.ctypes.data, 79) == CAP and (out == f32(-77.25)).all()
    mixed = (R * 2)(R(cid, 0, 1000, 10), R(gone, 0, 1000, 10))                        # one bad request fails the whole call
    assert lib.zlhip_sound_overview_batch(e, mixed, 2, out.ctypes.data, out.size) == INV and (out == f32(-77.25)).all()
    assert b"sound_overview" in lib.zlhip_last_error(e)
    # the limits themselves are fine
    assert lib.zlhip_sound_overview_batch(e, many, 64, out.ctypes.data, 4 * 262144) == 0
    assert ov.same_bits(out[:4 * 4096].reshape(4096, 4), ov.overview(src, 4096)) and (out[4 * 262144:] == f32(-77.25)).all()
    assert lib.zlhip_sound_overview_batch(e, two, 2, out.ctypes.data, 80) == 0
    syn.unregister_clip(cid)


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _source("both", 2, 5000))
        total0, _ = s.memory_bytes()
        s.clip_overview(cid, 100)
        total1, _ = s.memory_bytes()
        assert total1 > total0
        s.clip_overview(cid, 4096); s.clip_overview(cid, 7)        # fits the first call's buffers
        assert s.memory_bytes()[0] == total1


@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_the_resident_kernel_stays(built, rt_env):
    """After one warm-up call (it allocates the call's buffers) overviews between real-time cycles leave the resident kernel where
    it is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the overviews right."""
    from libzl_amd import SamplerSynth
    from oracle import zl_oracle as zo
    sc = random_scene(341, num_buses=12, voices_per_bus=8, nclips=20, mode=0, nframes=128, nblocks=40)
    ref_bus, _, _ = run_oracle(sc)
    ref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    syn = SamplerSynth(num_buses=sc.num_buses, voices_per_bus=sc.voices_per_bus, mode=sc.mode, playback_sample_rate=sc.fs,
                       max_frames=max(64, sc.nframes), max_batch_blocks=4, max_sounds=max(8, len(sc.sounds)),
                       sound_arena_bytes=max(1 << 20, sum((s[0].shape[0] + 16) * 8 for s in sc.sounds) + (1 << 16)))
    try:
        planar = []
        for i, (L, R, sr) in enumerate(sc.sounds):
            assert ref.register_clip(L, R, sr) == i and syn.register_clip(L, R, sr) == i
            if i in sc.clip_setup:
                sc.clip_setup[i](ref.lib, ref.clips[i])
            syn.set_clip_params(i, snapshot_clip(ref.clips[i]))
            planar.append(np.stack([L, R]) if R is not None else L[None, :])
        syn.clip_overviews([(i, 512) for i in range(len(planar))])                     # the warm-up call
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts_after_first = None
        looping = [ev[1]["clip"] for ev in sc.events[0] if ev[1].get("looping")]      # started in block 0, play to the end
        checked = 0
        for k in range(sc.nblocks):
            for ev in sc.events.get(k, []):
                if ev[0] == "cmd":
                    syn.handle_clip_command(engine_cmd(**ev[1]), ev[2])
                elif ev[0] == "start":
                    syn.start_voice(ev[1], ev[2], engine_cmd(**ev[3]), ev[4])
                elif ev[0] == "clip":
                    ev[2](ref.lib, ref.clips[ev[1]])
                    syn.set_clip_params(ev[1], snapshot_clip(ref.clips[ev[1]]))
                elif ev[0] == "update":
                    syn.update_voice(ev[1], ev[2], engine_cmd(**ev[3]))
                elif ev[0] == "stopv":
                    syn.stop_voice(ev[1], ev[2], ev[3])
                elif ev[0] == "enable":
                    syn.set_bus_enabled(ev[1], ev[2])
                else:
                    raise AssertionError(ev[0])
            L, R = syn.process(N, sc.make_clocks(k, 1)[0])
            out[:, 0, k * N:(k + 1) * N] = L
            out[:, 1, k * N:(k + 1) * N] = R
            if starts_after_first is None:
                starts_after_first = syn.rt_stats()[0]
            # between the cycles: the overview of clips that play (the voice reports are host memory: no device call), a single call
            # and a batch in turn
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            for cid in playing[:2]:
                cols = (512, 64, 7)[k % 3]
                got = syn.clip_overview(cid, cols) if k % 2 else syn.clip_overviews([(cid, cols), (cid, 3, 1)])[0]
                assert ov.same_bits(got, ov.overview(planar[cid], cols)), (k, cid)
                checked += 1
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        assert checked >= sc.nblocks
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


def test_group_overview_equals_the_single_engine(syn, clips):
    from libzl_amd import SamplerSynthGroup
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        for key in (("both", 2, 4099), ("negative", 1, 70001), ("positive", 2, 3)):
            cid, src = clips[key]
            gid = _upload(g, src)
            for columns, first, n in ((100, 0, None), (4096, 0, None), (7, 1, src.shape[1] - 2) if src.shape[1] > 3 else (2, 1, 2)):
                a = g.clip_overview(gid, columns, first, n)
                assert ov.same_bits(a, syn.clip_overview(cid, columns, first, n))
                assert ov.same_bits(a, ov.overview(src, columns, first, n))
        a, b = g.clip_overviews([(0, 10), (1, 20, 5, 1000)])
        assert a.shape == (10, 4) and b.shape == (20, 4)
        from libzl_amd import ZlHipError
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_overviews([(0, 0)])


def test_libzl_clip_waveform(built, tmp_path):
    from libzl_amd import libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        sr = 44100.0
        src = _source("both", 2, 30001)
        path = str(tmp_path / "w.wav").encode()
        assert zl.libzl_wav_write(path, src[0].ctypes.data, src[1].ctypes.data, src.shape[1], sr, 32) == 0
        c = zl.ClipAudioSource_new(path, False)
        assert c

        def waveform(start, end, columns):
            out = np.full((columns + 1, 4), f32(9.5))
            assert zl.libzl_hotpath_clip_waveform(c, start, end, columns, out.ctypes.data) == 0
            assert (out[columns] == f32(9.5)).all()
            return out[:columns]

        def frames(seconds):
            return int(np.floor(float(f32(seconds)) * sr))

        assert ov.same_bits(waveform(0.0, 0.0, 300), ov.overview(src, 300))           # (0, 0): the whole clip
        a, b = frames(0.1), frames(0.45)
        assert ov.same_bits(waveform(0.1, 0.45, 200), ov.overview(src, 200, a, b - a))
        assert ov.same_bits(waveform(0.1, 99.0, 200), ov.overview(src, 200, a))        # an end beyond the data: to the end
        assert ov.same_bits(waveform(0.1, 0.05, 200), ov.overview(src, 200, a))        # end <= start: to the end
        zl.ClipAudioSource_setGain(c, -6.0)
        louder = ov.overview(src, 300)
        now, _ = sr_.render(src, sr, -6.0, 0.0, 1.0)
        got = waveform(0.0, 0.0, 300)
        assert ov.same_bits(got, ov.overview(now, 300)) and not ov.same_bits(got, louder)
        out = np.full((4, 4), f32(9.5))
        assert zl.libzl_hotpath_clip_waveform(c, 0.0, 0.0, 0, out.ctypes.data) < 0 and (out == f32(9.5)).all()
        zl.ClipAudioSource_destroy(c)
    finally:
        zl.shutdownJuce()
