"""Pitch detection, GPU tier: the kernels of libzl_amd/csrc/zl_pitch.hip against the numpy / Python-integer restatement
(tests/pitch_ref.py): d of every frame, every frame record and every integer of the result bit for bit, hz and confidence with ==,
note and cents within 1e-9 (two log2 implementations, each good to an ulp of a value near 7, times 12: five orders below that)."""
import ctypes as C
import os

import numpy as np
import pytest

import pitch_ref as pr
from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 48000.0
KEYS = ("first_frame", "num_frames", "window", "max_frames", "f_min", "f_max", "threshold", "gate")


def _tone(ch, length, period, seed=0, level=0.3, sr=SR):
    """a harmonic tone of `period` frames with a little noise; the channels differ"""
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    y = np.stack([np.sin(2 * np.pi * t / period + 0.3 * c) + 0.4 * np.sin(4 * np.pi * t / period + c) + 0.2 * np.sin(6 * np.pi * t / period) for c in range(ch)])
    return (level * (y / 1.6 + 0.003 * rng.standard_normal((ch, length)))).astype(f32)


def _upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def _fmin(rate, tmax):
    f = float(f32(rate / (tmax + 0.5)))
    assert pr.lags(rate, f, rate / 4)[1] == tmax
    return f


def _want(src, rate, r):
    n = r.get("num_frames")
    return pr.pitch(src, rate, r.get("first_frame", 0), n, *(r.get(k, 0) for k in KEYS[2:]), want_d=True)


def _same(got, want):
    """the whole result: the integers, hz and confidence with ==, note and cents within 1e-9"""
    return (all(int(got[k]) == int(want[k]) for k in pr.RESULT_INTS) and f32(got["hz"]) == want["hz"] and f32(got["confidence"]) == want["confidence"]
            and abs(float(got["note"]) - float(want["note"])) <= 1e-9 and abs(float(got["cents"]) - float(want["cents"])) <= 1e-9)


def _check_batch(syn, reqs, srcs, rates=None, cache=None):
    """reqs: dicts with "clip" and any of zlhip_pitch_request's fields; srcs: {clip: planar}.  d, the frame records and the result of
    every request against the restatement; returns the mismatches and the results"""
    bad = []
    outs = syn.clip_pitch_batch(reqs)
    for i, (r, got) in enumerate(zip(reqs, outs)):
        key = tuple(sorted(r.items()))
        if cache is None or key not in cache:
            want = _want(srcs[r["clip"]], (rates or {}).get(r["clip"], SR), r)
            if cache is not None:
                cache[key] = want
        res, recs, ds = want if cache is None else cache[key]
        frames = syn.pitch_frames(i)
        okF = frames == recs
        okD = len(frames) == len(ds) and all(syn.pitch_diff(i, k).dtype == np.uint64 and [int(v) for v in syn.pitch_diff(i, k)] == ds[k] for k in range(len(ds)))
        if not (okF and okD and _same(got, res)):
            bad.append((srcs[r["clip"]].shape, r, "frames" if not okF else "d" if not okD else ("result", got, res)))
    return bad, outs


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


GRID = (dict(window=256, f_min=200.0, f_max=2000.0),                           # t_max = 240: one lag tile
        dict(window=512, f_min=100.0, f_max=2000.0),                           # t_max = 480: two tiles, the second partial
        dict(window=4096, f_min=_fmin(SR, 2047), f_max=2000.0))                # the largest frame: eight tiles


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_grid_equals_the_restatement(syn, ch):
    """first frame 1, 3, 5 (16-byte groups straddling the request's edges); one, two and eight lag tiles; max_frames 1, 2 and 5 over half
    a second (the stretched hop)"""
    src = _tone(ch, 24000, 218.4, 10 + ch)
    cid = _upload(syn, src)
    reqs = [dict(g, clip=cid, first_frame=first, num_frames=24000 - first - (first - 1), max_frames=mf) for first in (1, 3, 5) for g in GRID for mf in (1, 2, 5)]
    bad, outs = _check_batch(syn, reqs, {cid: src})
    assert not bad, (len(bad), bad[:3])
    assert [o["frames"] for o in outs[:9]] == [1, 2, 5, 1, 2, 5, 1, 2, 5]       # (24000 frames hold five windows of 4096 and a last span)
    assert all(o["lag"] == 218 and o["confidence"] == 1.0 and abs(o["hz"] - SR / 218.4) < 0.05 for o in outs)
    syn.unregister_clip(cid)


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                    0x39000000, 0x38FFFFFF, 0x39C00000, 0xB9C00000, 0x3A200000], np.uint32)


def test_a_full_scale_clip_and_special_values(syn):
    """full scale in both channels: |m| reaches 65534 and the shift is 4, the largest the definition gives; NaN, +-inf, -0 and
    denormals are quantised as section 12 defines"""
    loud = np.clip(_tone(2, 12000, 150.0, 3, level=60.0), -9.0, 9.0)
    cid = _upload(syn, loud)
    bad, outs = _check_batch(syn, [dict(clip=cid, max_frames=3), dict(GRID[1], clip=cid, first_frame=5, num_frames=11001, max_frames=4)], {cid: loud})
    assert not bad, bad
    assert outs[0]["shift"] == 4 and outs[1]["shift"] == 4 and outs[0]["lag"] == 150 and outs[1]["lag"] == 150
    syn.unregister_clip(cid)
    rng = np.random.default_rng(3)
    for ch in (1, 2):
        src = rng.permutation(np.tile(SPECIAL, 1200))[:12000 * ch].reshape(ch, -1).view(f32).copy()
        src[:, 6000:] = np.where(np.arange(6000) % 3 == 0, src[:, 6000:], _tone(ch, 6000, 99.0, 4))     # the second half: a tone with specials in it
        cid = _upload(syn, src)
        bad, outs = _check_batch(syn, [dict(GRID[0], clip=cid, max_frames=8), dict(GRID[1], clip=cid, first_frame=1, num_frames=11997, max_frames=5),
                                       dict(GRID[0], clip=cid, first_frame=6003, num_frames=5990, max_frames=3)], {cid: src})
        assert not bad, bad
        assert all(o["frames"] > 0 for o in outs)
        syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a small arena that held noise: a neighbour's frame in a head or tail group would
    change the shift and every sum (a full-scale frame is 10^6 times a quiet one)"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(9)
        fill = [_upload(s, rng.uniform(-7.9, 7.9, (ch, 60000)).astype(f32)) for _ in range(3)]
        for cid in fill:
            s.unregister_clip(cid)
        for n in (6001, 3333):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (3001, 3003)]
            quiet = _tone(ch, n, 77.0, n, level=0.004)
            ids = [_upload(s, x) for x in (loud[0], quiet, loud[1])]
            srcs = dict(zip(ids, (loud[0], quiet, loud[1])))
            g = GRID[0]
            reqs = [dict(g, clip=ids[0]), dict(g, clip=ids[1]), dict(g, clip=ids[2]),                # the whole clips: the last group's tail is masked
                    dict(g, clip=ids[1], first_frame=1, num_frames=n - 1), dict(g, clip=ids[0], first_frame=3, num_frames=2998, max_frames=2)]
            bad, outs = _check_batch(s, reqs, srcs)
            assert not bad, bad
            assert outs[1]["shift"] == 0 and outs[1]["lag"] == 77 and outs[3]["lag"] == 77
            assert outs[0]["lag"] == 0 and s.pitch_frames(0)[0]["shift"] >= 3 and s.pitch_frames(1)[0]["shift"] == 0
            for cid in ids:
                s.unregister_clip(cid)


def test_a_batch_of_40_mixed_requests(syn):
    from libzl_amd import _abi
    rng = np.random.default_rng(23)
    srcs = [_tone(1 + i % 2, int(rng.integers(3000, 9000)), float(rng.uniform(30.0, 230.0)), 500 + i) for i in range(7)]
    srcs += [np.zeros((2, 5000), f32), _tone(1, 400, 50.0, 77), rng.uniform(-0.5, 0.5, (1, 6000)).astype(f32)]      # silence, too short for a frame, noise
    ids = [_upload(syn, x) for x in srcs]
    reqs, cache = [], {}
    for i in range(40):
        k = i % 10
        length = srcs[k].shape[1]
        first = int(rng.integers(0, length // 4))
        n = int(rng.integers(length // 2, length - first + 1))
        reqs.append(dict(GRID[(i // 10) % 2], clip=ids[k], first_frame=first, num_frames=n, max_frames=int(rng.choice([0, 1, 3, 7]))))
    arr = (_abi.PitchRequest * 40)(*[_abi.PitchRequest(r["clip"], *(r.get(k, 0) for k in KEYS)) for r in reqs])
    out = (_abi.Pitch * 43)()                                      # three sentinels behind what the call may write
    C.memset(out, 0x5A, C.sizeof(out))
    assert syn._lib.zlhip_sound_pitch_batch(syn._e, arr, 40, out) == 0
    assert bytes(out)[40 * 80:] == b"\x5a" * (3 * 80)
    batch = [{k: getattr(out[i], k) for k, _ in _abi.Pitch._fields_} for i in range(40)]
    bad, outs = _check_batch(syn, reqs, dict(zip(ids, srcs)), cache=cache)
    assert not bad, (len(bad), bad[:3])
    found = 0
    for i, r in enumerate(reqs):
        want = cache[tuple(sorted(r.items()))][0]
        assert _same(batch[i], want) and batch[i] == outs[i], (i, r, batch[i], want)
        if i % 10 >= 7:                                            # no pitch, as defined: everything 0 except frames
            assert all(batch[i][k] == 0 for k in batch[i] if k != "frames"), batch[i]
            assert (batch[i]["frames"] > 0) == (i % 10 != 8)
        found += batch[i]["lag"] > 0
    assert found >= 24
    single = syn.clip_pitch(**{("clip" if k == "clip" else k): v for k, v in reqs[3].items()})
    assert single == outs[3]
    for cid in ids:
        syn.unregister_clip(cid)


def test_a_saw_at_midi_45_with_the_defaults(syn):
    src = pr.clip(pr.saw, SR, 45.0, 0.5)
    cid = _upload(syn, src)
    got = syn.clip_pitch(cid)
    assert _same(got, pr.pitch(src, SR)[0])
    print(got)
    assert got["root_note"] == 45 and abs(got["cents"]) <= 5.0 and abs(got["hz"] - 110.0) < 0.2 and got["confidence"] == 1.0 and got["frames"] == 26
    syn.unregister_clip(cid)


def test_pitch_follows_the_rerender(syn):
    """setPitch(+3) re-renders the clip: the answer comes from the data that plays, three semitones higher within 10 cents (the
    resampler is linear)"""
    src = np.repeat(pr.clip(pr.saw, SR, 57.0, 0.25), 2, 0)
    cid = _upload(syn, src)
    before = syn.clip_pitch(cid)
    assert _same(before, pr.pitch(src, SR)[0]) and before["root_note"] == 57
    syn.rerender_clip(cid, pitch=3.0)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert not np.array_equal(played[:, :4000], src[:, :4000])
    now = syn.clip_pitch(cid)
    assert _same(now, pr.pitch(played, SR)[0]), (now, played.shape)
    assert now["root_note"] == 60 and abs(float(now["note"]) - 60.0) <= 0.10, now
    bad, _ = _check_batch(syn, [dict(GRID[1], clip=cid, first_frame=3, num_frames=played.shape[1] - 7, max_frames=3)], {cid: played})
    assert not bad, bad
    from libzl_amd import ZlHipError
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_pitch(cid, 0, played.shape[1] + 1)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert syn.clip_pitch(cid) == before
    syn.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [_tone(1 + i % 2, 60000 + 1001 * i, 60.0 + 11 * i, 40 + i) for i in range(8)]
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        bad, outs = _check_batch(s, [dict(GRID[0], clip=cid, first_frame=1, num_frames=x.shape[1] - 3, max_frames=3) for cid, x in zip(ids, srcs)], dict(zip(ids, srcs)))
        assert not bad, bad
        assert [o["lag"] for o in outs] == [60 + 11 * i for i in range(8)]


def test_errors_leave_out_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = _tone(2, 50000, 100.0, 8)
    cid = _upload(syn, src)
    fast = _upload(syn, src, 192000.0)
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    R, T = _abi.PitchRequest, _abi.Pitch
    out = (T * 70)()
    C.memset(out, 0x5A, C.sizeof(out))
    INV = _abi.ZLHIP_ERR_INVALID

    def untouched():
        return bytes(out) == b"\x5a" * C.sizeof(out)

    def single(*a):
        r = R(*a)
        rc = lib.zlhip_sound_pitch(e, C.byref(r), out)
        assert untouched(), a
        return rc

    def batch(reqs, nreq=None):
        arr = (R * max(1, len(reqs)))(*reqs)
        rc = lib.zlhip_sound_pitch_batch(e, arr, len(reqs) if nreq is None else nreq, out)
        assert untouched()
        return rc

    ok = (cid, 0, 50000, 1792, 64, 55.0, 1760.0, 154, 8)
    assert single(255, *ok[1:]) == INV and single(-1, *ok[1:]) == INV and single(256, *ok[1:]) == INV and single(gone, *ok[1:]) == INV
    for w in (64, 192, 872, 900, 1791, 4097, 4160, -1792):
        assert single(cid, 0, 50000, w, *ok[4:]) == INV, w
    for lo, hi in ((19.99, 1760.0), (55.0, 24000.0), (1760.0, 1760.0), (1760.0, 55.0), (-55.0, 1760.0), (float("nan"), 1760.0), (55.0, float("nan")),
                   (55.0, float("inf")), (float("-inf"), 1760.0)):
        assert single(cid, 0, 50000, 1792, 64, lo, hi, 154, 8) == INV, (lo, hi)
    assert single(cid, 0, 50000, 4096, 64, 23.43, 1760.0, 154, 8) == INV        # t_max + 1 = 2049
    assert single(cid, 0, 50000, 256, 64, 187.0, 1760.0, 154, 8) == INV         # t_max + 1 = 257 > window
    assert single(fast, 0, 50000, 0, 0, 0.0, 0.0, 0, 0) == INV                  # 192 kHz with f_min = 55: t_max = 3490
    for thr, gate, mf in ((-1, 8, 64), (1025, 8, 64), (154, -1, 64), (154, 32768, 64), (154, 8, -1), (154, 8, 257)):
        assert single(cid, 0, 50000, 1792, mf, 55.0, 1760.0, thr, gate) == INV, (thr, gate, mf)
    assert single(cid, 0, 0, *ok[3:]) == INV and single(cid, 0, -5, *ok[3:]) == INV and single(cid, -1, 10, *ok[3:]) == INV
    assert single(cid, 1, 50000, *ok[3:]) == INV and single(cid, 50000, 1, *ok[3:]) == INV      # past the end
    many = R(cid, 0, 50000, 256, 256, 200.0, 2000.0, 154, 8)                    # (50000 - 497) // 256 + 1 = 194 frames each
    assert batch([many] * 337 + [R(cid, 0, 50000, 256, 159, 200.0, 2000.0, 154, 8)]) == INV             # 65537 analysis frames in one call
    assert batch([R(*ok)], nreq=-1) == INV
    assert batch([R(*ok), R(gone, *ok[1:])]) == INV                # one bad request fails the whole call
    assert b"sound_pitch" in lib.zlhip_last_error(e)
    assert lib.zlhip_sound_pitch_batch(e, None, 1, out) == INV and lib.zlhip_sound_pitch_batch(e, (R * 1)(R(*ok)), 1, None) == INV
    n = C.c_int32(-77)
    assert lib.zlhip_debug_pitch_frames(e, 99, None, 0, C.byref(n)) == INV and lib.zlhip_debug_pitch_diff(e, 99, 0, None, 0, C.byref(n)) == INV and n.value == -77
    # the limits themselves are fine
    assert batch([], nreq=0) == 0
    assert lib.zlhip_sound_pitch_batch(e, (R * 2)(R(*ok), R(cid, 0, 50000, 4096, 1, 23.45, 1760.0, 1024, 32767)), 2, out) == 0
    want = pr.pitch(src, SR, 0, 50000, *ok[3:])[0]
    assert _same({k: getattr(out[0], k) for k, _ in T._fields_}, want) and out[0].lag == 100 and bytes(out)[2 * 80:] == b"\x5a" * (68 * 80)
    d = np.zeros(4, np.uint64)
    h = C.c_int32(0)
    assert lib.zlhip_debug_pitch_diff(e, 0, 0, d.ctypes.data, 4, C.byref(h)) == _abi.ZLHIP_ERR_CAPACITY and h.value == 873 and not d.any()
    assert lib.zlhip_debug_pitch_diff(e, 0, 99, d.ctypes.data, 4, C.byref(h)) == INV and not d.any()
    rec = (_abi.PitchFrame * 1)()
    assert lib.zlhip_debug_pitch_frames(e, 0, C.addressof(rec), 1, C.byref(h)) == _abi.ZLHIP_ERR_CAPACITY and h.value == 27
    for c in (cid, fast):
        syn.unregister_clip(c)


def test_the_largest_call_is_accepted(syn):
    """65536 analysis frames in one call: 337 requests of 194 frames and one of 158"""
    from libzl_amd import _abi
    src = _tone(1, 50000, 100.0, 8)
    cid = _upload(syn, src)
    R = _abi.PitchRequest
    reqs = [R(cid, 0, 50000, 256, 256, 200.0, 2000.0, 154, 8)] * 337 + [R(cid, 0, 50000, 256, 158, 200.0, 2000.0, 154, 8)]
    out = (_abi.Pitch * 338)()
    assert syn._lib.zlhip_sound_pitch_batch(syn._e, (R * 338)(*reqs), 338, out) == 0
    want = pr.pitch(src, SR, 0, 50000, 256, 256, 200.0, 2000.0)[0]
    last = pr.pitch(src, SR, 0, 50000, 256, 158, 200.0, 2000.0)[0]
    assert want["frames"] == 194 and last["frames"] == 158
    assert all(_same({k: getattr(out[i], k) for k, _ in _abi.Pitch._fields_}, want) for i in (0, 1, 200, 336))
    assert _same({k: getattr(out[337], k) for k, _ in _abi.Pitch._fields_}, last)
    syn.unregister_clip(cid)


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _tone(2, 50000, 120.0, 2))
        total0, _ = s.memory_bytes()
        s.clip_tempo(cid)
        total1, _ = s.memory_bytes()
        s.clip_pitch(cid)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_pitch(cid); s.clip_pitch(cid, 3, 40000, **GRID[0]); s.clip_tempo(cid)       # fit the first call's buffers
        assert s.memory_bytes()[0] == total2


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
    """After one warm-up call (it allocates the call's buffers) pitch calls between real-time cycles leave the resident kernel where it
    is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the results right."""
    from libzl_amd import SamplerSynth
    from oracle import zl_oracle as zo
    sc = random_scene(341, num_buses=12, voices_per_bus=8, nclips=20, mode=0, nframes=128, nblocks=40)
    ref_bus, _, _ = run_oracle(sc)
    ref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    syn = SamplerSynth(num_buses=sc.num_buses, voices_per_bus=sc.voices_per_bus, mode=sc.mode, playback_sample_rate=sc.fs,
                       max_frames=max(64, sc.nframes), max_batch_blocks=4, max_sounds=max(8, len(sc.sounds) + 1),
                       sound_arena_bytes=(1 << 20) + sum((s[0].shape[0] + 16) * 8 for s in sc.sounds) + (1 << 16))
    try:
        planar, rates = [], []
        for i, (L, R, sr) in enumerate(sc.sounds):
            assert ref.register_clip(L, R, sr) == i and syn.register_clip(L, R, sr) == i
            if i in sc.clip_setup:
                sc.clip_setup[i](ref.lib, ref.clips[i])
            syn.set_clip_params(i, snapshot_clip(ref.clips[i]))
            planar.append(np.stack([L, R]) if R is not None else L[None, :])
            rates.append(float(sr))

        # one more clip, which no voice plays, has a pitch
        tone = _tone(1, 12000, 109.1, 5)
        extra = syn.register_clip(tone[0], None, SR)
        assert extra == len(planar)
        planar.append(tone); rates.append(SR)

        def params(cid, k):
            p = [dict(), dict(window=256, f_min=400.0, f_max=4000.0, max_frames=3), dict(window=512, f_min=200.0, f_max=3000.0, max_frames=2)][k % 3]
            return p if pr.resolve(rates[cid], planar[cid].shape[1], **p) is not None else dict(window=512, f_min=400.0, f_max=3000.0, max_frames=2)

        # the warm-up call: every clip with every parameter set, more frames, words and requests than any call below
        syn.clip_pitch_batch([dict(params(i, k), clip=i) for i in range(len(planar)) for k in range(3)] + [dict(clip=extra, window=256, f_min=400.0, f_max=4000.0)] * 2)
        expect = {}
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts_after_first = None
        looping = [ev[1]["clip"] for ev in sc.events[0] if ev[1].get("looping")]      # started in block 0, play to the end
        checked = found = 0
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
            # between the cycles: the pitch of clips that play, a single call and a batch in turn
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            reqs = [dict(params(cid, k), clip=cid) for cid in playing[:2]] + [dict(clip=extra, first_frame=k % 5, num_frames=11000, window=(256, 512)[k % 2], f_min=400.0, f_max=3000.0, max_frames=1 + k % 4)]
            gots = [syn.clip_pitch_batch([r])[0] for r in reqs] if k % 2 else syn.clip_pitch_batch(reqs)
            for r, got in zip(reqs, gots):
                key = tuple(sorted(r.items()))
                if key not in expect:
                    expect[key] = _want(planar[r["clip"]], rates[r["clip"]], r)[0]
                assert _same(got, expect[key]), (k, r, got, expect[key])
                checked += 1
                found += got["lag"] > 0
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        assert checked >= 2 * sc.nblocks and found >= sc.nblocks
        print("requests with a pitch:", found, "of", checked)
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


def test_group_pitch_equals_the_single_engine(syn):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    srcs = [pr.clip(pr.saw, SR, 50.0, 0.5, seconds=0.5), _tone(2, 20000, 130.0, 6)]
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        for src in srcs:
            cid, gid = _upload(syn, src), _upload(g, src)
            for args in ((), (3, 15000, 512, 3, 100.0, 2000.0)):
                a = g.clip_pitch(gid, *args)
                assert a == syn.clip_pitch(cid, *args) and a["lag"] > 0
            assert _same(a, pr.pitch(src, SR, 3, 15000, 512, 3, 100.0, 2000.0)[0])
            syn.unregister_clip(cid)
        a, b = g.clip_pitch_batch([(0,), (1, 5, 1000)])
        assert a["root_note"] == 50 and b["lag"] == 0 and b["frames"] == 0
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_pitch_batch([(0, 0, None, 65)])


def test_libzl_clip_pitch_and_detect_root_note(built, tmp_path):
    from libzl_amd import _abi, libzl
    from libzl_amd.engine import synthetic_clocks
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        saw = pr.clip(pr.saw, SR, 45.0, 0.5)
        noise = np.random.default_rng(5).uniform(-0.5, 0.5, (1, 48000)).astype(f32)
        clips = []
        for name, src in (("a", saw), ("b", saw), ("c", saw), ("n", noise)):
            path = str(tmp_path / (name + ".wav")).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, None, src.shape[1], SR, 32) == 0
            clips.append(zl.ClipAudioSource_new(path, False))
            assert clips[-1] and zl.ClipAudioSource_rootNote(clips[-1]) == 60
        a, b, c, n = clips

        hz, note, conf, root = C.c_float(-1.0), C.c_float(-1.0), C.c_float(-1.0), C.c_int(-1)
        assert zl.libzl_hotpath_clip_pitch(None, 0.0, 0.0, C.byref(hz), C.byref(note), C.byref(conf)) < 0
        assert zl.libzl_hotpath_clip_pitch(a, 1760.0, 55.0, C.byref(hz), C.byref(note), C.byref(conf)) < 0 and (hz.value, note.value, conf.value) == (-1.0, -1.0, -1.0)
        lib = _abi.load()
        eng, cid = C.c_void_p(zl.libzl_hotpath_engine()), zl.ClipAudioSource_engineClip(a)
        cnt = C.c_int32(0)
        assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(cnt)) >= 0 and cnt.value == 48000
        pl, pr_ = np.empty(cnt.value, f32), np.empty(cnt.value, f32)
        chans = lib.zlhip_sound_read(eng, cid, pl.ctypes.data, pr_.ctypes.data, cnt.value, C.byref(cnt))
        played = np.stack([pl, pr_]) if chans == 2 else pl[None, :]           # what the clip plays, as the engine holds it
        assert np.array_equal(played[0], saw[0])
        want = pr.pitch(played, SR)[0]
        assert zl.libzl_hotpath_clip_pitch(a, 0.0, 0.0, C.byref(hz), C.byref(note), C.byref(conf)) == 0
        assert f32(hz.value) == want["hz"] and f32(conf.value) == want["confidence"] and abs(note.value - float(want["note"])) <= 1e-9 and abs(note.value - 45.0) <= 0.05
        narrow = pr.pitch(played, SR, f_min=80.0, f_max=500.0)[0]
        assert zl.libzl_hotpath_clip_pitch(a, 80.0, 500.0, C.byref(hz), C.byref(note), C.byref(conf)) == 0 and f32(hz.value) == narrow["hz"]
        # noise: no pitch, not an error; the root note stays
        assert zl.libzl_hotpath_clip_pitch(n, 0.0, 0.0, C.byref(hz), C.byref(note), C.byref(conf)) == 0 and (hz.value, note.value, conf.value) == (0.0, 0.0, 0.0)
        assert zl.libzl_hotpath_clip_detect_root_note(n, 0.5, C.byref(root)) == 0 and root.value == -1 and zl.ClipAudioSource_rootNote(n) == 60
        # below the confidence asked for: nothing changes
        assert zl.libzl_hotpath_clip_detect_root_note(a, 2.0, C.byref(root)) == 0 and root.value == -1 and zl.ClipAudioSource_rootNote(a) == 60
        assert zl.libzl_hotpath_clip_detect_root_note(None, 0.5, C.byref(root)) < 0
        assert zl.libzl_hotpath_clip_detect_root_note(a, 0.5, C.byref(root)) == 1 and root.value == 45 and zl.ClipAudioSource_rootNote(a) == 45
        zl.ClipAudioSource_setRootNote(b, 45)                      # by hand; c keeps 60

        # a voice per clip at note 45 on its own channel: a and b render the same bits, at ratio 1; c plays fifteen semitones down
        N = 128
        outL = np.zeros((12, N), f32); outR = np.zeros((12, N), f32)
        for clip, ch in ((a, 1), (b, 2), (c, 3)):
            cmd = engine_cmd(clip=zl.ClipAudioSource_engineClip(clip), midiChannel=ch, midiNote=45, changeVolume=1, volume=1.0, looping=0, startPlayback=1)
            zl.libzl_hotpath_schedule_clip_command(C.byref(cmd), 0)
        blocks = []
        for k in range(24):
            assert zl.libzl_hotpath_process(N, synthetic_clocks(1, N, SR, start_block=k), outL.ctypes.data, outR.ctypes.data) == 0
            blocks.append(np.stack([outL.copy(), outR.copy()], 1))
        audio = np.concatenate(blocks, 2)                          # [bus][2][frames]
        live = [i for i in range(12) if audio[i].any()]
        assert len(live) == 3, live
        same = [(i, j) for i in live for j in live if i < j and np.array_equal(audio[i].view(np.int32), audio[j].view(np.int32))]
        assert len(same) == 1, same                                # a and b; c differs from both
        # ratio 1: what the voice renders is itself at note 45; the clip with root 60 comes out fifteen semitones lower
        heard = pr.pitch(audio[same[0][0]], SR, window=1216, f_min=40.0, f_max=500.0, max_frames=1)[0]
        assert heard["root_note"] == 45 and abs(float(heard["note"]) - 45.0) <= 0.1, heard
        other = [i for i in live if i not in same[0]][0]
        low = pr.pitch(audio[other], SR, window=1216, f_min=40.0, f_max=500.0, max_frames=1)[0]
        assert low["root_note"] == 30, low
        for clip in clips:
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
