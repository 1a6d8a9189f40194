"""Loudness measurement, GPU tier: the kernel of libzl_amd/csrc/zl_loudness.hip against the numpy restatement (tests/loudness_ref.py),
which takes its ten coefficients from zlhip_loudness_design: every sub-block record (the sums as doubles, the peaks as floats), every
integer of the result, mean_square and relative_gate with ==, lufs within 1e-9 (two log10 implementations, each good to an ulp of a
value below 100: five orders below that)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loudness_ref as lr
from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 48000.0
_COEFFS = {}


def _coeffs(rate):
    if rate not in _COEFFS:
        from libzl_amd import _abi
        c = (C.c_double * 10)()
        assert _abi.load().zlhip_loudness_design(rate, c) == 0
        _COEFFS[rate] = list(c)
    return _COEFFS[rate]


def _clip(ch, length, seed=0, level=0.2, period=48.3):
    """a tone with noise on it; the channels differ"""
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    y = np.stack([np.sin(2 * np.pi * t / period + 0.7 * c) for c in range(ch)])
    return (level * (y + 0.2 * rng.standard_normal((ch, length)))).astype(f32)


def _upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def _played(syn, cid):
    L, R = syn.read_clip(cid)
    return np.stack([L, R]) if R is not None else L[None, :]


def _check_batch(syn, reqs, srcs, rates=None):
    """reqs: dicts with "clip" and any of first_frame, num_frames, sub_frames; srcs: {clip: planar}.  Every record and the result of
    every request against the restatement; returns the mismatches and the results"""
    outs = syn.clip_loudness_batch(reqs)
    rate = lambda r: (rates or {}).get(r["clip"], SR)
    wants = lr.measure_batch([(srcs[r["clip"]], rate(r), r.get("first_frame", 0), r.get("num_frames"), r.get("sub_frames", 0), _coeffs(rate(r))) for r in reqs])
    bad = []
    for i, (r, got, (want, sums, peaks)) in enumerate(zip(reqs, outs, wants)):
        gs, gp = syn.loudness_subs(i)
        okS = gs.dtype == np.float64 and gs.shape == sums.shape and np.array_equal(gs.view(np.uint64), sums.view(np.uint64))
        okP = gp.dtype == f32 and gp.shape == peaks.shape and np.array_equal(gp.view(np.uint32), peaks.view(np.uint32))
        if not (okS and okP and lr.same(got, want)):
            bad.append((srcs[r["clip"]].shape, r, "sums" if not okS else "peaks" if not okP else ("result", got, want)))
    return bad, outs


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_grid_equals_the_restatement(syn, ch):
    """first frame 1, 3, 5 (16-byte groups straddling the request's edges); sub-blocks of 64, 100 and the default 4800; S = 1, 2, 3 (the
    short rule, with a partial last item where the remainder is 37), 4, 5, 9; remainder 0 and 37 (the last item's peak scan)"""
    src = _clip(ch, 47000, 10 + ch)
    src[:, 46990:] *= 4.0                                          # a peak that only a remainder's scan can find
    cid = _upload(syn, src)
    reqs = [dict(clip=cid, first_frame=first, num_frames=S * (sub or 4800) + rem, sub_frames=sub)
            for sub in (64, 100, 0) for first in (1, 3, 5) for S in (1, 2, 3, 4, 5, 9) for rem in (0, 37)]
    reqs.append(dict(clip=cid, first_frame=46990 - 9 * 100 - 3, num_frames=9 * 100 + 13, sub_frames=100))      # the loud tail lies in the remainder
    bad, outs = _check_batch(syn, reqs, {cid: src})
    assert not bad, (len(bad), bad[:3])
    assert [(o["sub_blocks"], o["blocks"]) for o in outs[:12]] == [(1, 1), (2, 1), (2, 1), (3, 1), (3, 1), (4, 1), (4, 1), (4, 1), (5, 2), (5, 2), (9, 6), (9, 6)]
    assert all(-25.0 < o["lufs"] < -10.0 and o["above_absolute"] == o["blocks"] for o in outs)
    assert max(outs[-1]["peak"]) > 1.5 * max(outs[0]["peak"])
    syn.unregister_clip(cid)


def test_a_mixed_batch_of_320_requests(syn):
    """44.1 and 48 kHz, mono and stereo, sub-blocks from 16 to the default, short-rule and one-frame requests in one call: the 5000 or
    so items put different numbers of steps into the same wavefronts, and most requests straddle a workgroup's 64 items"""
    from libzl_amd import _abi
    rng = np.random.default_rng(23)
    rates = [44100.0, 48000.0]
    srcs = [_clip(1 + i % 2, int(rng.integers(9000, 14000)), 500 + i, level=float(rng.uniform(0.01, 0.9))) for i in range(8)]
    ids = [_upload(syn, x, rates[(i // 2) % 2]) for i, x in enumerate(srcs)]
    rate_of = {cid: rates[(i // 2) % 2] for i, cid in enumerate(ids)}
    reqs = []
    for i in range(320):
        k = i % 8
        length = srcs[k].shape[1]
        sub = int(rng.choice([16, 17, 64, 100, 441, 1000, 0]))
        first = int(rng.integers(0, length // 4))
        kind = i % 5
        n = 1 if kind == 0 else int(rng.integers(1, 3 * (sub or 4410))) if kind == 1 else int(rng.integers(length // 2, length - first + 1))
        reqs.append(dict(clip=ids[k], first_frame=first, num_frames=min(n, length - first), sub_frames=sub))
    arr = (_abi.LoudnessRequest * 320)(*[_abi.LoudnessRequest(r["clip"], r["first_frame"], r["num_frames"], r["sub_frames"]) for r in reqs])
    out = (_abi.Loudness * 323)()                                  # three sentinels behind what the call may write
    C.memset(out, 0x5A, C.sizeof(out))
    assert syn._lib.zlhip_sound_loudness_batch(syn._e, arr, 320, out) == 0
    assert bytes(out)[320 * 48:] == b"\x5a" * (3 * 48)
    raw = [{k: (tuple(out[i].peak) if k == "peak" else getattr(out[i], k)) for k, _ in _abi.Loudness._fields_} for i in range(320)]
    bad, outs = _check_batch(syn, reqs, dict(zip(ids, srcs)), rate_of)
    assert not bad, (len(bad), bad[:3])
    assert raw == outs
    assert sum(o["sub_blocks"] for o in outs) > 3000 and sum(o["sub_blocks"] == 1 for o in outs) >= 64
    single = syn.clip_loudness(**{k: v for k, v in reqs[7].items()})
    assert single == outs[7]
    for cid in ids:
        syn.unregister_clip(cid)


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x3DCCCCCD, 0xBDCCCCCD], np.uint32)


def test_special_values(syn):
    """NaN and +-inf count as 0 and never as a peak; float subnormals (1e-40) are kept, the records still match with ==; silence and a
    clip at 1e-5 have no loudness; a full-scale square wave"""
    rng = np.random.default_rng(3)
    for ch in (1, 2):
        mixed = rng.permutation(np.tile(SPECIAL, 750))[:6000 * ch].reshape(ch, -1).view(f32).copy()
        tiny = np.full((ch, 6000), 1e-40, f32) * np.where(rng.random((ch, 6000)) < 0.5, -1, 1).astype(f32)
        assert tiny.view(np.uint32).max() & 0x7F800000 == 0 and np.abs(tiny).min() > 0        # subnormal, not zero
        silence = np.zeros((ch, 6000), f32)
        quiet = _clip(ch, 6000, 5, level=1e-5)
        square = np.where((np.arange(6000) // 24) % 2 == 0, 1.0, -1.0).astype(f32)[None, :].repeat(ch, 0)
        srcs = [mixed, tiny, silence, quiet, square]
        ids = [_upload(syn, x) for x in srcs]
        reqs = [dict(clip=c, first_frame=first, num_frames=5990, sub_frames=sub) for c in ids for first, sub in ((1, 100), (3, 480))]
        bad, outs = _check_batch(syn, reqs, dict(zip(ids, srcs)))
        assert not bad, bad[:3]
        for o in outs[:2]:
            assert math.isfinite(o["lufs"]) and max(o["peak"]) == 1.0          # the largest finite magnitude among the specials
        sums, peaks = syn.loudness_subs(2)                                      # (request 2: the subnormal clip)
        assert (sums[:, :ch] > 0).all() and (peaks[:, :ch] == f32(1e-40)).all() and (sums[:, ch:] == 0).all()
        for o in outs[2:8]:                                                     # subnormals, silence, 1e-5: no loudness, not an error
            assert o["lufs"] == -math.inf and o["above_absolute"] == 0 and o["above_relative"] == 0 and o["mean_square"] == 0.0 and o["relative_gate"] == 0.0
        assert outs[4]["peak"] == (0.0, 0.0) and 0 < max(outs[6]["peak"]) < 1e-4
        for o in outs[8:]:                                                      # the square: every block passes; a mean square of 1 per channel
            assert o["above_relative"] == o["blocks"] and o["peak"] == (1.0, 1.0 if ch == 2 else 0.0)
            assert 0.0 < o["lufs"] - (-0.691 + 10 * math.log10(ch)) < 3.0      # (the shelf lifts the harmonics)
        for cid in ids:
            syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a small arena that held noise, measured from its first frame and to its last, whose
    16-byte group lies partly behind the data: a neighbour's sample in a head or tail group would show in a sum and in a peak (a
    full-scale sample is 2000 times a quiet one)"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(9)
        fill = [_upload(s, rng.uniform(-7.9, 7.9, (ch, 60000)).astype(f32)) for _ in range(3)]
        for cid in fill:
            s.unregister_clip(cid)
        for n in (6001, 3333):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (3001, 3003)]
            quiet = _clip(ch, n, n, level=0.004)
            ids = [_upload(s, x) for x in (loud[0], quiet, loud[1])]
            srcs = dict(zip(ids, (loud[0], quiet, loud[1])))
            assert n % 64 and (n - 1) % 64
            reqs = [dict(clip=ids[0]), dict(clip=ids[1]), dict(clip=ids[2]),                             # the whole clips: the last group's tail is masked
                    dict(clip=ids[1], sub_frames=64), dict(clip=ids[1], first_frame=1, num_frames=n - 1, sub_frames=64),
                    dict(clip=ids[0], first_frame=3, num_frames=2998, sub_frames=100)]
            bad, outs = _check_batch(s, reqs, srcs)
            assert not bad, bad
            assert all(0.0 < max(outs[i]["peak"]) < 0.01 for i in (1, 3, 4)) and all(max(outs[i]["peak"]) == float(f32(7.9)) for i in (0, 2, 5))
            assert outs[3]["lufs"] < -40.0 < 0.0 < outs[0]["lufs"]
            for cid in ids:
                s.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [_clip(1 + i % 2, 60000 + 1001 * i, 40 + i, level=0.05 * (i + 1)) for i in range(8)]
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        bad, outs = _check_batch(s, [dict(clip=cid, first_frame=1, num_frames=x.shape[1] - 3, sub_frames=1000) for cid, x in zip(ids, srcs)], dict(zip(ids, srcs)))
        assert not bad, bad
        assert [o["sub_blocks"] for o in outs] == [(x.shape[1] - 3) // 1000 for x in srcs] and all(-30.0 < o["lufs"] < -5.0 for o in outs)
        assert all(a["lufs"] < b["lufs"] for a, b in zip(outs, outs[2:]))                  # (each louder than the last one with its channel count)


def test_loudness_follows_the_rendered_data(syn):
    """after a re-render (gain and pitch) and after a rate conversion the rendered extent is what gets measured"""
    from libzl_amd import ZlHipError
    src = _clip(2, 30000, 31)
    cid = _upload(syn, src)
    before = syn.clip_loudness(cid)
    assert lr.same(before, lr.measure(src, SR, coeffs=_coeffs(SR))[0])
    syn.rerender_clip(cid, gain_db=-6.0, pitch=3.0)
    played = _played(syn, cid)
    assert played.shape[1] == 30000 and not np.array_equal(played[:, :4000], src[:, :4000])
    bad, outs = _check_batch(syn, [dict(clip=cid), dict(clip=cid, first_frame=3, num_frames=played.shape[1] - 7, sub_frames=441)], {cid: played})
    assert not bad, bad
    assert abs(outs[0]["lufs"] - (before["lufs"] - 6.0)) < 1.0     # (the pitch moves the tone along the weighting curve a little)
    syn.rerender_clip(cid, speed=2.0)
    played = _played(syn, cid)
    assert played.shape[1] == 15000
    bad, _ = _check_batch(syn, [dict(clip=cid, first_frame=1)], {cid: played})
    assert not bad, bad
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_loudness(cid, 0, 15001)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert syn.clip_loudness(cid) == before
    syn.unregister_clip(cid)
    low = _clip(1, 22050, 32)
    cid = _upload(syn, low, 44100.0)
    a = syn.clip_loudness(cid)
    assert lr.same(a, lr.measure(low, 44100.0, coeffs=_coeffs(44100.0))[0]) and a["sub_blocks"] == 5
    syn.convert_clips([cid], SR)
    played = _played(syn, cid)
    assert syn.clip_info(cid)["sample_rate"] == SR and abs(played.shape[1] - 24000) <= 2
    bad, outs = _check_batch(syn, [dict(clip=cid), dict(clip=cid, first_frame=5, num_frames=23000, sub_frames=64)], {cid: played})
    assert not bad, bad
    assert abs(outs[0]["lufs"] - a["lufs"]) < 0.3                  # the same sound at another rate (the conversion's roll-off takes a little noise)
    syn.unregister_clip(cid)


def test_errors_leave_out_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = _clip(2, 20000, 8)
    cid = _upload(syn, src)
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    R, T = _abi.LoudnessRequest, _abi.Loudness
    out = (T * 20)()
    C.memset(out, 0x5A, C.sizeof(out))
    INV = _abi.ZLHIP_ERR_INVALID

    def untouched():
        return bytes(out) == b"\x5a" * C.sizeof(out)

    def single(*a):
        r = R(*a)
        rc = lib.zlhip_sound_loudness(e, C.byref(r), out)
        assert untouched(), a
        return rc

    def batch(reqs, nreq=None):
        arr = (R * max(1, len(reqs)))(*reqs)
        rc = lib.zlhip_sound_loudness_batch(e, arr, len(reqs) if nreq is None else nreq, out)
        assert untouched()
        return rc

    for bad in ((255, 0, 100, 0), (-1, 0, 100, 0), (256, 0, 100, 0), (gone, 0, 100, 0), (cid, 0, 0, 0), (cid, 0, -5, 0), (cid, -1, 10, 0),
                (cid, 1, 20000, 0), (cid, 20000, 1, 0), (cid, 0, 100, 15), (cid, 0, 100, -64), (cid, 0, 100, 131073)):
        assert single(*bad) == INV, bad
    big = np.zeros((1, 16 * 65537), f32)
    wide = _upload(syn, big)
    assert single(wide, 0, 16 * 65537, 16) == INV                  # 65537 sub-blocks in one request
    assert batch([R(wide, 0, 16 * 65536, 16)] * 16 + [R(cid, 0, 1, 0)]) == INV          # 1048577 in one call
    assert batch([R(cid, 0, 100, 0)], nreq=-1) == INV
    assert batch([R(cid, 0, 100, 0), R(200, 0, 100, 0)]) == INV    # one bad request fails the whole call (`gone`'s slot is wide's now)
    assert b"sound_loudness" in lib.zlhip_last_error(e)
    assert lib.zlhip_sound_loudness_batch(e, None, 1, out) == INV and lib.zlhip_sound_loudness_batch(e, (R * 1)(R(cid, 0, 100, 0)), 1, None) == INV
    n = C.c_int32(-77)
    assert lib.zlhip_debug_loudness_subs(e, 99, None, 0, C.byref(n)) == INV and n.value == -77
    # the limits themselves are fine
    assert batch([], nreq=0) == 0
    assert lib.zlhip_sound_loudness_batch(e, (R * 3)(R(cid, 0, 20000, 16), R(cid, 19999, 1, 131072), R(wide, 0, 16 * 65536, 16)), 3, out) == 0
    want = lr.measure(src, SR, 0, 20000, 16, coeffs=_coeffs(SR))[0]
    got = {k: (tuple(out[0].peak) if k == "peak" else getattr(out[0], k)) for k, _ in T._fields_}
    assert lr.same(got, want) and out[0].sub_blocks == 1250 and out[1].sub_blocks == 1 and out[2].sub_blocks == 65536 and out[2].above_absolute == 0
    assert bytes(out)[3 * 48:] == b"\x5a" * (17 * 48)
    rec = np.zeros(4, np.dtype([("sum", np.float64, 2), ("peak", f32, 2)]))
    assert lib.zlhip_debug_loudness_subs(e, 0, rec.ctypes.data, 4, C.byref(n)) == _abi.ZLHIP_ERR_CAPACITY and n.value == 1250 and not rec["sum"].any()
    for c in (cid, wide):
        syn.unregister_clip(c)


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _clip(2, 30000, 2))
        total0, _ = s.memory_bytes()
        s.clip_pitch(cid)
        total1, _ = s.memory_bytes()
        s.clip_loudness(cid)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_loudness(cid); s.clip_loudness(cid, 3, 20000, 100); s.clip_pitch(cid)       # fit the first call's buffers
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
    """After one warm-up call (it allocates the call's buffers) loudness calls between real-time cycles leave the resident kernel where
    it is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the results right."""
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
        # one more clip, which no voice plays
        tone = _clip(2, 6000, 5)
        extra = syn.register_clip(tone[0], tone[1], SR)
        assert extra == len(planar)
        planar.append(tone); rates.append(SR)

        def request(cid, k):
            n = planar[cid].shape[1]
            return dict(clip=cid, first_frame=min(k % 5, n - 1), num_frames=min(n - min(k % 5, n - 1), 3000), sub_frames=(64, 100, 256)[k % 3])

        # the warm-up call: more requests and items than any call below
        syn.clip_loudness_batch([dict(clip=i, sub_frames=16) for i in range(len(planar))] + [dict(clip=extra, sub_frames=16)] * 4)
        expect = {}
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts_after_first = None
        looping = [ev[1]["clip"] for ev in sc.events[0] if ev[1].get("looping")]      # started in block 0, play to the end
        todo = []
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
            # between the cycles: the loudness of clips that play, a single call and a batch in turn
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            reqs = [request(cid, k) for cid in playing[:2]] + [request(extra, k)]
            gots = [syn.clip_loudness_batch([r])[0] for r in reqs] if k % 2 else syn.clip_loudness_batch(reqs)
            todo += list(zip(reqs, gots))
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        keys = sorted({tuple(sorted(r.items())) for r, _ in todo})
        wants = lr.measure_batch([(planar[d["clip"]], rates[d["clip"]], d["first_frame"], d["num_frames"], d["sub_frames"], _coeffs(rates[d["clip"]])) for d in map(dict, keys)])
        expect = {key: w[0] for key, w in zip(keys, wants)}
        for r, got in todo:
            assert lr.same(got, expect[tuple(sorted(r.items()))]), (r, got, expect[tuple(sorted(r.items()))])
        assert len(todo) >= 2 * sc.nblocks and sum(g["above_absolute"] > 0 for _, g in todo) >= sc.nblocks
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


def test_group_loudness_equals_the_single_engine(syn):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    srcs = [_clip(1, 12000, 41), _clip(2, 20000, 42)]
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        for src in srcs:
            cid, gid = _upload(syn, src), _upload(g, src)
            for args in ((), (3, 9000, 100)):
                a = g.clip_loudness(gid, *args)
                assert a == syn.clip_loudness(cid, *args) and a["above_absolute"] > 0
            assert lr.same(a, lr.measure(src, SR, 3, 9000, 100, coeffs=_coeffs(SR))[0])
            syn.unregister_clip(cid)
        a, b = g.clip_loudness_batch([(0,), (1, 5, 1)])
        assert a["sub_blocks"] == 3 and b["sub_blocks"] == 1 and b["blocks"] == 1
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_loudness_batch([(0, 0, None, 15)])


def _predict_gain(res, current, target, ceiling):
    """libzl_hotpath_clip_normalize's arithmetic from a result of the restatement"""
    delta = float(f32(target)) - res["lufs"]
    peak = max(res["peak"])
    if peak > 0:
        delta = min(delta, float(f32(ceiling)) - 20.0 * math.log10(float(peak)))
    return f32(float(f32(current)) + delta)


def test_libzl_normalize_and_level(built, tmp_path):
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        lib = _abi.load()
        eng = C.c_void_p(zl.libzl_hotpath_engine())
        rng = np.random.default_rng(5)
        pad = _clip(2, 30000, 51, level=0.05)
        kick = (np.exp(-np.arange(30000) / 1500.0) * np.sin(2 * np.pi * 55.0 * np.arange(30000) / SR) * 0.9).astype(f32)[None, :]
        hot = _clip(1, 30000, 52, level=0.02)
        hot[0, 1000] = 0.99                                        # one full-scale click in a quiet clip: the ceiling binds
        silent = np.zeros((1, 30000), f32)
        clips = {}
        for name, src in (("pad", pad), ("kick", kick), ("hot", hot), ("silent", silent), ("pad2", pad)):
            path = str(tmp_path / (name + ".wav")).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, src[1].ctypes.data if src.shape[0] == 2 else None, src.shape[1], SR, 32) == 0
            clips[name] = zl.ClipAudioSource_new(path, False)
            assert clips[name]

        def played(clip):
            cid, cnt = zl.ClipAudioSource_engineClip(clip), C.c_int32(0)
            assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(cnt)) >= 0
            pl, pr_ = np.empty(cnt.value, f32), np.empty(cnt.value, f32)
            chans = lib.zlhip_sound_read(eng, cid, pl.ctypes.data, pr_.ctypes.data, cnt.value, C.byref(cnt))
            return np.stack([pl, pr_]) if chans == 2 else pl[None, :]

        def ref(clip):
            return lr.measure(played(clip), SR, coeffs=_coeffs(SR))[0]

        lufs, peak, gain = C.c_double(7.0), C.c_float(7.0), C.c_float(7.0)
        assert zl.libzl_hotpath_clip_loudness(None, C.byref(lufs), C.byref(peak)) < 0 and lufs.value == 7.0
        assert zl.libzl_hotpath_clip_normalize(clips["pad"], float("nan"), -1.0, C.byref(gain)) == _abi.ZLHIP_ERR_INVALID
        assert zl.libzl_hotpath_clip_normalize(clips["pad"], -16.0, float("nan"), C.byref(gain)) == _abi.ZLHIP_ERR_INVALID and gain.value == 7.0
        want = ref(clips["pad"])
        assert np.array_equal(played(clips["pad"]), pad)
        assert zl.libzl_hotpath_clip_loudness(clips["pad"], C.byref(lufs), C.byref(peak)) == 1
        assert abs(lufs.value - want["lufs"]) <= 1e-9 and f32(peak.value) == f32(20.0 * math.log10(max(want["peak"])))
        assert zl.libzl_hotpath_clip_loudness(clips["silent"], C.byref(lufs), C.byref(peak)) == 0 and lufs.value == -math.inf and peak.value == -math.inf
        assert zl.libzl_hotpath_clip_normalize(clips["silent"], -16.0, -1.0, C.byref(gain)) == 0 and gain.value == 7.0

        # to -16 LUFS: exactly the gain the restatement predicts, and the re-measured loudness lands on the target
        assert zl.libzl_hotpath_clip_normalize(clips["pad"], -16.0, -1.0, C.byref(gain)) == 1
        g1 = _predict_gain(want, 0.0, -16.0, -1.0)
        assert f32(gain.value) == g1 and 5.0 < g1 < 30.0
        after = ref(clips["pad"])
        assert zl.libzl_hotpath_clip_loudness(clips["pad"], C.byref(lufs), C.byref(peak)) == 1
        print("pad: gain", gain.value, "lufs", lufs.value, "off target by", lufs.value + 16.0)
        assert abs(lufs.value - after["lufs"]) <= 1e-9 and abs(lufs.value - (-16.0)) <= 1e-4
        # again, to another target: the measured data carries the first gain, the new gain is the sum
        assert zl.libzl_hotpath_clip_normalize(clips["pad"], -23.0, -1.0, C.byref(gain)) == 1
        assert f32(gain.value) == _predict_gain(after, g1, -23.0, -1.0)
        assert zl.libzl_hotpath_clip_loudness(clips["pad"], C.byref(lufs), C.byref(peak)) == 1
        print("pad: gain", gain.value, "lufs", lufs.value, "off target by", lufs.value + 23.0)
        assert abs(lufs.value - (-23.0)) <= 1e-4
        # the ceiling binds: the click ends at -1 dBFS and the loudness stays under the target
        want = ref(clips["hot"])
        assert zl.libzl_hotpath_clip_normalize(clips["hot"], -10.0, -1.0, C.byref(gain)) == 1
        assert f32(gain.value) == _predict_gain(want, 0.0, -10.0, -1.0) and abs(gain.value - (-1.0 - 20.0 * math.log10(0.99))) < 1e-3
        assert zl.libzl_hotpath_clip_loudness(clips["hot"], C.byref(lufs), C.byref(peak)) == 1 and abs(peak.value - (-1.0)) < 1e-3 and lufs.value < -20.0

        # a bank: four clips with one silent and one NULL, one loudness call and one re-render call (-30 LUFS: the kick's peak is 21 dB
        # above its loudness, so a higher target would be held by the ceiling)
        bank = [clips["kick"], None, clips["silent"], clips["pad2"]]
        wants = [ref(c) if c else None for c in bank]
        arr = (C.c_void_p * 4)(*bank)
        gains = (C.c_float * 4)(9.0, 9.0, 9.0, 9.0)
        assert zl.libzl_hotpath_clips_level(arr, 4, -30.0, -0.5, gains) == 2
        assert f32(gains[0]) == _predict_gain(wants[0], 0.0, -30.0, -0.5) and f32(gains[3]) == _predict_gain(wants[3], 0.0, -30.0, -0.5)
        assert gains[1] == 0.0 and gains[2] == 0.0
        for c in (bank[0], bank[3]):
            assert zl.libzl_hotpath_clip_loudness(c, C.byref(lufs), C.byref(peak)) == 1 and abs(lufs.value - (-30.0)) <= 1e-4, lufs.value
        assert np.array_equal(played(clips["silent"]), silent)
        dup = (C.c_void_p * 3)(clips["kick"], clips["pad2"], clips["kick"])
        gains[0] = 9.0
        assert zl.libzl_hotpath_clips_level(dup, 3, -18.0, -0.5, gains) == _abi.ZLHIP_ERR_INVALID and gains[0] == 9.0
        assert zl.libzl_hotpath_clips_level(arr, 4, float("nan"), -0.5, gains) == _abi.ZLHIP_ERR_INVALID
        assert zl.libzl_hotpath_clips_level(None, 0, -18.0, -0.5, None) == 0
        for clip in clips.values():
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
