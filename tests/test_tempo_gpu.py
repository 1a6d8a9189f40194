"""Tempo estimate on the device (zlhip_sound_tempo / _batch, include/zlhip.h): the flux W and the autocorrelation A
(zlhip_debug_tempo_acf), the whole integer record, and bpm and confidence with ==, against the numpy / Python-integer restatement
(tests/tempo_ref.py) -- over channel counts, hop sizes, unaligned sub-ranges, hops at the segment's edges, loud and special values,
several segments and lag tiles, the largest request, neighbouring clips, re-rendered clips, a grown arena, batches, errors -- and the
call's place next to the resident real-time kernel, in the engine group and behind the libzl-named layer."""
import ctypes as C
import os

import numpy as np
import pytest

import stretch_ref
import tempo_ref as tr
from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 48000.0
INTS = ("lag_coarse", "lag_fine", "doublings", "shift", "hops", "acf_lo", "acf_mid", "acf_hi", "acf_zero", "sum")


def _pulsed_noise(ch, length, seed, period=23000, level=0.3):
    """noise under a train of decaying pulses: a flux with a period, and something in every hop"""
    rng = np.random.default_rng(seed)
    env = 0.02 + np.exp(-(np.arange(length) % period) / 2500.0)
    return (rng.uniform(-level, level, (ch, length)) * env).astype(f32)


def _upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def _matches(got, want):
    """the whole record: the integers, and bpm and confidence with =="""
    return all(got[k] == want[k] for k in INTS) and f32(got["bpm"]) == want["bpm"] and f32(got["confidence"]) == want["confidence"]


def _check_batch(syn, reqs, srcs, rates=None):
    """reqs: (clip, first, n, hop, bpm_min, bpm_max); srcs: {clip: planar}.  W, A and the record of every request against the
    restatement; returns the mismatches and the records"""
    bad = []
    outs = syn.clip_tempo_batch(reqs)
    for i, (r, got) in enumerate(zip(reqs, outs)):
        cid, first, n, hop, lo, hi = r
        rec, W, first_lag, A = tr.tempo(srcs[cid], (rates or {}).get(cid, SR), first, n, hop, lo, hi)
        gW, gfirst, gA = syn.tempo_acf(i)
        okW = gW.dtype == np.uint16 and np.array_equal(gW, W)
        okA = gA.dtype == np.uint64 and [int(v) for v in gA] == A and (len(A) == 0 or gfirst == first_lag)
        if not (okW and okA and _matches(got, rec)):
            bad.append((srcs[cid].shape, r, "W" if not okW else "A" if not okA else ("record", got, rec)))
    return bad, outs


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_grid_equals_the_restatement(syn, ch):
    """first frame 1, 3, 5; 3, 130, 257, 4096 and 4097 hops (one and two segments, too short for a tempo and not), the last hop whole
    and cut; hop 64 and 256"""
    src = _pulsed_noise(ch, 4097 * 256 + 8, 10 + ch)
    cid = _upload(syn, src)
    reqs = [(cid, first, hops * hop - (7 if hops % 2 else 0), hop, 0.0, 0.0) for first in (1, 3, 5) for hops in (3, 130, 257, 4096, 4097) for hop in (64, 256)]
    bad, outs = _check_batch(syn, reqs, {cid: src})
    assert not bad, (len(bad), bad[:4])
    assert [o["hops"] for o in outs[:10]] == [3, 3, 130, 130, 257, 257, 4096, 4096, 4097, 4097]
    assert sum(1 for o in outs if o["lag_fine"] > 0) >= 15 and sum(1 for o in outs if o["lag_fine"] == 0) >= 6
    # 23000 frames per pulse: 89.84 hops of 256
    assert all(abs(o["bpm"] - 60 * SR / 23000) < 0.5 for o, r in zip(outs, reqs) if r[3] == 256 and o["hops"] >= 4096)
    syn.unregister_clip(cid)


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                    0x39000000, 0x38FFFFFF, 0x39C00000, 0xB9C00000, 0x3A200000], np.uint32)


def test_a_loud_clip_and_special_values(syn):
    """full scale in both channels: R reaches 2^20 and the shift is 4; NaN, +-inf, -0 and denormals are quantised as section 12 defines"""
    rng = np.random.default_rng(3)
    loud = (rng.choice([-7.9, 7.9], (2, 300000)) * (0.05 + (np.arange(300000) % 24000 < 3000))).astype(f32)
    cid = _upload(syn, loud)
    bad, outs = _check_batch(syn, [(cid, 0, 300000, 0, 0.0, 0.0), (cid, 5, 299001, 64, 60.0, 200.0)], {cid: loud})
    assert not bad, bad
    assert outs[0]["shift"] == 4 and outs[0]["lag_fine"] > 0 and abs(outs[0]["bpm"] - 120.0) < 0.25
    syn.unregister_clip(cid)
    for ch in (1, 2):
        src = rng.permutation(np.tile(SPECIAL, 5000))[:50000 * ch].reshape(ch, -1).view(f32)
        cid = _upload(syn, src)
        bad, outs = _check_batch(syn, [(cid, 0, 50000, 64, 0.0, 0.0), (cid, 1, 49997, 80, 100.0, 400.0), (cid, 3, 49001, 256, 0.0, 0.0)], {cid: src})
        assert not bad, bad
        assert outs[0]["acf_zero"] > 0
        syn.unregister_clip(cid)


def test_several_hop_segments_and_lag_tiles(syn):
    """9000 hops of 64 frames with l_max = 1024: three segments, the lags 299 .. 4500 in 17 tiles, atomic sums"""
    src = _pulsed_noise(1, 9000 * 64 + 5, 21, period=700 * 64)
    cid = _upload(syn, src)
    assert tr.lags(SR, 64, float(f32(43.945)), 150.0, 9000) == (300, 1024, 4499)
    bad, outs = _check_batch(syn, [(cid, 5, 9000 * 64, 64, 43.945, 150.0)], {cid: src})
    assert not bad, bad
    W, first_lag, A = syn.tempo_acf(0)
    assert first_lag == 299 and len(A) == 4500 - 299 + 1 and outs[0]["lag_coarse"] == 700 and outs[0]["doublings"] == 2
    syn.unregister_clip(cid)


def test_one_request_of_65536_hops(syn):
    n = 65536 * 64
    src = _pulsed_noise(1, n + 3, 65, period=500 * 64, level=0.5)
    cid = _upload(syn, src)
    bad, outs = _check_batch(syn, [(cid, 3, n, 64, 0.0, 0.0)], {cid: src})
    assert not bad, bad
    assert outs[0]["hops"] == 65536 and outs[0]["lag_coarse"] == 500 and outs[0]["doublings"] == 3 and len(syn.tempo_acf(0)[2]) == 8 * 600 + 8 - 299 + 1
    syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a small arena that held noise: a neighbour's frame in a head or tail group, or a
    hop of a neighbour's W in a staged window, would change the sums (a full-scale frame is 10^6 times a quiet one)"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=4 << 20) as s:
        rng = np.random.default_rng(9)
        fill = [_upload(s, rng.uniform(-7.9, 7.9, (ch, 120000)).astype(f32)) for _ in range(3)]
        for cid in fill:
            s.unregister_clip(cid)
        for n in (60001, 33333):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (30001, 30003)]
            quiet = _pulsed_noise(ch, n, n, period=6000, level=0.005)
            ids = [_upload(s, x) for x in (loud[0], quiet, loud[1])]
            srcs = dict(zip(ids, (loud[0], quiet, loud[1])))
            # the quiet request sits between two loud ones in the call's W and A too
            reqs = [(ids[0], 0, 30001, 64, 200.0, 400.0), (ids[1], 0, n, 64, 200.0, 400.0), (ids[2], 0, 30003, 64, 200.0, 400.0),
                    (ids[0], 1, 30000, 80, 0.0, 0.0), (ids[1], 1, n - 2, 80, 240.0, 400.0), (ids[2], 3, 30000, 80, 0.0, 0.0)]
            bad, outs = _check_batch(s, reqs, srcs)
            assert not bad, bad
            assert outs[1]["shift"] == 0 and outs[1]["lag_fine"] > 0 and outs[0]["shift"] > 0
            for cid in ids:
                s.unregister_clip(cid)


def test_a_batch_of_64_equals_64_single_calls(syn):
    from libzl_amd import _abi
    rng = np.random.default_rng(23)
    srcs = [_pulsed_noise(1 + i % 2, int(rng.integers(30000, 200000)), 500 + i, period=int(rng.integers(15000, 30000))) for i in range(14)]
    srcs += [np.zeros((2, 100000), f32), _pulsed_noise(1, 5000, 77)]              # silence, and a clip too short for any range
    ids = [_upload(syn, x) for x in srcs]
    reqs = []
    for i in range(64):
        k = i % 16
        length = srcs[k].shape[1]
        first = int(rng.integers(0, length // 4))
        n = int(rng.integers(length // 2, length - first + 1))
        lo, hi = [(0.0, 0.0), (60.0, 120.0), (100.0, 200.0), (150.0, 400.0)][(i // 16) % 4]      # several ranges over one clip
        reqs.append((ids[k], first, n, int(rng.choice([0, 64, 80, 256, 1024])), lo, hi))
    arr = (_abi.TempoRequest * 64)(*[_abi.TempoRequest(*r) for r in reqs])
    out = (_abi.Tempo * 67)()                                      # three sentinels behind what the call may write
    C.memset(out, 0x5A, C.sizeof(out))
    assert syn._lib.zlhip_sound_tempo_batch(syn._e, arr, 64, out) == 0
    assert bytes(out)[64 * 72:] == b"\x5a" * (3 * 72)
    batch = [{k: getattr(out[i], k) for k in INTS + ("bpm", "confidence", "reserved")} for i in range(64)]
    found = 0
    for i, (r, k) in enumerate(zip(reqs, [i % 16 for i in range(64)])):
        single = syn.clip_tempo(*r)
        want = tr.tempo(srcs[k], SR, *r[1:])[0]
        assert _matches(single, want) and _matches(batch[i], want) and batch[i]["reserved"] == 0, (i, r, batch[i], want)
        if k >= 14:                                                # no tempo, as defined: everything 0 except hops, shift, sum and acf_zero
            assert batch[i]["bpm"] == 0.0 and batch[i]["confidence"] == 0.0 and all(batch[i][f] == 0 for f in ("lag_coarse", "lag_fine", "doublings", "acf_lo", "acf_mid", "acf_hi"))
            assert batch[i]["hops"] > 0 and (batch[i]["acf_zero"] > 0) == (k == 15)
        found += batch[i]["lag_fine"] > 0
    assert found >= 40
    for cid in ids:
        syn.unregister_clip(cid)


def test_pattern_a_at_120_bpm(syn):
    src = tr.pattern_a(SR, 4.0, 120)
    cid = _upload(syn, src)
    got = syn.clip_tempo(cid)
    assert _matches(got, tr.tempo(src, SR)[0])
    print(got)
    assert abs(got["bpm"] - 120.0) <= 0.25 and got["confidence"] >= 0.4
    syn.unregister_clip(cid)


def test_tempo_follows_the_rerender(syn):
    src = np.concatenate([tr.pattern_a(SR, 6.0, 100), tr.pattern_b(SR, 6.0, 100)])
    cid = _upload(syn, src)
    before = syn.clip_tempo(cid)
    assert _matches(before, tr.tempo(src, SR)[0]) and abs(before["bpm"] - 100.0) <= 0.25
    syn.rerender_clip(cid, speed=1.25)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert played.shape[1] == 230400
    ext = syn.clip_extent(cid)                                     # the extent as it lies in the arena: the frames that play, then zeros
    assert np.array_equal(ext[:2 * 230400].reshape(-1, 2).T, played) and not ext[2 * 230400:].any()
    now = syn.clip_tempo(cid)
    assert _matches(now, tr.tempo(played, SR)[0]) and not _matches(now, before)
    bad, _ = _check_batch(syn, [(cid, 3, 230000, 80, 90.0, 180.0)], {cid: played})
    assert not bad, bad
    from libzl_amd import ZlHipError
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_tempo(cid, 0, 288000)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert _matches(syn.clip_tempo(cid), before) and _matches(syn.clip_tempo(cid, 0, 288000), before)
    syn.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [_pulsed_noise(1 + i % 2, 60000 + 1001 * i, 40 + i, period=20000 + 500 * i) for i in range(8)]
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        bad, outs = _check_batch(s, [(cid, 1, x.shape[1] - 3, 80, 100.0, 200.0) for cid, x in zip(ids, srcs)], dict(zip(ids, srcs)))
        assert not bad, bad
        assert all(o["lag_fine"] > 0 for o in outs)


def test_errors_leave_out_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = _pulsed_noise(2, 50000, 8)
    cid = _upload(syn, src)
    big = _upload(syn, np.zeros((1, 65536 * 64 + 64), f32))
    fast = _upload(syn, src, 192000.0)
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    R, T = _abi.TempoRequest, _abi.Tempo
    out = (T * 70)()
    C.memset(out, 0x5A, C.sizeof(out))
    INV = _abi.ZLHIP_ERR_INVALID

    def untouched():
        return bytes(out) == b"\x5a" * C.sizeof(out)

    def single(*a):
        r = R(*a)
        rc = lib.zlhip_sound_tempo(e, C.byref(r), out)
        assert untouched(), a
        return rc

    def batch(reqs, nreq=None):
        arr = (R * max(1, len(reqs)))(*reqs)
        rc = lib.zlhip_sound_tempo_batch(e, arr, len(reqs) if nreq is None else nreq, out)
        assert untouched()
        return rc

    ok = (cid, 0, 50000, 256, 75.0, 150.0)
    assert single(255, *ok[1:]) == INV and single(-1, *ok[1:]) == INV and single(256, *ok[1:]) == INV and single(gone, *ok[1:]) == INV
    for hop in (48, 63, 65, 72, 4097, 4112, -256):
        assert single(cid, 0, 50000, hop, 75.0, 150.0) == INV, hop
    for lo, hi in ((19.99, 150.0), (75.0, 400.01), (150.0, 150.0), (150.0, 75.0), (-75.0, 150.0), (float("nan"), 150.0), (75.0, float("nan")),
                   (75.0, float("inf")), (float("-inf"), 150.0)):
        assert single(cid, 0, 50000, 256, lo, hi) == INV, (lo, hi)
    assert single(cid, 0, 50000, 64, 43.9, 150.0) == INV           # l_max = 1025
    assert single(fast, 0, 50000, 64, 0.0, 0.0) == INV             # 192 kHz at hop 64: l_max = 2400
    assert single(cid, 0, 0, *ok[3:]) == INV and single(cid, 0, -5, *ok[3:]) == INV and single(cid, -1, 10, *ok[3:]) == INV
    assert single(cid, 1, 50000, *ok[3:]) == INV and single(cid, 50000, 1, *ok[3:]) == INV      # past the end
    assert single(big, 0, 65536 * 64 + 1, 64, 75.0, 150.0) == INV                              # 65537 hops
    assert batch([R(big, 0, 65536 * 64, 64, 75.0, 150.0)] * 64 + [R(cid, 0, 1, 64, 75.0, 150.0)]) == INV      # 4 Mi + 1 hops in one call
    assert batch([R(*ok)], nreq=-1) == INV
    assert batch([R(*ok), R(gone, *ok[1:])]) == INV                # one bad request fails the whole call
    assert b"sound_tempo" in lib.zlhip_last_error(e)
    assert lib.zlhip_sound_tempo_batch(e, None, 1, out) == INV and lib.zlhip_sound_tempo_batch(e, (R * 1)(R(*ok)), 1, None) == INV
    n = C.c_int32(-77)
    assert lib.zlhip_debug_tempo_acf(e, 99, None, None, 0, C.byref(n), C.byref(n), C.byref(n)) == INV and n.value == -77
    # the limits themselves are fine
    assert batch([], nreq=0) == 0
    assert lib.zlhip_sound_tempo_batch(e, (R * 2)(R(*ok), R(cid, 0, 50000, 64, 43.945, 400.0)), 2, out) == 0
    want = tr.tempo(src, SR, *ok[1:])[0]
    assert _matches({k: getattr(out[0], k) for k in INTS + ("bpm", "confidence")}, want) and bytes(out)[2 * 72:] == b"\x5a" * (68 * 72)
    W = np.zeros(4, np.uint16)
    h = C.c_int32(0)
    assert lib.zlhip_debug_tempo_acf(e, 0, W.ctypes.data, None, 4, C.byref(h), None, None) == _abi.ZLHIP_ERR_CAPACITY and h.value == 196 and not W.any()
    for c in (cid, big, fast):
        syn.unregister_clip(c)


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _pulsed_noise(2, 50000, 2))
        total0, _ = s.memory_bytes()
        s.clip_onsets(cid)
        total1, _ = s.memory_bytes()
        s.clip_tempo(cid)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_tempo(cid); s.clip_tempo(cid, 3, 40000, 64, 100.0, 200.0); s.clip_onsets(cid)     # fit the first call's buffers
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
    """After one warm-up call (it allocates the call's buffers) tempo calls between real-time cycles leave the resident kernel where it
    is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the records right."""
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

        # the scene's clips are too short for any range (no tempo, which is checked too); one more clip, which no voice plays, has one
        extra = syn.register_clip(tr.pattern_a(SR, 2.0, 120)[0], None, SR)
        assert extra == len(planar)
        planar.append(tr.pattern_a(SR, 2.0, 120)); rates.append(SR)

        def params(cid, k):
            p = [(0, 0.0, 0.0), (256, 200.0, 400.0), (0, 300.0, 400.0)][k % 3]
            return p if tr.resolve(rates[cid], planar[cid].shape[1], *p) is not None else (0, 0.0, 0.0)

        # the warm-up call: every clip twice, more hops, lags and requests than any call below
        syn.clip_tempo_batch([(i, 0, None, 0, 300.0, 400.0) for i in range(len(planar))] + [(i, 0, None, *params(i, 1)) for i in range(len(planar))]
                             + [(extra, 0, None, 64, 75.0, 400.0)])
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
            # between the cycles: the tempo of clips that play, a single call and a batch in turn
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            reqs = [(cid, 0, None, *params(cid, k)) for cid in playing[:2]] + [(extra, k % 5, 90000, (0, 64)[k % 2], 0.0, (0.0, 200.0)[k % 3 == 0])]
            gots = [syn.clip_tempo(*r) for r in reqs] if k % 2 else syn.clip_tempo_batch(reqs)
            for r, got in zip(reqs, gots):
                if r not in expect:
                    expect[r] = tr.tempo(planar[r[0]], rates[r[0]], *r[1:])[0]
                assert _matches(got, expect[r]), (k, r, got, expect[r])
                checked += 1
                found += got["lag_fine"] > 0
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        assert checked >= 2 * sc.nblocks and found >= sc.nblocks
        print("requests with a tempo:", found, "of", checked)
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


def test_group_tempo_equals_the_single_engine(syn):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    srcs = [tr.pattern_a(SR, 4.0, 128), np.concatenate([tr.pattern_b(SR, 3.0, 90), tr.pattern_a(SR, 3.0, 90)])]
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        for src in srcs:
            cid, gid = _upload(syn, src), _upload(g, src)
            for args in ((), (3, 100000, 80, 60.0, 180.0)):
                a = g.clip_tempo(gid, *args)
                assert _matches(a, syn.clip_tempo(cid, *args)) and a["lag_fine"] > 0
            assert _matches(a, tr.tempo(src, SR, 3, 100000, 80, 60.0, 180.0)[0])
            syn.unregister_clip(cid)
        a, b = g.clip_tempo_batch([(0,), (1, 5, 1000)])
        assert abs(a["bpm"] - 128.0) <= 0.25 and b["lag_fine"] == 0 and b["hops"] == 4
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_tempo_batch([(0, 0, None, 65)])


def test_libzl_clip_tempo_and_match_tempo(built, tmp_path):
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        src = np.concatenate([tr.pattern_a(SR, 6.0, 100, seed=5), tr.pattern_a(SR, 6.0, 100, seed=6)])
        length = src.shape[1]
        path = str(tmp_path / "a.wav").encode()
        assert zl.libzl_wav_write(path, src[0].ctypes.data, src[1].ctypes.data, length, SR, 32) == 0
        c = zl.ClipAudioSource_new(path, False)
        assert c
        lib = _abi.load()
        eng, cid = C.c_void_p(zl.libzl_hotpath_engine()), zl.ClipAudioSource_engineClip(c)

        def played():
            n = C.c_int32(0)
            assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(n)) >= 0
            L = np.empty(n.value, f32); R = np.empty(n.value, f32)
            assert lib.zlhip_sound_read(eng, cid, L.ctypes.data, R.ctypes.data, n.value, C.byref(n)) == 2
            return np.stack([L, R])

        def detect(lo=0.0, hi=0.0):
            bpm, conf = C.c_float(-1.0), C.c_float(-1.0)
            assert zl.libzl_hotpath_clip_tempo(c, lo, hi, C.byref(bpm), C.byref(conf)) == 0
            return f32(bpm.value), f32(conf.value)

        bpm, conf = C.c_float(-1.0), C.c_float(-1.0)
        assert zl.libzl_hotpath_clip_tempo(None, 0.0, 0.0, C.byref(bpm), C.byref(conf)) < 0
        assert zl.libzl_hotpath_clip_tempo(c, 150.0, 75.0, C.byref(bpm), C.byref(conf)) < 0 and bpm.value == -1.0 and conf.value == -1.0
        want = tr.tempo(src, SR)[0]
        assert detect() == (want["bpm"], want["confidence"]) and abs(float(want["bpm"]) - 100.0) <= 0.25
        wide = tr.tempo(src, SR, bpm_min=150.0, bpm_max=300.0)[0]
        assert detect(150.0, 300.0) == (wide["bpm"], wide["confidence"])
        # below the confidence asked for: nothing changes
        ratio = C.c_float(-1.0)
        assert zl.libzl_hotpath_clip_match_tempo(c, 120.0, 2.0, C.byref(ratio)) == 0 and ratio.value == -1.0
        assert played().shape[1] == length and detect() == (want["bpm"], want["confidence"])
        assert zl.libzl_hotpath_clip_match_tempo(c, 0.0, 0.3, C.byref(ratio)) < 0 and zl.libzl_hotpath_clip_match_tempo(None, 120.0, 0.3, C.byref(ratio)) < 0
        # to 120 bpm: the ratio, the length of what plays, and what plays
        assert zl.libzl_hotpath_clip_match_tempo(c, 120.0, 0.3, C.byref(ratio)) == 1
        assert f32(ratio.value) == f32(120.0 * 1.0 / float(want["bpm"]))
        now = played()
        assert now.shape[1] == int(np.floor(length / float(f32(ratio.value))))
        stretched = stretch_ref.render(src, SR, speed=float(f32(ratio.value)))[0]
        assert np.array_equal(now.view(np.int32), stretched.view(np.int32))
        again = tr.tempo(stretched, SR)[0]
        assert detect() == (again["bpm"], again["confidence"])
        zl.ClipAudioSource_destroy(c)
    finally:
        zl.shutdownJuce()
