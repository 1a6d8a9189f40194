"""Transient detection on the device (zlhip_sound_onsets / _batch, include/zlhip.h): the onsets, the hops' energy E and the novelty N
(zlhip_debug_onset_hops) against the numpy / Python-integer restatement (tests/onset_ref.py) bit for bit -- over lengths, channel
counts, hop sizes and sub-ranges at every alignment, special values, neighbouring clips, re-rendered clips, a grown arena, batches,
errors -- what the definition does to a scene of bursts, and the call's place next to the resident real-time kernel, in the engine
group and behind the libzl-named layer."""
import ctypes as C
import os

import numpy as np
import pytest

import onset_ref as onr
from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu
f32 = np.float32

LENGTHS = (1, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 4099, 70001)
FIRSTS = (0, 1, 2, 3, 5)
SHORT = (0, 1, 2, 3)
HOPS = (64, 80, 256, 4096)
SR = 48000.0
DEFAULTS = dict(hop=256, gate=8, threshold=128, min_gap=10, max_onsets=128)      # at 48 kHz (tests/test_onset_cpu.py::test_defaults)


def _noise_with_bursts(ch, length, seed):
    """quiet noise with a few loud stretches, so that onsets exist"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.01, 0.01, (ch, length))
    for p in rng.integers(0, length, 1 + length // 3000):
        n = min(length - p, 400)
        x[:, p:p + n] += rng.uniform(-0.8, 0.8, (ch, n)) * np.exp(-np.arange(n) / 120.0)
    return x.astype(f32)


def _upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def _check_batch(syn, reqs, srcs):
    """reqs: (clip, first, n, hop, gate, threshold, min_gap, max_onsets) with every field given; srcs: {clip: planar}.  Onsets, E and N
    of every request against the restatement; returns the mismatches"""
    bad = []
    outs = syn.clip_onsets_batch(reqs)
    for i, (r, got) in enumerate(zip(reqs, outs)):
        cid, first, n, hop, gate, thr, gap, keep = r
        want, E, N = onr.onsets(srcs[cid], first, n, hop, gate, thr, gap, keep)
        gE, gN = syn.onset_hops(i)
        if not (_same(gE, E) and _same(gN, N) and _same(got, want)):
            bad.append((srcs[cid].shape, r, "E" if not _same(gE, E) else "N" if not _same(gN, N) else "onsets"))
    return bad


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=256, sound_arena_bytes=64 << 20)
    yield s
    s.close()


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_grid_equals_the_restatement(syn, ch):
    """first frame 0, 1, 2, 3, 5 and a last frame 0, 1, 2, 3 short of the end, hops that are and are not multiples of the wave's reach:
    the head and tail of misaligned 16-byte groups are masked, at the request's edges and at every hop edge"""
    bad, total = [], 0
    for length in LENGTHS:
        src = _noise_with_bursts(ch, length, 100 * length + ch)
        cid = _upload(syn, src)
        reqs = [(cid, first, length - first - short, hop, 8, 128, 2, 16) for first in FIRSTS for short in SHORT for hop in HOPS
                if length - first - short >= 1]
        bad += _check_batch(syn, reqs, {cid: src})
        total += sum(len(o) for o in syn.clip_onsets_batch(reqs[:4]))
        syn.unregister_clip(cid)
    assert not bad, (len(bad), bad[:10])
    assert total > 0                                               # onsets exist


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_thousands_of_candidates_and_ties(syn, ch):
    """threshold 1 and min_gap 1 on plain noise: a third of the hops are candidates, their strengths repeat, max_onsets cuts through
    a strength"""
    src = np.random.default_rng(77 + ch).uniform(-0.5, 0.5, (ch, 600001)).astype(f32)
    cid = _upload(syn, src)
    reqs = [(cid, 0, 600001, 64, 8, 1, 1, 1024), (cid, 3, 599990, 64, 8, 1, 1, 100), (cid, 1, 600000, 80, 1, 1, 2, 1), (cid, 0, 70001, 64, 8, 1, 1, 1024)]
    N = onr.onsets(src, 0, 600001, 64, 8, 1, 1, 1024)[2]
    cand = onr.candidates(N, 1, 1)
    assert len(cand) > 2000
    kept = onr.select(N, cand, 1024)
    cut = min(int(N[h]) for h in kept)
    assert sum(1 for h in cand if N[h] == cut) > sum(1 for h in kept if N[h] == cut) > 0      # the cut-off strength is shared: ties are broken
    bad = _check_batch(syn, reqs, {cid: src})
    assert not bad, bad
    syn.unregister_clip(cid)


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                    0x39000000, 0x38FFFFFF, 0x39C00000, 0xB9C00000, 0x3A200000], np.uint32)      # ... and ties of rint: 0.5, just below, 1.5, -1.5, 2.5


def test_special_values_are_quantised_as_defined(syn):
    """+-0 and denormals are 0, +-inf and +-FLT_MAX clamp to +-32767, NaNs of both signs are 0, halves round to even"""
    assert list(onr.quantise(SPECIAL.view(f32))) == [0, 0, 0, 0, 0, 0, 32767, -32767, 0, 0, 0, 0, 4096, -4096, 32767, -32767, 0, 0, 2, -2, 2]
    rng = np.random.default_rng(5)
    for ch in (1, 2):
        src = rng.permutation(np.tile(SPECIAL, 120))[:1100 * ch].reshape(ch, -1).view(f32)
        cid = _upload(syn, src)
        bad = _check_batch(syn, [(cid, 0, 1100, 64, 8, 1, 1, 64), (cid, 1, 1097, 80, 1, 1, 2, 8), (cid, 3, 1001, 256, 8, 128, 1, 8)], {cid: src})
        assert not bad, bad
        # one value per hop-sized run: E is its square times the run
        for k, bits in enumerate(SPECIAL):
            one = np.full((ch, 64), bits, np.uint32).view(f32)
            c1 = _upload(syn, one)
            syn.clip_onsets(c1, 0, 64, 64, 8, 128, 1, 1)
            q = int(onr.quantise(one[0, :1])[0])
            assert int(syn.onset_hops(0)[0][0]) == 64 * ch * q * q, hex(int(bits))
            syn.unregister_clip(c1)
        syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a fresh small arena: a neighbour's frame or a pad zero in a head or tail group would
    change E (a full-scale frame is 10^6 times a quiet one) and make an onset"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=1 << 20) as s:
        rng = np.random.default_rng(9)
        for n in (1001, 777, 1003, 64, 65):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (1001, 1003)]
            quiet = rng.uniform(0.004, 0.006, (ch, n)).astype(f32)
            ids = [_upload(s, x) for x in (loud[0], quiet, loud[1])]
            for hop in (64, 80, 256):
                for first, m in ((0, n), (1, n - 2), (0, n - 1), (3, n - 3), (n - 5, 5)):
                    got = s.clip_onsets(ids[1], first, m, hop, 1, 64, 1, 16)
                    want, E, N = onr.onsets(quiet, first, m, hop, 1, 64, 1, 16)
                    gE, gN = s.onset_hops(0)
                    assert _same(gE, E) and _same(gN, N), (n, hop, first, m)
                    # the rise from E[-1] = 0 at the request's first hop is the only one there can be
                    assert _same(got, want) and all(f == first for f, _ in got), (n, hop, first, m, got)
                    assert len(s.clip_onsets(ids[1], first, m, hop, 64, 64, 1, 16)) == 0      # below the gate: no onset at all
            for cid in ids:
                s.unregister_clip(cid)


# ---- the scene of bursts ------------------------------------------------------------------------------------------------------------
BURSTS = (0, 24000, 50011, 77777, 100003, 150000)


def _burst_scene(ch, sine, length=192000, seed=1):
    rng = np.random.default_rng(seed)
    x = np.zeros((ch, length))
    for p in (p for p in BURSTS if p < length):
        n = min(length - p, 12000)
        x[:, p:p + n] += rng.uniform(-0.5, 0.5, (ch, n)) * np.exp(-np.arange(n) / 1500.0)
    if sine:
        x += 10 ** (-30 / 20) * np.sin(2 * np.pi * 220.0 * np.arange(length) / SR)
    return x.astype(f32)


@pytest.fixture(scope="module")
def burst_clips(syn):
    table = {}
    for ch in (1, 2):
        for sine in (False, True):
            src = _burst_scene(ch, sine)
            table[(ch, sine)] = (_upload(syn, src), src)
    return table


@pytest.mark.parametrize("sine", [False, True], ids=["silence", "sine"])
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_the_burst_scene(syn, burst_clips, ch, sine):
    """decaying noise bursts, with and without a 220 Hz sine at -30 dB under them, with the defaults: every burst comes back once,
    within S = hop / 16 frames of where it begins"""
    cid, src = burst_clips[(ch, sine)]
    got = syn.clip_onsets(cid)
    want, E, N = onr.onsets(src, **DEFAULTS)
    assert _same(got, want) and _same(syn.onset_hops(0)[0], E) and _same(syn.onset_hops(0)[1], N)
    S = DEFAULTS["hop"] // 16
    assert len(got) == len(BURSTS), got
    for (frame, strength), true in zip(got, BURSTS):
        assert true - S < frame <= true and strength >= 128, (frame, true)


def test_sine_silence_and_fade_in(syn):
    """a steady sine gives one onset, at frame 0; silence gives none; a one-second linear fade-in gives none"""
    n = 96000
    t = np.arange(n) / SR
    sine = (0.25 * np.sin(2 * np.pi * 220.0 * t)).astype(f32)
    fade = (sine * np.minimum(t, 1.0)).astype(f32)
    for x, expect in ((sine, [0]), (np.zeros(n, f32), []), (fade, [])):
        cid = _upload(syn, x[None, :])
        got = syn.clip_onsets(cid)
        assert _same(got, onr.onsets(x[None, :], **DEFAULTS)[0])
        assert [int(f) for f, _ in got] == expect
        syn.unregister_clip(cid)


def test_max_onsets_returns_the_first_of_equal_bursts(syn):
    """eight identical bursts on hop-aligned positions: equal strengths, max_onsets = 3 keeps the first three"""
    burst = (np.random.default_rng(4).uniform(-0.5, 0.5, 2048) * np.exp(-np.arange(2048) / 300.0)).astype(f32)
    x = np.zeros(8 * 16384, f32)
    for k in range(8):
        x[1024 + k * 16384:1024 + k * 16384 + 2048] = burst
    cid = _upload(syn, x[None, :])
    allof = syn.clip_onsets(cid, hop=256, min_gap=10, max_onsets=64)
    assert [int(f) for f, _ in allof] == [1024 + k * 16384 for k in range(8)] and len({int(s) for _, s in allof}) == 1
    got = syn.clip_onsets(cid, hop=256, min_gap=10, max_onsets=3)
    assert _same(got, allof[:3]) and _same(got, onr.onsets(x[None, :], 0, None, 256, 8, 128, 10, 3)[0])
    syn.unregister_clip(cid)


def test_onsets_follow_the_rerender(syn):
    src = _burst_scene(2, False, length=60000, seed=3)
    cid = _upload(syn, src, 44100.0)
    d = onr.resolve(44100)
    before = syn.clip_onsets(cid)
    assert _same(before, onr.onsets(src, **d)[0]) and len(before) >= 3
    syn.rerender_clip(cid, gain_db=-6.0, pitch=3.0, speed=1.25)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert played.shape[1] == 48000
    now = syn.clip_onsets(cid)
    assert _same(now, onr.onsets(played, **d)[0]) and not _same(now, before)
    assert _same(syn.clip_onsets(cid, 3, 47990, 80, 4, 64, 2, 5), onr.onsets(played, 3, 47990, 80, 4, 64, 2, 5)[0])
    from libzl_amd import ZlHipError
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_onsets(cid, 0, 60000)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert _same(syn.clip_onsets(cid), before) and _same(syn.clip_onsets(cid, 0, 60000), before)
    syn.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    """a small arena and uploads beyond it: the later clips lie in further segments, far from the first one in the address space"""
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [_noise_with_bursts(1 + i % 2, 60000 + 1001 * i, 40 + i) for i in range(8)]      # 0.24 - 0.54 MB each
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        reqs = [(cid, 1, x.shape[1] - 3, 80, 8, 128, 3, 32) for cid, x in zip(ids, srcs)]
        bad = _check_batch(s, reqs, dict(zip(ids, srcs)))
        assert not bad, bad
        assert _same(s.clip_onsets(ids[-1]), onr.onsets(srcs[-1], **DEFAULTS)[0])


def test_a_batch_of_64_equals_64_single_calls(syn):
    from libzl_amd import _abi
    rng = np.random.default_rng(23)
    srcs = [_noise_with_bursts(1 + i % 2, int(rng.integers(1, 20000)), 500 + i) for i in range(16)]
    ids = [_upload(syn, x) for x in srcs]
    reqs = []
    for i in range(64):
        k = i % 16
        length = srcs[k].shape[1]
        first = int(rng.integers(0, length))
        n = int(rng.integers(1, length - first + 1))
        reqs.append((ids[k], first, n, int(rng.choice([64, 80, 256, 1024])), int(rng.choice([1, 8])), int(rng.choice([1, 64, 128])),
                     int(rng.choice([1, 2, 10])), int(rng.choice([1, 3, 128]))))
    arr = (_abi.OnsetRequest * 64)(*[_abi.OnsetRequest(*r) for r in reqs])
    capacity = sum(r[7] for r in reqs)
    packed = np.full((capacity + 3, 2), -1234, np.int32)           # three sentinels behind what the call may write
    counts = np.full(64 + 3, -1234, np.int32)
    assert syn._lib.zlhip_sound_onsets_batch(syn._e, arr, 64, packed.ctypes.data, capacity, counts.ctypes.data) == 0
    assert (counts[64:] == -1234).all() and (counts[:64] >= 0).all() and counts[:64].sum() > 0
    total = int(counts[:64].sum())
    assert (packed[total:] == -1234).all()                         # packed without gaps: nothing behind the last onset is written
    at = 0
    for r, k, n in zip(reqs, [i % 16 for i in range(64)], counts[:64]):
        single = syn.clip_onsets(*r)
        assert _same(packed[at:at + n], single), r                 # request i starts where i - 1 ended
        assert _same(single, onr.onsets(srcs[k], *r[1:])[0]), r
        at += int(n)
    for cid in ids:
        syn.unregister_clip(cid)


def test_one_request_of_65536_hops(syn):
    n = 65536 * 64
    src = np.random.default_rng(65).uniform(-0.5, 0.5, (1, n + 3)).astype(f32)
    cid = _upload(syn, src)
    bad = _check_batch(syn, [(cid, 3, n, 64, 8, 1, 1, 1024)], {cid: src})
    assert not bad, bad
    E, N = syn.onset_hops(0)
    assert E.shape == (65536,) and len(onr.candidates(N, 1, 1)) > 8192
    syn.unregister_clip(cid)


def test_errors_leave_out_and_counts_untouched(syn):
    from libzl_amd import _abi
    lib, e = syn._lib, syn._e
    src = _noise_with_bursts(2, 5000, 8)
    cid = _upload(syn, src)
    big = _upload(syn, np.zeros((1, 65536 * 64 + 64), f32))
    gone = _upload(syn, src)
    syn.unregister_clip(gone)
    out = np.full((70000, 2), -77, np.int32)
    counts = np.full(80, -77, np.int32)
    R = _abi.OnsetRequest
    INV, CAP = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY

    def single(*a, capacity=1024):
        r = R(*a)
        rc = lib.zlhip_sound_onsets(e, C.byref(r), out.ctypes.data, capacity, counts.ctypes.data_as(C.POINTER(C.c_int32)))
        assert (out == -77).all() and (counts == -77).all(), a
        return rc

    def batch(reqs, nreq=None, capacity=out.shape[0]):
        arr = (R * max(1, len(reqs)))(*reqs)
        rc = lib.zlhip_sound_onsets_batch(e, arr, len(reqs) if nreq is None else nreq, out.ctypes.data, capacity, counts.ctypes.data)
        assert (out == -77).all() and (counts == -77).all()
        return rc

    ok = (cid, 0, 5000, 256, 8, 128, 10, 128)
    assert single(255, *ok[1:]) == INV and single(-1, *ok[1:]) == INV and single(256, *ok[1:]) == INV and single(gone, *ok[1:]) == INV
    for field, values in ((3, (48, 63, 65, 72, 4097, 4112, -256)), (4, (-1, 32768)), (5, (-1, 4097)), (6, (-1, 1025)), (7, (-1, 1025))):
        for v in values:
            assert single(*ok[:field], v, *ok[field + 1:]) == INV, (field, v)
    assert single(cid, 0, 0, *ok[3:]) == INV and single(cid, 0, -5, *ok[3:]) == INV and single(cid, -1, 10, *ok[3:]) == INV
    assert single(cid, 1, 5000, *ok[3:]) == INV and single(cid, 5000, 1, *ok[3:]) == INV      # past the end
    assert single(big, 0, 65536 * 64 + 1, 64, 8, 128, 10, 128) == INV                          # 65537 hops
    assert batch([R(big, 0, 65536 * 64, 64, 8, 128, 10, 1)] * 64 + [R(cid, 0, 1, 64, 8, 128, 10, 1)]) == INV      # 4 Mi + 1 hops in one call
    assert batch([R(*ok)], nreq=-1) == INV
    assert single(*ok, capacity=127) == CAP and single(*ok, capacity=-1) == INV
    assert single(cid, 0, 5000, 0, 0, 0, 0, 0, capacity=127) == CAP                            # the resolved max_onsets counts
    assert batch([R(*ok), R(*ok)], capacity=255) == CAP
    assert batch([R(*ok), R(gone, *ok[1:])]) == INV                                            # one bad request fails the whole call
    assert b"sound_onsets" in lib.zlhip_last_error(e)
    assert lib.zlhip_sound_onsets_batch(e, None, 1, out.ctypes.data, 1024, counts.ctypes.data) == INV
    n = C.c_int32(-77)
    assert lib.zlhip_debug_onset_hops(e, 99, None, None, 0, C.byref(n)) == INV and n.value == -77
    # the limits themselves are fine
    assert batch([], nreq=0) == 0
    assert lib.zlhip_sound_onsets_batch(e, (R * 2)(R(*ok), R(*ok)), 2, out.ctypes.data, 256, counts.ctypes.data) == 0
    want = onr.onsets(src, *ok[1:])[0]
    assert counts[0] == counts[1] == len(want) and (counts[2:] == -77).all()
    assert _same(out[:len(want)], want) and _same(out[len(want):2 * len(want)], want) and (out[2 * len(want):] == -77).all()
    E = np.zeros(4, np.uint64)
    assert lib.zlhip_debug_onset_hops(e, 1, E.ctypes.data, None, 4, C.byref(n)) == CAP and n.value == 20 and not E.any()
    for c in (cid, big):
        syn.unregister_clip(c)


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _noise_with_bursts(2, 5000, 2))
        total0, _ = s.memory_bytes()
        s.clip_overview(cid, 10)
        total1, _ = s.memory_bytes()
        s.clip_onsets(cid)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_onsets(cid); s.clip_onsets(cid, 3, 4000, 64, 1, 1, 1, 128)        # fit the first call's buffers
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
    """After one warm-up call (it allocates the call's buffers) onset calls between real-time cycles leave the resident kernel where it
    is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the onsets right."""
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
        params = [(64, 8, 32, 2, 128), (80, 4, 1, 1, 16), (256, 8, 128, 10, 128)]
        syn.clip_onsets_batch([(i, 0, None, 64, 8, 1, 1, 128) for i in range(len(planar))])      # the warm-up call: the largest of them
        expect = {}
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
            # between the cycles: the onsets of clips that play (the voice reports are host memory: no device call), a single call and
            # a batch in turn
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            for cid in playing[:2]:
                p = params[k % 3]
                got = syn.clip_onsets(cid, 0, None, *p) if k % 2 else syn.clip_onsets_batch([(cid, 0, None, *p), (cid, 1, 3, 64, 1, 1, 1, 1)])[0]
                if (cid, p) not in expect:
                    expect[(cid, p)] = onr.onsets(planar[cid], 0, None, *p)[0]
                assert _same(got, expect[(cid, p)]), (k, cid)
                checked += 1
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        assert checked >= sc.nblocks
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


def test_group_onsets_equal_the_single_engine(syn, burst_clips):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        for key in ((1, True), (2, False)):
            cid, src = burst_clips[key]
            gid = _upload(g, src)
            for args in ((), (3, 150000, 80, 4, 64, 2, 3)):
                a = g.clip_onsets(gid, *args)
                assert _same(a, syn.clip_onsets(cid, *args)) and len(a) >= 3
            assert _same(a, onr.onsets(src, 3, 150000, 80, 4, 64, 2, 3)[0])
        a, b = g.clip_onsets_batch([(0,), (1, 5, 1000)])
        assert len(a) == len(BURSTS) and len(b) == 1
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_onsets_batch([(0, 0, None, 65)])


def test_libzl_clip_slice_at_transients(built, tmp_path):
    from libzl_amd import _abi, libzl
    from libzl_amd.engine import synthetic_clocks
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        src = _burst_scene(2, True)
        path = str(tmp_path / "b.wav").encode()
        assert zl.libzl_wav_write(path, src[0].ctypes.data, src[1].ctypes.data, src.shape[1], SR, 32) == 0
        c = zl.ClipAudioSource_new(path, False)
        assert c

        def table():
            p = _abi.ClipParams()
            assert zl.libzl_hotpath_clip_params(c, C.byref(p)) == 0
            return [p.slice_positions[i] for i in range(p.num_slice_positions)]

        even = table()
        assert len(even) == 16                                     # the constructor's setSlices(16)
        assert zl.libzl_hotpath_clip_slice_at_transients(c, 0) < 0 and zl.libzl_hotpath_clip_slice_at_transients(None, 8) < 0
        assert table() == even                                     # a failing call leaves the table as it was
        want = onr.onsets(src, **DEFAULTS)[0]
        assert [int(f) for f, _ in want][0] == 0 and len(want) == len(BURSTS)
        n = zl.libzl_hotpath_clip_slice_at_transients(c, 64)
        assert n == len(BURSTS)
        got = table()
        # slice 0 is 0.0 (the onset at frame 0 is slice 0 itself), then the onsets as fractions of the region (the whole clip)
        assert got == [0.0] + [float(f) / float(src.shape[1]) for f, _ in want[1:]] and len(got) == n
        # `slices` is the table's length: setSlices(n) finds nothing to do, setSlices(n - 1) drops the last entry
        zl.ClipAudioSource_setSlices(c, n)
        assert table() == got
        # fewer slices than transients: the strongest stay
        assert zl.libzl_hotpath_clip_slice_at_transients(c, 3) == 3
        few = onr.onsets(src, **dict(DEFAULTS, max_onsets=3))[0]
        assert table() == [0.0] + [float(f) / float(src.shape[1]) for f, _ in few if f > 0][:2]
        assert zl.libzl_hotpath_clip_slice_at_transients(c, 64) == n and table() == got
        # a note mapped to slice 2 (sliceForMidiNote: base note 60, so note 62) plays from the third burst
        slice_ = ((n - 60 % n) + 62) % n
        assert slice_ == 2
        # (an engine of the test's own plays the clip with the parameters the libzl layer hands to its engine)
        from libzl_amd import SamplerSynth
        p = _abi.ClipParams()
        assert zl.libzl_hotpath_clip_params(c, C.byref(p)) == 0
        N = 256
        with SamplerSynth(num_buses=12, voices_per_bus=2, max_sounds=4, playback_sample_rate=SR, max_frames=N, sound_arena_bytes=4 << 20) as s:
            cid = _upload(s, src)
            s.set_clip_params(cid, p)
            s.handle_clip_command(engine_cmd(clip=cid, midiChannel=-2, midiNote=60, startPlayback=1, changeSlice=1, slice=slice_,
                                             changeVolume=1, volume=1.0, looping=0), 0)
            L, R = s.process(N, synthetic_clocks(1, N, SR, start_block=0)[0])
        heard = L.sum(axis=0).astype(np.float64)
        assert np.abs(heard).max() > 0.01
        # at pitch ratio 1 what is heard on the left is a fixed mix of the source's two channels from the slice's first frame on
        # (frame f lands in out[f + 1]): the residual of the best such mix is rounding at the right frame and the signal itself elsewhere
        def residual(at):
            A = src[:, at:at + 199].T.astype(np.float64)
            return float(np.linalg.norm(A @ np.linalg.lstsq(A, heard[1:200], rcond=None)[0] - heard[1:200]) / np.linalg.norm(heard[1:200]))
        start = int(want[2][0])
        best = min(range(start - 2, start + 3), key=residual)
        assert residual(best) < 1e-4 and residual(int(want[1][0])) > 0.5 and residual(int(want[3][0])) > 0.5, residual(best)
        assert BURSTS[2] - 16 - 2 <= best <= BURSTS[2] + 2
        zl.ClipAudioSource_destroy(c)
    finally:
        zl.shutdownJuce()
