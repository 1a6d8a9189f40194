"""The seven clip analyses -- overviews, transients, tempo, pitch, loudness, loop points, key -- through ONE engine and against each other: they share one
call scaffold in libzl_amd/csrc/zl_clip_calls.cpp (check, reserve, stage timer), which can go wrong only where a neighbour is present:
a mixed-up buffer index, a timer shared by mistake, a read-back table overwritten by another service.  Expected values are the
restatements' (tests/overview_ref.py, onset_ref.py, tempo_ref.py, pitch_ref.py, loudness_ref.py, loop_ref.py, key_ref.py), compared as the
per-service tests compare them: every integer and every debug array bit for bit, bpm, hz and confidence with ==, note and cents within
1e-9, lufs within 1e-9, the loop's three dB fields within 1e-9, the key's two confidences with == (tests/test_pitch_gpu.py,
tests/test_loudness_gpu.py, tests/test_loop_gpu.py, tests/test_key_gpu.py).

And, at the end, the five calls that replace clip data -- PCM upload, re-render, rate conversion, loop crossfade, warp -- through the one
path none of their own tests reaches: a call that fails after the arena has grown by a segment."""
import ctypes as C
import math

import numpy as np
import pytest

import key_ref as kr
import loop_checks as lc
import loudness_ref as lr
import onset_ref as onr
import overview_ref as ov
import pitch_ref as pr
import tempo_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 48000.0
# the length at which the per-service tests put a default request to every analysis (test_*_gpu.py::test_an_engine_that_never_asks_allocates_nothing)
LENGTH = 50000
COLUMNS = 100
TEMPO_INTS = ("lag_coarse", "lag_fine", "doublings", "shift", "hops", "acf_lo", "acf_mid", "acf_hi", "acf_zero", "sum")
SERVICES = ("overview", "onsets", "tempo", "pitch", "loudness", "loop", "key")
# the loop finder's default request: 10 ms either way at 48 kHz, 961 x 961 candidate pairs -- one request keeps its cost matrix, a batch of 70 does not
LOOP = dict(start_frame=12000, stop_frame=36011)
KEY_INTS = kr.RESULT_INTS


def _clip(ch, seed):
    """a harmonic tone under a train of decaying pulses, on a little noise: onsets, a flux with a period, a pitch and a loudness"""
    rng = np.random.default_rng(seed)
    t = np.arange(LENGTH)
    env = 0.05 + np.exp(-(t % 9600) / 1500.0)
    y = np.stack([np.sin(2 * np.pi * t / (218.4 + 30 * seed) + 0.3 * c) + 0.4 * np.sin(4 * np.pi * t / (218.4 + 30 * seed) + c) for c in range(ch)])
    return (0.3 * env * (y / 1.4 + 0.01 * rng.standard_normal((ch, LENGTH)))).astype(f32)


def _coeffs(rate):
    from libzl_amd import _abi
    c = (C.c_double * 10)()
    assert _abi.load().zlhip_loudness_design(rate, c) == 0
    return list(c)


@pytest.fixture(scope="module")
def wants(built):
    """per clip (mono, stereo): the planar source and every analysis' default request restated, computed once"""
    from libzl_amd import _abi
    coeffs = _coeffs(SR)
    table = []
    for ch, seed in ((1, 0), (2, 1)):
        src = _clip(ch, seed)
        table.append(dict(src=src, overview=ov.overview(src, COLUMNS), onsets=onr.onsets(src, **onr.resolve(SR)), tempo=tr.tempo(src, SR),
                          pitch=pr.pitch(src, SR, want_d=True), loudness=lr.measure(src, SR, coeffs=coeffs), loop=lc.want(src, SR, LOOP),
                          key=kr.key(src, SR, *kr.library_table(_abi.load(), SR))))
    return table


def _engine():
    from libzl_amd import SamplerSynth
    return SamplerSynth(num_buses=1, voices_per_bus=2, max_sounds=8, sound_arena_bytes=8 << 20)


def _upload(syn, src):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, SR)


def _same_arrays(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def _tempo_matches(got, want):
    return all(got[k] == want[k] for k in TEMPO_INTS) and f32(got["bpm"]) == want["bpm"] and f32(got["confidence"]) == want["confidence"]


def _pitch_matches(got, want):
    return (all(int(got[k]) == int(want[k]) for k in pr.RESULT_INTS) and f32(got["hz"]) == want["hz"] and f32(got["confidence"]) == want["confidence"]
            and abs(float(got["note"]) - float(want["note"])) <= 1e-9 and abs(float(got["cents"]) - float(want["cents"])) <= 1e-9)


def _onset_hops_match(syn, i, want):
    E, N = syn.onset_hops(i)
    return _same_arrays(E, want[1]) and _same_arrays(N, want[2])


def _tempo_acf_matches(syn, i, want):
    W, first_lag, A = syn.tempo_acf(i)
    return (W.dtype == np.uint16 and np.array_equal(W, want[1]) and A.dtype == np.uint64 and [int(v) for v in A] == want[3]
            and (len(want[3]) == 0 or first_lag == want[2]))


def _pitch_frames_match(syn, i, want):
    frames = syn.pitch_frames(i)
    return frames == want[1] and len(frames) == len(want[2]) and all([int(v) for v in syn.pitch_diff(i, k)] == want[2][k] for k in range(len(frames)))


def _loudness_subs_match(syn, i, want):
    sums, peaks = syn.loudness_subs(i)
    return (sums.shape == want[1].shape and np.array_equal(sums.view(np.uint64), want[1].view(np.uint64))
            and peaks.shape == want[2].shape and np.array_equal(peaks.view(np.uint32), want[2].view(np.uint32)))


def _key_matches(got, want):
    return (all(int(got[k]) == int(want[k]) for k in KEY_INTS) and tuple(got["chroma"]) == want["chroma"] and got["confidence"] == want["confidence"]
            and got["second_confidence"] == want["second_confidence"])


def _loop_costs_match(syn, i, want, kept):
    """a single request keeps its cost matrix; the batch of 70 has more than 2^20 candidate pairs and keeps none (ZLHIP_ERR_STATE)"""
    from libzl_amd import ZlHipError
    if kept:
        c = syn.loop_costs(i)
        return c.dtype == np.uint32 and c.shape == want[2].shape == (961, 961) and np.array_equal(c.astype(np.int64), want[2])
    with pytest.raises(ZlHipError, match=r"\(-5\)"):
        syn.loop_costs(i)
    return True


def _key_read_backs_match(syn, i, want):
    totals, frames = syn.key_bins(i), syn.key_frames(i)
    ok = totals.dtype == np.uint64 and [int(v) for v in totals] == want[1] and frames == len(want[2]) and frames >= 2
    for k in (0, frames - 1):
        re, im = syn.key_frame(i, k)
        ok = ok and re.dtype == np.int64 and [int(v) for v in re] == want[2][k]["re"] and [int(v) for v in im] == want[2][k]["im"]
    return ok


def _run(syn, service, ids, which, wants):
    """one call of `service` with the default request of clips which[0], which[1], ...; every result and, for the requests in `probe`,
    every read-back against the restatement.  Returns the results as comparable bytes / values (round 3 against round 1)."""
    clips = [ids[w] for w in which]
    probe = sorted({0, 1, len(which) - 2, len(which) - 1} & set(range(len(which))))
    if service == "overview":
        outs = syn.clip_overviews([(c, COLUMNS) for c in clips])
        assert all(ov.same_bits(o, wants[w]["overview"]) for o, w in zip(outs, which)), service
        return [o.tobytes() for o in outs]
    if service == "onsets":
        outs = syn.clip_onsets_batch([(c,) for c in clips])
        assert all(_same_arrays(o, wants[w]["onsets"][0]) for o, w in zip(outs, which)), service
        assert all(_onset_hops_match(syn, i, wants[which[i]]["onsets"]) for i in probe), service
        return [o.tobytes() for o in outs]
    if service == "tempo":
        outs = syn.clip_tempo_batch([(c,) for c in clips])
        assert all(_tempo_matches(o, wants[w]["tempo"][0]) for o, w in zip(outs, which)), service
        assert all(_tempo_acf_matches(syn, i, wants[which[i]]["tempo"]) for i in probe), service
        return outs
    if service == "pitch":
        outs = syn.clip_pitch_batch([(c,) for c in clips])
        assert all(_pitch_matches(o, wants[w]["pitch"][0]) for o, w in zip(outs, which)), service
        assert all(_pitch_frames_match(syn, i, wants[which[i]]["pitch"]) for i in probe), service
        return outs
    if service == "loop":
        outs = syn.clip_loop_batch([dict(LOOP, clip=c) for c in clips])
        assert all(lc.same(o, wants[w]["loop"][0]) for o, w in zip(outs, which)), service
        assert all(syn.loop_items(i) == wants[which[i]]["loop"][1] for i in probe), service
        assert all(_loop_costs_match(syn, i, wants[which[i]]["loop"], len(which) == 1) for i in probe), service
        return outs
    if service == "key":
        outs = syn.clip_key_batch([dict(clip=c) for c in clips])
        assert all(_key_matches(o, wants[w]["key"][0]) for o, w in zip(outs, which)), service
        assert all(_key_read_backs_match(syn, i, wants[which[i]]["key"]) for i in probe), service
        return outs
    outs = syn.clip_loudness_batch([(c,) for c in clips])
    assert all(lr.same(o, wants[w]["loudness"][0]) for o, w in zip(outs, which)), service
    assert all(_loudness_subs_match(syn, i, wants[which[i]]["loudness"]) for i in probe), service
    return outs


def _timings(syn):
    return ((syn.overview_timings(),) + tuple(syn.onset_timings()) + tuple(syn.tempo_timings()) + tuple(syn.pitch_timings()) + (syn.loudness_timings(),)
            + tuple(syn.loop_timings()) + tuple(syn.key_timings()))


def test_every_call_on_one_engine_growing(wants):
    """Single requests with profiling off, then batches of 70 in reverse order with profiling on (70 is past the request buffers' floor
    of 64 and the mapped results' first capacity of 64: every service's buffers are replaced once, next to its neighbours'), then the
    single requests again: every result equals the restatement, round 3 equals round 1 bit for bit, and the stage times are those of
    round 2 -- finite, not negative, and not touched by the unprofiled round behind it."""
    syn = _engine()
    try:
        ids = [_upload(syn, w["src"]) for w in wants]
        syn.set_profiling(False)
        first = {}
        for service in SERVICES:
            first[service] = [_run(syn, service, ids, [k], wants) for k in (0, 1)]
        total1 = syn.memory_bytes()[0]
        syn.set_profiling(True)
        for service in reversed(SERVICES):
            _run(syn, service, ids, [i % 2 for i in range(70)], wants)
        assert syn.memory_bytes()[0] > total1                      # the buffers grew
        times = _timings(syn)
        print("stage times of the batches of 70 (ms):", times)
        assert len(times) == 14 and all(math.isfinite(t) and t >= 0.0 for t in times), times
        syn.set_profiling(False)
        for service in SERVICES:
            assert [_run(syn, service, ids, [k], wants) for k in (0, 1)] == first[service], service
        assert _timings(syn) == times
    finally:
        syn.close()


def test_read_backs_belong_to_their_own_service(wants):
    """An onsets call, then a tempo call on the other clip -- it runs the transients' energy kernel, on its own buffers -- then a pitch
    call: every service's read-backs still return its own last call."""
    syn = _engine()
    try:
        ids = [_upload(syn, w["src"]) for w in wants]
        got_on = syn.clip_onsets(ids[0])
        got_tp = syn.clip_tempo(ids[1])
        got_pt = syn.clip_pitch(ids[0])
        assert _same_arrays(got_on, wants[0]["onsets"][0]) and _tempo_matches(got_tp, wants[1]["tempo"][0]) and _pitch_matches(got_pt, wants[0]["pitch"][0])
        assert _onset_hops_match(syn, 0, wants[0]["onsets"])
        assert _tempo_acf_matches(syn, 0, wants[1]["tempo"])
        assert _pitch_frames_match(syn, 0, wants[0]["pitch"])
        # (the two clips' energies differ, so the tempo call's E in the transients' buffer would show)
        assert not np.array_equal(wants[0]["onsets"][1], wants[1]["onsets"][1])
    finally:
        syn.close()


# ---- the five calls that replace clip data: a batch that fails after the arena grew ---------------------------------------------
# Their all-or-none tests elsewhere pin sound_arena_max_bytes to sound_arena_bytes, so nothing there gives back a segment the failed
# call itself added.  Here the first arena has 1 MiB (262144 floats).  A further segment is never smaller than the first arena, so
# a cap of 2 MiB allows exactly one.  Request 0's new extent is larger than what the first arena has free: it gets the segment.
# Request 1's is larger than what either has free then, and a second segment would pass the cap: ZLHIP_ERR_CAPACITY.
ARENA = 1 << 20


def _noise(frames, seed):
    return (0.25 * np.random.default_rng(seed).standard_normal(frames)).astype(f32)


def _grown_rerender(s):
    """120008 floats each, 22128 free: gain only, request 0 takes 120008 of the segment; at half speed request 1 wants 240008"""
    ids = [s.register_clip(_noise(120000, k), None, SR) for k in (0, 1)]
    return ids, lambda which: s.rerender_clips([ids[k] for k in which], gain_db=-6.0, speed=[(1.0, 0.5)[k] for k in which])


def _grown_convert(s):
    """60008 and 120008 floats at 24 kHz, 82128 free: at 48 kHz request 0 takes 120008 of the segment, request 1 wants 240008.  The
    filter table of the ratio is made before the extents: the failed call gives that back too."""
    ids = [s.register_clip(_noise(n, k), None, SR / 2) for k, n in enumerate((60000, 120000))]
    return ids, lambda which: s.convert_clips([ids[k] for k in which])


def _grown_warp(s):
    """100008 floats each, 62128 free: request 0 is stretched to 125008, request 1 to 200008"""
    ids = [s.register_clip(_noise(100000, k), None, SR) for k in (0, 1)]
    return ids, lambda which: s.clip_warp_batch([(ids[k], [(0, 0), (100000, (125000, 200000)[k])]) for k in which])


def _grown_pcm(s):
    """a clip of 100008 floats, 162136 free: request 0 wants 200008, request 1 180008; a failed call takes no slot either"""
    ids = [s.register_clip(_noise(100000, 0), None, SR)]
    pcm = [(8192.0 * _noise(n, k)).astype(np.int16) for k, n in ((1, 200000), (2, 180000))]

    def call(which):
        assert s.register_clips_pcm([(pcm[k], None, 1, SR) for k in which]) == list(range(1, 1 + len(which)))
    return ids, call


def _grown_xfade(s):
    """A crossfaded extent is as large as its original, and two originals that share the first arena fit one segment: with a cap of
    2 MiB no crossfade call fails after the arena grew.  So the cap is 3 MiB and the second clip's upload adds the first segment
    (200008 floats each, 62136 free in either allocation).  Request 0 gets the second segment, request 1 would need a third."""
    ids = [s.register_clip(_noise(200000, k), None, SR) for k in (0, 1)]
    assert s.memory_bytes()[1] == 2 * ARENA
    return ids, lambda which: s.clip_loop_crossfade_batch([(ids[k], 50000, 150000, 1000) for k in which])


GROWN = {"rerender": (2 * ARENA, _grown_rerender), "convert_rate": (2 * ARENA, _grown_convert), "loop_crossfade": (3 * ARENA, _grown_xfade),
         "warp": (2 * ARENA, _grown_warp), "upload_pcm": (2 * ARENA, _grown_pcm)}


@pytest.mark.parametrize("service", sorted(GROWN))
def test_a_call_that_fails_after_the_arena_grew_gives_the_segment_back(built, service):
    """The call fails with ZLHIP_ERR_CAPACITY, zlhip_memory_bytes is what it was before the call (the segment went back to the device),
    every clip's extent has the bits it had, and the same call without the request that did not fit succeeds and keeps the segment."""
    from libzl_amd import SamplerSynth, ZlHipError
    cap, scene = GROWN[service]
    with SamplerSynth(num_buses=1, voices_per_bus=2, max_sounds=8, sound_arena_bytes=ARENA, sound_arena_max_bytes=cap) as s:
        ids, call = scene(s)
        exts, mem = [s.clip_extent(i) for i in ids], s.memory_bytes()
        with pytest.raises(ZlHipError, match=r"\(-4\)"):
            call((0, 1))
        assert s.memory_bytes() == mem
        assert all(np.array_equal(s.clip_extent(i).view(np.uint32), x.view(np.uint32)) for i, x in zip(ids, exts))
        call((0,))
        assert s.memory_bytes()[1] == mem[1] + ARENA and s.memory_bytes()[0] > mem[0] + ARENA
