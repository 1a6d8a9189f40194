"""Pitch detection, CPU tier: what the definition does to sound, with the numpy / Python-integer restatement (tests/pitch_ref.py)
alone; the host build of libzl_amd/csrc/zl_pitch.h (tests/cpu_harness/pitch_host.cpp walks a call the way the kernels do, work item by
work item, with the header's own arithmetic) against the restatement on every integer of d, of every frame record and of the result,
with == on hz and confidence; the defaults and the limits; the struct layouts; the new kernels' resources; the walk under the
sanitizers (tests/cpp/pitch_check.cpp); the edge cases that reach the kernels as clips (tests/pitch_cases.py): every predicate, and the
list through the walk.  tests/test_pitch_gpu.py and tests/test_pitch_edges_gpu.py hold the kernels themselves to the restatement on
the GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_pitch_harness())
        l.zlpt_resolve.restype = C.c_int32
        l.zlpt_resolve.argtypes = [C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32)]
        l.zlpt_sizes.argtypes = [C.c_void_p]
        l.zlpt_call.restype = C.c_int64
        l.zlpt_call.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        l.zlpt_pick_vote.restype = C.c_int32
        l.zlpt_pick_vote.argtypes = [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_double, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


# ---- what the definition does to sound (the restatement alone) ----------------------------------------------------------------------
NOTES = tuple(range(33, 91, 3))


@pytest.mark.parametrize("rate", [48000.0, 44100.0])
@pytest.mark.parametrize("signal", pr.SIGNALS, ids=[s.__name__ for s in pr.SIGNALS])
def test_signals_give_their_note(signal, rate):
    """640 cases over the eight parameter sets: 1 s clips with 1 % noise at the levels 0.5 and 0.005, MIDI 33, 36, ..., 90 on the note and
    30 cents sharp, max_frames = 8.  Measured: the worst error is 2.98 cents (saw, note 90.3, 44.1 kHz); sine 0.69, pluck 1.11,
    missing fundamental 1.16; rint(note) is right in every case; the confidence is 1.0 at level 0.5.  The lag
    alone is up to 68 cents off at t = 25, so the bound shows the parabola is doing its work."""
    worst = 0.0
    for level in (0.5, 0.005):
        for n0 in NOTES:
            for note in (float(n0), n0 + 0.3):
                res = pr.pitch(pr.clip(signal, rate, note, level), rate, max_frames=8)[0]
                assert res["lag"] > 0, (note, level, res)
                err = 1200.0 * math.log2(float(res["hz"]) / pr.hz_of(note))
                worst = max(worst, abs(err))
                print(signal.__name__, rate, level, note, float(res["hz"]), round(err, 3), res["root_note"], float(res["confidence"]))
                assert abs(err) <= 5.0, (note, level, err, res)
                assert res["root_note"] == int(np.rint(note)), (note, level, res)
                assert abs(float(res["note"]) - note) <= 0.05 and abs(float(res["cents"]) - 100.0 * (note - res["root_note"])) <= 5.0
                if level == 0.5:
                    assert res["confidence"] >= 0.9, (note, level, res)
    print("worst", signal.__name__, rate, worst)


def test_noise_silence_dc_and_a_short_clip_give_no_pitch():
    rng = np.random.default_rng(1)
    L = 1792 + 872 + 1
    for x, frames in ((rng.uniform(-0.5, 0.5, (1, 48000)).astype(np.float32), 8), (np.zeros((1, 48000), np.float32), 8),
                      (np.full((2, 48000), 0.3, np.float32), 8), (pr.clip(pr.saw, 48000.0, 45, 0.5)[:, :L - 1], 0)):
        res, recs = pr.pitch(x, 48000.0, max_frames=8)
        assert res["frames"] == frames == len(recs)
        assert all(int(res[k]) == 0 for k in pr.RESULT_INTS if k != "frames") and res["hz"] == 0.0 and res["confidence"] == 0.0, res
    assert [r["flag"] for r in pr.pitch(np.zeros((1, 48000), np.float32), 48000.0, max_frames=8)[1]] == [pr.SILENT] * 8
    assert [r["flag"] for r in pr.pitch(np.full((2, 48000), 0.3, np.float32), 48000.0, max_frames=8)[1]] == [pr.UNVOICED] * 8
    # one frame more and the saw is there
    assert pr.pitch(pr.clip(pr.saw, 48000.0, 45, 0.5)[:, :L], 48000.0, max_frames=8)[0]["root_note"] == 45


def test_the_two_forms_of_the_difference_function_agree():
    rng = np.random.default_rng(2)
    x = rng.integers(-4096, 4096, 256 + 130).astype(np.int64)
    assert pr.diff(x, 256, 129) == pr.diff_direct(x, 256, 129)
    x = np.full(4096 + 2048, -4096, np.int64); x[::2] = 4095
    assert pr.diff(x, 4096, 2047) == pr.diff_direct(x, 4096, 2047) and max(pr.diff(x, 4096, 2047)) == 4096 * 8191 ** 2 < 2 ** 38


# ---- the harness against the restatement --------------------------------------------------------------------------------------------
def arena(x):
    """float32 [channels][frames] -> the arena's layout, padded with zeros to a whole 16-byte group"""
    flat = np.ascontiguousarray(np.asarray(x, np.float32).T).reshape(-1)
    return np.concatenate([flat, np.zeros(-len(flat) % 4, np.float32)])


def same_result(got, want, what):
    assert {k: int(getattr(got, k)) for k in pr.RESULT_INTS} == {k: int(want[k]) for k in pr.RESULT_INTS}, (what, want)
    assert np.float32(got.hz) == want["hz"] and np.float32(got.confidence) == want["confidence"], (what, got.hz, want)
    assert abs(float(got.note) - float(want["note"])) <= 1e-9 and abs(float(got.cents) - float(want["cents"])) <= 1e-9, (what, got.note, got.cents, want)


def call(requests, count_limit=48 << 20):
    """requests: (x float32 [channels][frames], rate, dict of zlhip_pitch_request's fields but id).  Runs the harness walk over the whole
    call and holds d, every frame record and every result to the restatement; returns (result, frame records, geometry) per request"""
    n = len(requests)
    reqs = (_abi.PitchRequest * n)()
    datas, refs = [], []
    for i, (x, rate, f) in enumerate(requests):
        x = np.atleast_2d(np.asarray(x, np.float32))
        first = f.get("first_frame", 0)
        nf = f.get("num_frames", x.shape[1] - first)
        reqs[i] = _abi.PitchRequest(0, first, nf, f.get("window", 0), f.get("max_frames", 0), f.get("f_min", 0.0), f.get("f_max", 0.0), f.get("threshold", 0), f.get("gate", 0))
        datas.append(arena(x))
        refs.append(pr.pitch(x, rate, first, nf, f.get("window", 0), f.get("max_frames", 0), f.get("f_min", 0.0), f.get("f_max", 0.0), f.get("threshold", 0),
                             f.get("gate", 0), want_d=True))
    data = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    length = np.array([np.atleast_2d(r[0]).shape[1] for r in requests], np.int32)
    channels = np.array([np.atleast_2d(r[0]).shape[0] for r in requests], np.int32)
    rate = np.array([r[1] for r in requests], np.float64)
    words = sum(len(ds) * len(ds[0]) for _, _, ds in refs if ds)
    nframes = sum(len(recs) for _, recs, _ in refs)
    D = np.full(words + 1, 0xDEADBEEF, np.uint64)
    frames = (_abi.PitchFrame * (nframes + 1))()
    C.memset(frames, 0x5A, C.sizeof(frames))
    geom = np.zeros((n, 8), np.int32)
    dbase = np.zeros(n, np.int64)
    out = (_abi.Pitch * n)()
    sizes = np.zeros(3, np.int32)
    lib().zlpt_sizes(sizes.ctypes.data)
    assert list(sizes) == [C.sizeof(_abi.Pitch), C.sizeof(_abi.PitchFrame), 64] and C.sizeof(_abi.Pitch) == 80 and C.sizeof(_abi.PitchFrame) == 48
    touched = [np.zeros(len(d), np.uint8) for d in datas]
    tptr = (C.c_void_p * n)(*[t.ctypes.data for t in touched])
    cbufs = []
    for (x, r, f), (_, recs, ds) in zip(requests, refs):
        size = len(ds) * len(ds[0]) if ds else 0
        cbufs.append(None)
        if ds:
            W = pr.resolve(r, 10 ** 6, f.get("window", 0), f.get("max_frames", 0), f.get("f_min", 0.0), f.get("f_max", 0.0), f.get("threshold", 0), f.get("gate", 0))["window"]
            if size * W <= count_limit:
                cbufs[-1] = np.zeros((len(ds), len(ds[0]), W), np.uint8)
    cptr = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in cbufs])
    walk = np.zeros(4, np.int64)
    used = lib().zlpt_call(n, C.addressof(reqs), C.addressof(data), length.ctypes.data, channels.ctypes.data, rate.ctypes.data, D.ctypes.data, words,
                           C.addressof(frames), nframes, geom.ctypes.data, dbase.ctypes.data, C.addressof(out), C.addressof(tptr), C.addressof(cptr), walk.ctypes.data)
    assert used == words and int(D[words]) == 0xDEADBEEF and bytes(frames[nframes]) == b"\x5a" * 48
    terms, results, fb = 0, [], 0
    for i, (res, recs, ds) in enumerate(refs):
        tmin, tmax, W, K, hop, items, frame_base, tiles = (int(v) for v in geom[i])
        q = pr.resolve(float(rate[i]), 10 ** 6, *(getattr(reqs[i], k) for k in ("window", "max_frames", "f_min", "f_max", "threshold", "gate")))
        assert (tmin, tmax) == pr.lags(float(rate[i]), q["f_min"], q["f_max"]) and W == q["window"]
        assert (K, hop) == pr.frames_of(reqs[i].num_frames, W, tmax, q["max_frames"]) and K == len(recs) and frame_base == fb
        assert tiles == -(-(tmax + 1) // 256) and items == K * tiles
        for k in range(K):
            got = [int(v) for v in D[dbase[i] + k * (tmax + 1):dbase[i] + (k + 1) * (tmax + 1)]]
            assert got == ds[k], (i, k, "d")
            rec = frames[fb + k]
            assert {f: int(getattr(rec, f)) for f in pr.FRAME_INTS} == recs[k], (i, k, recs[k])
        same_result(out[i], res, i)
        # every float of the frames' spans is used exactly once per frame that holds it, and nothing else of the sound is
        want = np.zeros(len(datas[i]), np.uint8)
        ch = int(channels[i])
        for k in range(K):
            s = reqs[i].first_frame + k * hop
            want[s * ch:(s + W + tmax + 1) * ch] += 1
        assert np.array_equal(touched[i], want), (i, "a float of a span is not read, or one outside is")
        if cbufs[i] is not None:
            assert np.all(cbufs[i] == 1), (i, "a term enters twice or not at all")
        terms += K * (tmax + 1) * W
        results.append((res, recs, dict(tmin=tmin, tmax=tmax, window=W, frames=K, hop=hop, items=items, tiles=tiles)))
        fb += K
    assert [int(v) for v in walk] == [terms, 0, 0, 0], walk
    return results


def tone(rate, frames, period, level=0.4, channels=1, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    y = level * (np.sin(2 * np.pi * t / period) + 0.5 * np.sin(4 * np.pi * t / period + 1.0)) / 1.5 + 0.001 * rng.standard_normal(frames)
    return np.repeat(y[None, :], channels, 0).astype(np.float32)


def fmin_for(rate, tmax):
    """an f_min whose floor(rate / f_min) is tmax"""
    f = float(np.float32(rate / (tmax + 0.5)))
    assert pr.lags(rate, f, rate / 4)[1] == tmax
    return f


def test_mono_and_stereo_odd_first_frames_and_the_frame_counts():
    rate = 48000.0
    base = dict(window=256, f_min=fmin_for(rate, 239), f_max=2000.0)
    L = 256 + 240
    reqs = []
    for ch in (1, 2):
        for first in (0, 1, 3, 5):
            reqs.append((tone(rate, first + L + 300, 100.3, channels=ch, seed=first), rate, dict(base, first_frame=first, num_frames=L + 299, max_frames=4)))
    # K of 1, 2, max_frames and max_frames + 1 (the stretched hop)
    for want, mf in ((1, 4), (2, 4), (4, 4), (5, 4), (9, 1)):
        reqs.append((tone(rate, 7 + L + want * 256, 57.7, channels=2), rate, dict(base, first_frame=2, num_frames=L + (want - 1) * 256 + 77, max_frames=mf)))
    out = call(reqs)
    assert [g["frames"] for _, _, g in out] == [2] * 8 + [1, 2, 4, 4, 1]
    assert out[11][2]["hop"] == (4 * 256 + 77) // 3 > 256 and out[10][2]["hop"] == 256
    assert all(res["lag"] == 100 and res["confidence"] == 1.0 for res, _, _ in out[:8]) and all(res["lag"] == 58 for res, _, _ in out[8:])


def test_lag_tile_edges():
    rate = 48000.0
    out = call([(tone(rate, 1500, 97.0, seed=n), rate, dict(window=320, f_min=fmin_for(rate, n - 1), f_max=2000.0, max_frames=2)) for n in (255, 256, 257)])
    assert [g["tiles"] for _, _, g in out] == [1, 1, 2] and [g["tmax"] for _, _, g in out] == [254, 255, 256]
    assert all(res["lag"] == 97 for res, _, _ in out)


def test_shift_of_zero_and_of_stereo_full_scale():
    rate = 48000.0
    f = dict(window=256, f_min=fmin_for(rate, 200), f_max=2000.0, max_frames=2)
    quiet = np.full((2, 1000), 0.5, np.float32); quiet[:, ::80] = -0.5          # |m| = 2 * 2048 = 4096: thirteen bits, the first shift
    loud = tone(rate, 1000, 80.0, level=9.0, channels=2)                       # clipped to +-32767 in both channels: |m| = 65534, sixteen bits
    mono = tone(rate, 1000, 80.0, level=0.9)
    edge = np.full((1, 1000), 4095.0 / 4096.0, np.float32); edge[0, ::80] = -4095.0 / 4096.0       # |m| = 4095: twelve bits, no shift
    out = call([(quiet, rate, f), (loud, rate, f), (mono, rate, f), (edge, rate, f)])
    assert [res["shift"] for res, _, _ in out] == [1, 4, 0, 0]                 # 4 is the largest there is: bitlength(2 * 32767) - 12
    assert all(res["lag"] == 80 for res, _, _ in out)
    assert min(int(np.min(pr.quantise(loud))), -int(np.max(pr.quantise(loud)))) == -65534


def test_special_values_are_quantised_as_the_definition_says():
    rate = 48000.0
    x = tone(rate, 1200, 90.0, level=0.3, channels=2)
    x[0, 5] = np.nan; x[1, 6] = -np.nan; x[0, 100] = np.inf; x[1, 101] = -np.inf; x[0, 200] = 1e30; x[1, 300] = -1e-42; x[0, 301] = -0.0
    x[1, 400] = np.float32(7.99987793); x[0, 401] = np.float32(-8.0); x[1, 500] = np.float32(0.5 / 4096); x[0, 501] = np.float32(1.5 / 4096)
    res, recs, _ = call([(x, rate, dict(window=256, f_min=fmin_for(rate, 200), f_max=2000.0, max_frames=3))])[0]
    assert res["lag"] == 90 and recs[0]["shift"] == 4              # inf and 1e30 clamp to 32767, -8 to -32767; the other channel adds to it


def test_a_call_with_silent_and_too_short_requests_between_the_others():
    rate = 44100.0
    f = dict(window=256, f_min=fmin_for(rate, 255), f_max=2000.0, max_frames=3)
    L = 256 + 256
    reqs = [(np.zeros((1, L - 1), np.float32), rate, f),                        # too short, first
            (tone(rate, 1400, 64.0), rate, f),
            (np.zeros((2, 1400), np.float32), rate, f),                         # silence: frames, all silent
            (tone(rate, 300, 64.0), rate, f),                                   # too short between the others
            (tone(rate, 1400, 64.0, level=0.0005), rate, f),                    # below the gate
            (tone(rate, 2000, 111.0, channels=2), rate, dict(f, first_frame=3, num_frames=1900)),
            (np.full((1, 1400), 0.25, np.float32), rate, f),                    # DC: unvoiced
            (tone(rate, 200, 64.0), rate, f)]                                   # too short, last
    out = call(reqs)
    assert [res["frames"] for res, _, _ in out] == [0, 3, 3, 0, 3, 3, 3, 0]
    assert [res["lag"] for res, _, _ in out] == [0, 64, 0, 0, 0, 111, 0, 0]
    assert [r["flag"] for r in out[2][1]] == [pr.SILENT] * 3 == [r["flag"] for r in out[4][1]] and [r["flag"] for r in out[6][1]] == [pr.UNVOICED] * 3


def test_the_largest_frame():
    rate = 48000.0
    out = call([(tone(rate, 4096 + 2048 + 9, 1000.5, channels=2), rate, dict(window=4096, f_min=fmin_for(rate, 2047), f_max=2000.0, first_frame=3, num_frames=4096 + 2048 + 5))],
               count_limit=0)
    assert out[0][2]["tiles"] == 8 and out[0][2]["frames"] == 1 and out[0][0]["lag"] in (1000, 1001)


# ---- pick and vote on hand-made d ---------------------------------------------------------------------------------------------------
def pick_vote(ds, tmin, tmax, threshold=154, silent=None, shift=None, rate=48000.0):
    K = len(ds)
    d = np.array(ds, np.uint64).reshape(K, tmax + 1)
    silent = np.array(silent if silent is not None else [0] * K, np.int32)
    shift = np.array(shift if shift is not None else [0] * K, np.int32)
    frames = (_abi.PitchFrame * K)()
    out = _abi.Pitch()
    assert lib().zlpt_pick_vote(K, tmin, tmax, threshold, d.ctypes.data, silent.ctypes.data, shift.ctypes.data, rate, C.addressof(frames), C.addressof(out)) == 0
    recs = [pr.pick([int(v) for v in d[k]], tmin, tmax, threshold, bool(silent[k]), int(shift[k])) for k in range(K)]
    for k in range(K):
        assert {f: int(getattr(frames[k], f)) for f in pr.FRAME_INTS} == recs[k], (k, recs[k])
    want = pr.finish(pr.vote(recs), rate)
    same_result(out, want, "vote")
    return want, recs


def valley(tmax, at, depth=10, high=10 ** 6):
    """d with one valley: `high` everywhere, falling to `depth` at lag `at`"""
    d = [high] * (tmax + 1)
    for k, v in ((-2, high // 2), (-1, high // 8), (0, depth), (1, high // 8 + 1), (2, high // 2)):
        if 1 <= at + k <= tmax + 1:
            d[at + k - 1] = v
    return d


def test_pick_edges():
    tmin, tmax = 10, 300
    # t0 = t_min: the valley's wall is already below the threshold there, and the descent walks down to the floor
    d = valley(tmax, 12)
    res, recs = pick_vote([d], tmin, tmax, threshold=1024)
    assert d[tmin - 1] * tmin * 1024 < 1024 * sum(d[:tmin]) and d[tmin - 1] > d[tmin] > d[tmin + 1]
    assert recs[0]["lag"] == 12 and (recs[0]["d_lo"], recs[0]["d_mid"], recs[0]["d_hi"]) == (d[10], d[11], d[12])
    # a descent that ends at t_max: d falls all the way; the triple still exists because d reaches t_max + 1
    d = [10 ** 6] * 290 + [10 ** 6 - 90000 * k for k in range(1, 12)]
    assert len(d) == tmax + 1
    res, recs = pick_vote([d], tmin, tmax, threshold=1024)
    assert recs[0]["lag"] == tmax and recs[0]["d_hi"] == d[tmax] < recs[0]["d_mid"] and res["hz"] == np.float32(48000.0 / tmax)     # (a straight line: den = 0, no parabola)
    # the descent runs on d, not on the normalised value: a plateau stops it (d[t + 1] >= d[t] with equality)
    d = valley(tmax, 100); d[100] = d[99]
    assert pick_vote([d], tmin, tmax)[1][0]["lag"] == 100
    # below the threshold only in front of t_min or only at t_max + 1: unvoiced
    d = valley(tmax, 5)
    assert pick_vote([d], tmin, tmax)[1][0] == dict(lag=0, clarity=0, shift=0, flag=pr.UNVOICED, d_lo=0, d_mid=0, d_hi=0, cum=0)
    d = [10 ** 6] * tmax + [0]
    assert pick_vote([d], tmin, tmax)[1][0]["flag"] == pr.UNVOICED
    # all zero: C = 0, unvoiced; silent wins over everything; the shift is kept
    assert pick_vote([[0] * (tmax + 1)], tmin, tmax)[1][0]["flag"] == pr.UNVOICED
    assert pick_vote([valley(tmax, 100)], tmin, tmax, silent=[1], shift=[3])[1][0] == dict(lag=0, clarity=0, shift=3, flag=pr.SILENT, d_lo=0, d_mid=0, d_hi=0, cum=0)
    # the largest values: d < 2^38 at t_max = 2047 keeps both sides of the comparison below 2^60
    big = 2 ** 38 - 1
    d = [big] * 2048; d[2000] = big // 8; d[2001] = 0; d[2002] = big // 8
    res, recs = pick_vote([d], 25, 2047, threshold=1024)
    assert recs[0]["lag"] == 2002 and recs[0]["cum"] < 2 ** 49 and recs[0]["clarity"] == pr.level(recs[0]["cum"] + 1)


def test_vote_ties_in_the_median_and_in_the_clarity():
    tmin, tmax = 10, 300
    # lags 100, 100, 200, 200: the lower median is 100; 200 is not consistent; the two at 100 tie in clarity: the earlier frame
    res, recs = pick_vote([valley(tmax, 200), valley(tmax, 100), valley(tmax, 200), valley(tmax, 100)], tmin, tmax)
    assert [r["lag"] for r in recs] == [200, 100, 200, 100] and recs[1]["clarity"] == recs[3]["clarity"]
    assert (res["voiced"], res["consistent"], res["frame"], res["lag"]) == (4, 2, 1, 100) and res["confidence"] == 0.5
    # the consistent band: |lag - med| <= med >> 5 = 3 at med = 100; the deeper valley wins although it is later
    res, recs = pick_vote([valley(tmax, 100), valley(tmax, 103, depth=1), valley(tmax, 104, depth=0), valley(tmax, 97), valley(tmax, 100)], tmin, tmax)
    assert (res["voiced"], res["consistent"], res["frame"], res["lag"]) == (5, 4, 1, 103)
    # silent and unvoiced frames do not vote; one voiced frame of many is its own median
    res, recs = pick_vote([[0] * (tmax + 1), valley(tmax, 150), valley(tmax, 100)], tmin, tmax, silent=[0, 0, 1], shift=[0, 2, 0])
    assert (res["frames"], res["voiced"], res["consistent"], res["frame"], res["lag"], res["shift"]) == (3, 1, 1, 1, 150, 2)
    # nobody voiced: every field 0 except frames
    res, recs = pick_vote([[0] * (tmax + 1)] * 3, tmin, tmax)
    assert res["frames"] == 3 and all(int(res[k]) == 0 for k in pr.RESULT_INTS if k != "frames")
    # 256 frames, a lane each
    res, recs = pick_vote([valley(tmax, 100 + (k % 2)) for k in range(256)], tmin, tmax)
    assert (res["frames"], res["consistent"], res["frame"], res["lag"]) == (256, 256, 0, 100)


# ---- the edge cases that reach the device as clips (tests/pitch_cases.py) -------------------------------------------------------------
def test_every_edge_case_hits_its_edge():
    """by the restatement alone: a case that stops hitting its edge fails here, without a GPU.  The list holds every kind of case"""
    cases = pc.cases()
    for c in cases:
        pc.holds(c)
    names = " | ".join(c["name"] for c in cases)
    for kind in ("threshold at equality", "plateau", "descent ends at t_max", "neighbouring lanes", "neighbouring waves", "one lane", "at t_max + 1", "at t_min - 1", "DC",
                 "gate at equality, mono", "gate one below, mono", "gate at equality, stereo", "shift 0", "shift 4", "in the lagged tail", "at the last sample", "= -32768",
                 "even count", "consistent band", "silent frames", "256 frames", "different waves", "neighbouring frames", "bin 7", "bin 8", "bin 511", "bin 512",
                 "median 31", "median 32", "mono, first frame 2", "mono, first frame 6", "window 256, t_max + 1 = 256", "window 576", "t_max + 1 = 255", "t_max + 1 = 257"):
        assert kind in names, kind
    assert len(cases) == 82
    for c in pc.too_short():
        res, recs, ds = pc.want(c)
        assert res["frames"] == 0 and recs == [] and all(int(res[k]) == 0 for k in pr.RESULT_INTS)


def test_the_edge_cases_through_the_harness():
    """the whole list in one call of the host walk, requests without a frame first, last and twice in a row in the middle: d, every
    frame record and every result equal the restatement's (call), and the named outcomes are the harness's too"""
    cases, (s0, s1) = pc.cases(), pc.too_short()
    half = len(cases) // 2
    order = [s0] + cases[:half] + [s1, s0] + cases[half:] + [s1]
    out = call([(c["x"], c["rate"], c["req"]) for c in order])
    assert len(out) == len(cases) + 4
    for c, (res, recs, g) in zip(order, out):
        if "pred" in c:
            pc.literal(c, res, recs)
        else:
            assert g["frames"] == 0 and res["frames"] == 0


# ---- defaults and limits ------------------------------------------------------------------------------------------------------------
FIELDS = ("window", "max_frames", "f_min", "f_max", "threshold", "gate")


def resolve(sr, num_frames=1000, first_frame=0, **f):
    r = _abi.PitchRequest(0, first_frame, num_frames, f.get("window", 0), f.get("max_frames", 0), f.get("f_min", 0.0), f.get("f_max", 0.0), f.get("threshold", 0), f.get("gate", 0))
    before = bytes(r)
    rc = zlhip().zlhip_pitch_resolve(sr, C.byref(r))
    want = pr.resolve(sr, num_frames, first_frame=first_frame, **f)
    if rc != 0:
        assert rc == _abi.ZLHIP_ERR_INVALID and bytes(r) == before and want is None, (f, want)     # a refused request is left as it was
        return None
    got = {k: getattr(r, k) for k in FIELDS}
    assert got == want, (got, want)
    a = [C.c_int32(f.get("window", 0)), C.c_int32(f.get("max_frames", 0)), C.c_float(f.get("f_min", 0.0)), C.c_float(f.get("f_max", 0.0)), C.c_int32(f.get("threshold", 0)),
         C.c_int32(f.get("gate", 0))]
    assert lib().zlpt_resolve(sr, *[C.byref(v) for v in a]) == 0 and [v.value for v in a] == [got[k] for k in FIELDS]
    return got


def test_defaults():
    for sr, window in {8000: 320, 22050: 832, 44100: 1664, 48000: 1792, 96000: 3520}.items():
        assert resolve(float(sr)) == dict(window=window, max_frames=64, f_min=55.0, f_max=1760.0, threshold=154, gate=8)
    assert resolve(48000.0, f_min=30.0)["window"] == 3200 and resolve(48000.0, f_min=23.5)["window"] == 4096
    assert resolve(48000.0, window=1024, f_min=100.0, gate=100) == dict(window=1024, max_frames=64, f_min=100.0, f_max=1760.0, threshold=154, gate=100)
    assert resolve(0.0) is None and resolve(float("nan")) is None and resolve(-48000.0) is None
    # where the default window would fall below 256 the request is refused; a window given by hand works
    assert resolve(4000.0, f_max=1000.0) is None and resolve(4000.0, f_max=1000.0, window=256) is not None


def test_every_limit_either_side():
    ok = dict(window=1792, max_frames=64, f_min=55.0, f_max=1760.0, threshold=154, gate=8)
    for w in (896, 960, 4032, 4096):
        assert resolve(48000.0, **dict(ok, window=w)) == dict(ok, window=w)
    for w in (64, 192, 872, 900, 1791, 4097, 4160, -1792):
        assert resolve(48000.0, **dict(ok, window=w)) is None, w
    assert resolve(48000.0, **dict(ok, window=256, f_min=200.0)) is not None and resolve(48000.0, **dict(ok, window=192, f_min=400.0)) is None
    # t_max + 1 <= window: 48000 / 188 = 255.3
    assert resolve(48000.0, **dict(ok, window=256, f_min=188.0)) is not None and resolve(48000.0, **dict(ok, window=256, f_min=187.0)) is None
    # t_max + 1 <= 2048: 48000 / 23.45 = 2046.9, 48000 / 23.43 = 2048.7
    assert resolve(48000.0, **dict(ok, window=4096, f_min=23.45)) is not None and resolve(48000.0, **dict(ok, window=4096, f_min=23.43)) is None
    assert resolve(96000.0, **dict(ok, window=4096)) is not None and resolve(192000.0, **dict(ok, window=4096)) is None
    assert resolve(8000.0, **dict(ok, window=512, f_min=20.0, f_max=3999.0)) is not None
    for lo, hi in ((19.99, 1760.0), (55.0, 4000.0), (55.0, 4001.0), (1760.0, 1760.0), (1760.0, 55.0), (-55.0, 1760.0), (float("nan"), 1760.0), (55.0, float("nan")),
                   (55.0, float("inf")), (float("-inf"), 1760.0)):
        assert resolve(8000.0, **dict(ok, window=512, f_min=lo, f_max=hi)) is None, (lo, hi)
    for k, good, bad in (("threshold", (1, 1024), (-1, 1025)), ("gate", (1, 32767), (-1, 32768)), ("max_frames", (1, 256), (-1, 257))):
        for v in good:
            assert resolve(48000.0, **dict(ok, **{k: v})) == dict(ok, **{k: v})
        for v in bad:
            assert resolve(48000.0, **dict(ok, **{k: v})) is None, (k, v)
    assert resolve(48000.0, num_frames=1, **ok) == ok and resolve(48000.0, num_frames=0, **ok) is None and resolve(48000.0, num_frames=-5, **ok) is None
    assert resolve(48000.0, first_frame=-1, **ok) is None
    assert zlhip().zlhip_pitch_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = _abi.PitchRequest(0, 0, 100000, 0, 0, 0.0, 0.0, 0, 0)
    out = (_abi.Pitch * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert z.zlhip_sound_pitch(None, C.byref(r), out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_pitch_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_pitch_frames(None, 0, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_pitch_diff(None, 0, 0, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_pitch_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_pitch_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * 80 and n.value == -7
    lz = C.CDLL(build.build_engine())
    lz.libzl_hotpath_clip_pitch.restype = C.c_int
    lz.libzl_hotpath_clip_pitch.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lz.libzl_hotpath_clip_detect_root_note.restype = C.c_int
    lz.libzl_hotpath_clip_detect_root_note.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    assert lz.libzl_hotpath_clip_pitch(None, 0.0, 0.0, None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clip_detect_root_note(None, 0.5, C.byref(n)) == _abi.ZLHIP_ERR_INVALID and n.value == -7


def test_pitch_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_pitch_request", _abi.PitchRequest), ("zlhip_pitch", _abi.Pitch), ("zlhip_pitch_frame", _abi.PitchFrame))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:3] == [36, 80, 48]
    assert got[3:] == list(range(0, 36, 4)) + list(range(0, 48, 4)) + [48, 56, 64, 72] + [0, 4, 8, 12, 16, 24, 32, 40]


def test_pitch_kernels_resources(built):
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_pitch_kernel_resources.txt")
    assert os.path.exists(path), "no zl_pitch kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    diff = [r for n, r in rows.items() if "zl_k_pitch_diff" in n]
    pick = [r for n, r in rows.items() if "zl_k_pitch_pick" in n]
    vote = [r for n, r in rows.items() if "zl_k_pitch_vote" in n]
    assert len(diff) == 1 and len(pick) == 1 and len(vote) == 1 and len(rows) == 3, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    # the frame's samples as int16 (the largest L is 4096 + 2048) and the reductions' four words
    assert diff[0]["lds"] == 2 * (4096 + 2048) + 32, rows
    assert diff[0]["vgprs"] <= 64 and diff[0]["waves"] >= 8, rows
    # d and C as uint64 for 2048 lags; the histogram's 2048 bins
    assert pick[0]["lds"] == 2 * 8 * 2048 + 32 and vote[0]["lds"] == 4 * 2048 + 32, rows


# ---- the walk under the sanitizers --------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/pitch_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with
    AddressSanitizer and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the
    environment loads in front of it."""
    exe = str(tmp_path / "pitch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pitch_check.cpp"), "-o", exe])
    for args in (["1", "12"], ["2", "12"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "pitch check ok" in rc.stdout
