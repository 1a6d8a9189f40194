"""Key detection, GPU tier: the kernels of libzl_amd/csrc/zl_key.hip against the numpy / Python-integer restatement (tests/key_ref.py,
fed with the library's table): re and im of every frame and bin, the per-bin totals, the chroma and every integer of the result bit
for bit, the two confidences with == (both sides run the same serial double arithmetic).  The shapes are the smallest at which the
kernels can still go wrong: 8 kHz clips and narrowed note ranges, so a span is some hundred samples, unless a test says otherwise."""
import ctypes as C
import os

import numpy as np
import pytest

import key_ref as kr
import rt_between_cycles as rtc

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 8000.0
KEYS = ("first_frame", "num_frames", "hop", "max_frames", "a4_hz", "note_lo", "note_hi", "q", "gate")
TABLE = ("hop", "max_frames", "a4_hz", "note_lo", "note_hi", "q", "gate")
NARROW = dict(note_lo=57, note_hi=80, q=17)                                          # 8 kHz: L = 618, three bin groups
TINY = dict(note_lo=47, note_hi=59, q=1)                                             # 8 kHz: L = 66, the top bin 32 samples


def _tone(ch, length, notes, seed=0, level=0.3, sr=SR):
    """a few notes with two harmonics each and a little noise; the channels differ"""
    rng = np.random.default_rng(seed)
    t = np.arange(length) / sr
    y = np.stack([sum(np.sin(2 * np.pi * kr.hz_of(n) * t + 0.4 * c + n) + 0.5 * np.sin(4 * np.pi * kr.hz_of(n) * t + c) for n in notes) for c in range(ch)])
    return (level * (y / (1.5 * len(notes)) + 0.003 * rng.standard_normal((ch, length)))).astype(f32)


def _upload(syn, src, sr=SR):
    return syn.register_clip(src[0], src[1] if src.shape[0] == 2 else None, sr)


def _table(rate, r):
    from libzl_amd import _abi
    return kr.library_table(_abi.load(), rate, **{k: r[k] for k in TABLE if k in r})


def _want(src, rate, r):
    bins, T = _table(rate, r)
    first = r.get("first_frame", 0)
    return kr.key(src, rate, bins, T, first, r.get("num_frames", np.atleast_2d(src).shape[1] - first), r.get("hop", 0), r.get("max_frames", 0), r.get("gate", 0))


def _same(got, res):
    return (all(int(got[k]) == int(res[k]) for k in kr.RESULT_INTS) and tuple(got["chroma"]) == res["chroma"] and got["confidence"] == res["confidence"]
            and got["second_confidence"] == res["second_confidence"])


def _check_batch(syn, reqs, srcs, rates=None, every_frame=True):
    """reqs: dicts with "clip" and any of zlhip_key_request's fields; srcs: {clip: planar}.  The totals, re and im (of every frame, or of
    the first and the last) and the result of every request against the restatement; returns the mismatches and the results"""
    bad = []
    outs = syn.clip_key_batch(reqs)
    for i, (r, got) in enumerate(zip(reqs, outs)):
        res, totals, recs = _want(srcs[r["clip"]], (rates or {}).get(r["clip"], SR), r)
        okT = syn.key_bins(i).dtype == np.uint64 and [int(v) for v in syn.key_bins(i)] == totals
        okF = syn.key_frames(i) == len(recs)
        for k in (range(len(recs)) if every_frame or not recs else sorted({0, len(recs) - 1})):
            re, im = syn.key_frame(i, k)
            okF = okF and re.dtype == np.int64 and [int(v) for v in re] == recs[k]["re"] and [int(v) for v in im] == recs[k]["im"]
        if not (okT and okF and _same(got, res)):
            bad.append((srcs[r["clip"]].shape, r, "totals" if not okT else "frames" if not okF else ("result", got, res)))
    return bad, outs


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=64, sound_arena_bytes=64 << 20)
    yield s
    s.close()


def test_frame_count_edges(syn):
    """num_frames = L (one frame), L - 1 (none), L + hop - 1 and L + hop (one, then two), max_frames below K (the hop is spread)"""
    src = _tone(1, 6000, (57, 61, 64), 1)
    cid = _upload(syn, src)
    L, hop = _table(SR, NARROW)[0][0][1], 300
    assert L == 618
    reqs = [dict(NARROW, clip=cid, hop=hop, first_frame=7, num_frames=n) for n in (L, L - 1, L + hop - 1, L + hop)]
    reqs += [dict(NARROW, clip=cid, hop=hop, max_frames=mf) for mf in (1, 2, 5)] + [dict(NARROW, clip=cid, hop=hop)]
    bad, outs = _check_batch(syn, reqs, {cid: src})
    assert not bad, (len(bad), bad[:3])
    assert [o["frames"] for o in outs] == [1, 0, 1, 2, 1, 2, 5, 18]
    assert outs[1]["tonic"] == -1 and all(o["tonic"] == 9 and o["mode"] == 0 for o in outs[:1] + outs[2:])              # A major
    syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_layouts_and_alignment(syn, ch):
    """first_frame at every residue of the 16-byte load group (four mono frames, two stereo frames) and one more; a region that ends at
    the sound's last frame, whose last group is partly behind the data"""
    n = 4001 + ch
    src = _tone(ch, n, (62, 66, 69), 10 + ch)
    cid = _upload(syn, src)
    reqs = [dict(NARROW, clip=cid, hop=257, first_frame=first, num_frames=n - first) for first in range(5)]
    reqs += [dict(NARROW, clip=cid, hop=257, first_frame=first, num_frames=3000 + first) for first in (1, 2, 3)]
    bad, outs = _check_batch(syn, reqs, {cid: src})
    assert not bad, (len(bad), bad[:3])
    assert all(o["frames"] >= 10 and o["tonic"] == 2 and o["mode"] == 0 for o in outs)                                   # D major
    syn.unregister_clip(cid)


def test_span_limits(syn):
    """one bin with N clamped to 32768 (96 kHz, note 36, one frame: the longest span, sixteen staged chunks); the smallest N the resolve
    accepts (32); a top bin just under rate / 2, where step is near 2^31"""
    long_ = _tone(2, 32768 + 11, (36, 43), 7, level=2.0, sr=96000.0)
    short = _tone(1, 2000, (52,), 6)
    high = _tone(1, 3000, (100, 107), 8)
    a, b, c = _upload(syn, long_, 96000.0), _upload(syn, short), _upload(syn, high)
    top = dict(note_lo=100, note_hi=106, q=34, hop=500, a4_hz=470.0)
    reqs = [dict(clip=a, note_lo=36, note_hi=36, first_frame=5, num_frames=32768 + 5), dict(TINY, clip=b, hop=64, max_frames=5), dict(top, clip=c)]
    assert _table(96000.0, reqs[0])[0][0][1] == 32768 and _table(SR, reqs[1])[0][-1][1] == 32 and _table(SR, reqs[2])[0][-1][2] > 0.99 * (1 << 31)
    bad, outs = _check_batch(syn, reqs, {a: long_, b: short, c: high}, {a: 96000.0})
    assert not bad, bad
    assert [o["frames"] for o in outs] == [1, 5, 6] and all(o["sounding"] == o["frames"] for o in outs)
    for cid in (a, b, c):
        syn.unregister_clip(cid)


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                    0x39000000, 0x38FFFFFF, 0x39C00000, 0xB9C00000, 0x3A200000], np.uint32)


def test_sample_content(syn):
    """+-1.0 in both channels on every sample as a square wave on a bin's frequency, and the same clamped at the quantiser's limit
    (+-100: |m| = 65534, where a single term reaches 2^31 - 131070); NaN, +-inf, -0 and denormals; loud frames between silent ones"""
    t = np.arange(3000)
    square = np.where(np.sin(2 * np.pi * kr.hz_of(64) * t / SR) >= 0, 1.0, -1.0).astype(f32)
    srcs = [np.stack([square, square]), np.stack([square, square]) * f32(100.0)]
    rng = np.random.default_rng(3)
    special = rng.permutation(np.tile(SPECIAL, 300))[:6000].reshape(2, -1).view(f32).copy()
    special[:, 1500:] = np.where(np.arange(1500) % 3 == 0, special[:, 1500:], _tone(2, 1500, (60, 64, 67), 4))
    gaps = _tone(1, 6000, (60, 64, 67), 3)
    gaps[:, :1500] = 0.0
    gaps[:, 3000:4500] = 0.0
    srcs += [special, gaps]
    ids = [_upload(syn, s) for s in srcs]
    reqs = [dict(NARROW, clip=ids[0], hop=700), dict(NARROW, clip=ids[1], hop=700, first_frame=1), dict(NARROW, clip=ids[2], hop=400),
            dict(NARROW, clip=ids[3], hop=750)]
    bad, outs = _check_batch(syn, reqs, dict(zip(ids, srcs)))
    assert not bad, bad
    re, im = syn.key_frame(1, 0)
    assert max(np.abs(re).max(), np.abs(im).max()) > (1 << 30) * 200                  # hundreds of terms near 2^31 each on the square's own bin
    assert outs[3]["frames"] == 8 and outs[3]["sounding"] == 4
    assert all(not syn.key_frame(3, k)[0].any() and not syn.key_frame(3, k)[1].any() for k in (0, 1, 4, 5))               # silent frames read 0
    for cid in ids:
        syn.unregister_clip(cid)


def test_a_batch_of_14_mixed_requests(syn):
    """rates, channel counts, bin counts (1, 7, 8, 9, 24, 60), hops and a "no key" request in one call: the totals, re and im of the first
    and the last frame of each, the results; the same requests one by one give the same answers"""
    from libzl_amd import _abi
    a = _tone(1, 7000, (57, 61, 64), 21)
    b = _tone(2, 9000, (50, 57, 65), 22, sr=11025.0)
    c = kr.cadence(12000.0, 5, 1)
    d = np.zeros((2, 5000), f32)
    ids = [_upload(syn, a), _upload(syn, b, 11025.0), _upload(syn, c, 12000.0), _upload(syn, d)]
    srcs, rates = dict(zip(ids, (a, b, c, d))), {ids[1]: 11025.0, ids[2]: 12000.0}
    reqs = [dict(NARROW, clip=ids[0], hop=700), dict(clip=ids[0], note_lo=60, note_hi=60, q=17, hop=333), dict(clip=ids[0], note_lo=60, note_hi=66, q=17, hop=500),
            dict(clip=ids[0], note_lo=60, note_hi=67, q=17, hop=500, first_frame=3), dict(clip=ids[0], note_lo=60, note_hi=68, q=17, hop=500, max_frames=3),
            dict(clip=ids[1], note_lo=45, note_hi=70, q=20, hop=1111, first_frame=1), dict(clip=ids[1], note_lo=45, note_hi=70, q=20, hop=1111, gate=2000),
            dict(clip=ids[1], note_lo=50, note_hi=81, q=12, hop=64, max_frames=9, a4_hz=432.0), dict(clip=ids[2]), dict(clip=ids[2], first_frame=9000, num_frames=20001),
            dict(NARROW, clip=ids[3], hop=700), dict(NARROW, clip=ids[0], hop=700, num_frames=617), dict(TINY, clip=ids[0], hop=64, max_frames=256),
            dict(NARROW, clip=ids[0], hop=123, first_frame=2001, num_frames=4999)]
    bad, outs = _check_batch(syn, reqs, srcs, rates, every_frame=False)
    assert not bad, (len(bad), bad[:3])
    assert [o["frames"] for o in outs] == [10, 20, 13, 13, 3, 7, 7, 9, 4, 2, 7, 0, 109, 36]
    assert outs[8]["tonic"] == 5 and outs[8]["mode"] == 1 and outs[10]["tonic"] == -1 and outs[11]["tonic"] == -1 and outs[6]["sounding"] == 0
    assert outs[10] == dict(outs[10], sounding=0, confidence=0.0, chroma=(0,) * 12)
    assert [syn.clip_key_batch([r])[0] for r in reqs] == outs
    # the plain C call writes 136 bytes per request and nothing behind them
    arr = (_abi.KeyRequest * 14)(*[_abi.KeyRequest(r["clip"], r.get("first_frame", 0), r.get("num_frames", srcs[r["clip"]].shape[1] - r.get("first_frame", 0)),
                                                   *(r.get(k, 0) for k in KEYS[2:])) for r in reqs])
    out = (_abi.Key * 16)()
    C.memset(out, 0x5A, C.sizeof(out))
    assert _abi.load().zlhip_sound_key_batch(syn._e, arr, 14, out) == 0
    assert bytes(out)[14 * 136:] == b"\x5a" * 272 and [out[i].tonic for i in range(14)] == [o["tonic"] for o in outs]
    for cid in ids:
        syn.unregister_clip(cid)


def test_the_calls_frame_limit(syn):
    """65536 frames in one call are accepted; one request more is ZLHIP_ERR_INVALID with nothing launched: out and the last call's
    debug data stay as they were"""
    from libzl_amd import _abi
    src = _tone(1, 400, (52, 55), 31)
    cid = _upload(syn, src)
    r = dict(TINY, clip=cid, hop=1, first_frame=2, num_frames=66 + 255)
    want = _want(src, SR, r)
    assert want[0]["frames"] == 256
    R = _abi.KeyRequest(cid, 2, 66 + 255, 1, 0, 0.0, 47, 59, 1, 0)
    lib = _abi.load()
    out = (_abi.Key * 257)()
    assert lib.zlhip_sound_key_batch(syn._e, (_abi.KeyRequest * 256)(*[R] * 256), 256, out) == 0
    for i in (0, 1, 200, 255):
        assert _same({k: (tuple(out[i].chroma) if k == "chroma" else getattr(out[i], k)) for k, _ in _abi.Key._fields_}, want[0]), i
        assert [int(v) for v in syn.key_bins(i)] == want[1]
    re, im = syn.key_frame(255, 255)
    assert [int(v) for v in re] == want[2][255]["re"] and [int(v) for v in im] == want[2][255]["im"]
    C.memset(out, 0x5A, C.sizeof(out))
    assert lib.zlhip_sound_key_batch(syn._e, (_abi.KeyRequest * 257)(*[R] * 257), 257, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * (257 * 136) and b"65536" in lib.zlhip_last_error(syn._e)
    assert syn.key_frames(255) == 256 and [int(v) for v in syn.key_bins(255)] == want[1]
    re2, im2 = syn.key_frame(255, 255)
    assert np.array_equal(re, re2) and np.array_equal(im, im2)
    # other refusals: a request outside its limits or outside the data, a sound that does not exist
    bad = [_abi.KeyRequest(cid, 0, 401, 0, 0, 0.0, 47, 59, 1, 0), _abi.KeyRequest(cid, 0, 400, 0, 257, 0.0, 47, 59, 1, 0), _abi.KeyRequest(63, 0, 400, 0, 0, 0.0, 47, 59, 1, 0),
           _abi.KeyRequest(cid, 0, 400, 0, 0, 0.0, 47, 107, 1, 0), _abi.KeyRequest(cid, 0, 400, 0, 0, float("nan"), 47, 59, 1, 0)]
    for q in bad:
        assert lib.zlhip_sound_key_batch(syn._e, (_abi.KeyRequest * 2)(R, q), 2, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * (257 * 136) and syn.key_frames(255) == 256
    syn.unregister_clip(cid)


def test_key_follows_the_rerender(syn):
    """setPitch(+2) re-renders the clip: the answer comes from the data that plays, equals the restatement on a snapshot of it, and a
    cadence's tonic moves by 2"""
    rate = 12000.0
    src = np.repeat(kr.cadence(rate, 0, 0), 2, 0)
    cid = _upload(syn, src, rate)
    before = syn.clip_key(cid)
    assert _same(before, _want(src, rate, {})[0]) and (before["tonic"], before["mode"]) == (0, 0)
    syn.rerender_clip(cid, pitch=2.0)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert not np.array_equal(played[:, :4000], src[:, :4000])
    bad, outs = _check_batch(syn, [dict(clip=cid), dict(clip=cid, first_frame=3, num_frames=played.shape[1] - 7, hop=5000)], {cid: played}, {cid: rate})
    assert not bad, bad
    assert (outs[0]["tonic"], outs[0]["mode"]) == (2, 0) and (outs[1]["tonic"], outs[1]["mode"]) == (2, 0)
    from libzl_amd import ZlHipError
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_key(cid, 0, played.shape[1] + 1)
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert syn.clip_key(cid) == before
    syn.unregister_clip(cid)


def test_key_follows_the_rate_conversion(syn):
    """the bin table is built from the sound's rate: after convert_clips to 48 kHz the spans, the totals, re and im and the result are
    those of the converted data at 48 kHz"""
    src = _tone(2, 11025, (57, 61, 64), 51, sr=44100.0)
    cid = _upload(syn, src, 44100.0)
    r = dict(NARROW, clip=cid, hop=2000)
    assert _table(44100.0, NARROW)[0][0][1] == 3408 and _table(48000.0, NARROW)[0][0][1] == 3710
    bad, outs = _check_batch(syn, [r], {cid: src}, {cid: 44100.0})
    assert not bad, bad
    assert outs[0]["frames"] == 4 and (outs[0]["tonic"], outs[0]["mode"]) == (9, 0)
    syn.convert_clips([cid], 48000.0)
    L, R = syn.read_clip(cid)
    played = np.stack([L, R])
    assert syn.clip_info(cid)["sample_rate"] == 48000.0 and abs(played.shape[1] - 12000) <= 2
    bad, outs = _check_batch(syn, [r, dict(r, first_frame=3, num_frames=played.shape[1] - 7, hop=700)], {cid: played}, {cid: 48000.0})
    assert not bad, bad
    assert outs[0]["frames"] == 5 and all((o["tonic"], o["mode"]) == (9, 0) and o["sounding"] == o["frames"] for o in outs)      # the same sound: A major
    syn.unregister_clip(cid)


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a small arena that held noise, analysed from its first frame and to its last, whose
    16-byte group lies partly behind the data: a neighbour's sample in a head or tail group would change re and im (a full-scale sample
    is 2000 times a quiet one).  The quiet tone sounds under the default gate (amplitude 16 of 4096, mean square 134 per channel against
    64); a gated frame would read 0 and hide a leak"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(9)
        fill = [_upload(s, rng.uniform(-7.9, 7.9, (ch, 60000)).astype(f32)) for _ in range(3)]
        for cid in fill:
            s.unregister_clip(cid)
        L = _table(SR, NARROW)[0][0][1]
        for n in (6001, 3333):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (3001, 3003)]
            t = np.arange(n)
            quiet = np.stack([0.004 * np.sin(2 * np.pi * kr.hz_of(64) * t / SR + 0.4 * c) for c in range(ch)]).astype(f32)
            ids = [_upload(s, x) for x in (loud[0], quiet, loud[1])]
            srcs = dict(zip(ids, (loud[0], quiet, loud[1])))
            # two frames each: the first begins at the request's first frame, the last ends at its last one
            reqs = [dict(NARROW, clip=ids[1], hop=n - L), dict(NARROW, clip=ids[1], first_frame=1, num_frames=n - 1, hop=n - 1 - L),
                    dict(NARROW, clip=ids[0], hop=3001 - L), dict(NARROW, clip=ids[2], hop=3003 - L)]
            bad, outs = _check_batch(s, reqs, srcs)
            assert not bad, bad
            assert all(o["sounding"] == o["frames"] == 2 for o in outs), outs
            assert 0 < max(int(np.abs(v).max()) for k in (0, 1) for v in s.key_frame(1, k)) < 1 << 28       # (a full-scale frame reaches 2^34)
            for cid in ids:
                s.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        notes = ((57, 61, 64), (62, 66, 69))
        srcs = [_tone(1 + i % 2, 60000 + 1001 * i, notes[i % 2], 40 + i) for i in range(8)]
        ids = [_upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        bad, outs = _check_batch(s, [dict(NARROW, clip=cid, first_frame=1, num_frames=x.shape[1] - 3, hop=20000) for cid, x in zip(ids, srcs)], dict(zip(ids, srcs)))
        assert not bad, bad
        assert [(o["tonic"], o["frames"]) for o in outs] == [((9, 2)[i % 2], 3 + (i >= 1)) for i in range(8)]


def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = _upload(s, _tone(2, 20000, (57, 61, 64), 2))
        total0, _ = s.memory_bytes()
        s.clip_loop(cid, 5000, 15000)
        total1, _ = s.memory_bytes()
        s.clip_key(cid, hop=500, **NARROW)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_key(cid, hop=500, **NARROW); s.clip_key(cid, 3, 15000, hop=1000, **TINY); s.clip_loop(cid, 5000, 15000)       # fit the first call's buffers
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
    """After one warm-up call (it allocates the call's buffers) key calls between real-time cycles leave the resident kernel where it
    is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the results right.  The scene's clips are
    1500 to 6000 frames at 22.05, 44.1 and 48 kHz: twelve notes from A4 up with q of 3 to 5 keep a span under 550 frames."""
    sc = rtc.scene()
    tone = _tone(2, 6000, (69, 73, 76), 5, sr=48000.0)             # one more clip, which no voice plays

    def request(cid, k, planar):
        n, first = planar[cid].shape[1], k % 5
        return dict(clip=cid, note_lo=69, note_hi=80, q=(3, 5, 4)[k % 3], hop=(300, 500)[k % 2], first_frame=first, num_frames=min(n - first, 3000))

    def warm_up(syn, planar, rates):
        # more requests, bins, analysis frames and (frame, bin) pairs than any call below
        outs = syn.clip_key_batch([dict(clip=i, note_lo=69, note_hi=80, q=3, hop=100) for i in range(len(planar))] + [dict(clip=len(planar) - 1, note_lo=69, note_hi=80, q=3, hop=100)] * 4)
        assert len(outs) == 25 and sum(o["frames"] for o in outs) > 500

    def between(syn, k, playing, planar, rates):
        # the keys of clips that play, a single call and a batch in turn
        reqs = [request(cid, k, planar) for cid in playing[:2]] + [request(len(planar) - 1, k, planar)]
        gots = [syn.clip_key_batch([r])[0] for r in reqs] if k % 2 else syn.clip_key_batch(reqs)
        return zip(reqs, gots)

    out, ref_bus, stats, todo, planar, rates = rtc.run(sc, [(tone, 48000.0)], warm_up, between)
    assert stats[0] == 1 and stats[1:] == (1, sc.nblocks)
    expect = {}
    for r, got in todo:
        key = tuple(sorted(r.items()))
        if key not in expect:
            expect[key] = _want(planar[r["clip"]], rates[r["clip"]], r)[0]
        assert _same(got, expect[key]), (r, got, expect[key])
    assert max(g["frames"] for _, g in todo) <= 11
    assert len(todo) >= 2 * sc.nblocks and sum(g["tonic"] >= 0 for _, g in todo) >= sc.nblocks
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


def test_group_key_equals_the_single_engine(syn):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    srcs = [_tone(1, 5000, (57, 61, 64), 41), _tone(2, 5000, (62, 65, 69), 42)]
    with SamplerSynthGroup([0, 0], 4, 8, max_sounds=16, sound_arena_bytes=1 << 23) as g:
        for src in srcs:
            cid, gid = _upload(syn, src), _upload(g, src)
            for args in ((0, None, 700, 0, 0.0, 57, 80, 17), (3, 4000, 300, 4, 0.0, 57, 80, 17)):
                a = g.clip_key(gid, *args)
                assert a == syn.clip_key(cid, *args) and a["tonic"] >= 0
            assert _same(a, _want(src, SR, dict(NARROW, first_frame=3, num_frames=4000, hop=300, max_frames=4))[0])
            syn.unregister_clip(cid)
        a, b = g.clip_key_batch([dict(NARROW, clip=0, hop=700), dict(NARROW, clip=1, first_frame=5, num_frames=600)])
        assert (a["tonic"], a["mode"]) == (9, 0) and b["tonic"] == -1 and b["frames"] == 0
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_key_batch([dict(NARROW, clip=0, max_frames=257)])


def test_libzl_clip_key_keys_and_match_key(built):
    """libzl_hotpath_clip_key over a clip from a buffer; clips_keys equal to the single calls; clip_match_key from C major to D major
    reports +2, the clip then analyses as D major, and a second call reports 0"""
    from libzl_amd import _abi, libzl
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        rate = 12000.0
        srcs = [kr.cadence(rate, 0, 0), kr.cadence(rate, 9, 1), np.zeros((1, 36000), f32), kr.cadence(rate, 7, 0)]
        clips = [zl.ClipAudioSource_newFromBuffer(s[0].ctypes.data, None, s.shape[1], rate, b"k%d" % i) for i, s in enumerate(srcs)]
        assert all(clips)
        lib = _abi.load()
        eng = C.c_void_p(zl.libzl_hotpath_engine())
        tonic, mode, conf, semis = C.c_int(-7), C.c_int(-7), C.c_double(-7.0), C.c_int(-7)
        assert zl.libzl_hotpath_clip_key(None, C.byref(tonic), C.byref(mode), C.byref(conf)) < 0 and tonic.value == -7
        singles = []
        for clip, src in zip(clips, srcs):
            cnt = C.c_int32(0)
            cid = zl.ClipAudioSource_engineClip(clip)
            assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(cnt)) >= 0 and cnt.value == src.shape[1]
            pl, pr_ = np.empty(cnt.value, f32), np.empty(cnt.value, f32)
            chans = lib.zlhip_sound_read(eng, cid, pl.ctypes.data, pr_.ctypes.data, cnt.value, C.byref(cnt))
            played = np.stack([pl, pr_]) if chans == 2 else pl[None, :]           # what the clip plays, as the engine holds it
            want = _want(played, rate, {})[0]
            assert zl.libzl_hotpath_clip_key(clip, C.byref(tonic), C.byref(mode), C.byref(conf)) == 0
            assert (tonic.value, mode.value, conf.value) == (want["tonic"], want["mode"], want["confidence"])
            singles.append((tonic.value, mode.value, conf.value))
        assert [s[:2] for s in singles] == [(0, 0), (9, 1), (-1, 0), (7, 0)]
        arr = (C.c_void_p * 5)(*clips, None)
        tonics, modes, confs = (C.c_int * 5)(), (C.c_int * 5)(), (C.c_double * 5)()
        assert zl.libzl_hotpath_clips_keys(arr, 5, tonics, modes, confs) == 3
        assert [(tonics[i], modes[i], confs[i]) for i in range(5)] == singles + [(-1, 0, 0.0)]
        # C major into D major: +2, one re-render; then it is there
        assert zl.libzl_hotpath_clip_match_key(clips[0], 12, 0, C.byref(semis)) < 0 and semis.value == -7
        assert zl.libzl_hotpath_clip_match_key(clips[0], 2, 0, C.byref(semis)) == 1 and semis.value == 2
        assert zl.libzl_hotpath_clip_key(clips[0], C.byref(tonic), C.byref(mode), C.byref(conf)) == 0 and (tonic.value, mode.value) == (2, 0)
        assert zl.libzl_hotpath_clip_match_key(clips[0], 2, 0, C.byref(semis)) == 1 and semis.value == 0
        # A minor into C major: its relative key, nothing to do; silence: no key, the clip stays
        assert zl.libzl_hotpath_clip_match_key(clips[1], 0, 0, C.byref(semis)) == 1 and semis.value == 0
        assert zl.libzl_hotpath_clip_match_key(clips[2], 0, 0, C.byref(semis)) == 0 and semis.value == 0
        # G major into E minor (the relative key of G): 0; into A minor: E minor + 5, and the clip is then in C major, A minor's relative
        assert zl.libzl_hotpath_clip_match_key(clips[3], 4, 1, C.byref(semis)) == 1 and semis.value == 0
        assert zl.libzl_hotpath_clip_match_key(clips[3], 9, 1, C.byref(semis)) == 1 and semis.value == 5
        assert zl.libzl_hotpath_clip_key(clips[3], C.byref(tonic), C.byref(mode), C.byref(conf)) == 0 and (tonic.value, mode.value) == (0, 0)
        for clip in clips:
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
