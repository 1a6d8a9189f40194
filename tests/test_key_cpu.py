"""Key detection, CPU tier: the library's table against numpy's own; the host build of libzl_amd/csrc/zl_key.h
(tests/cpu_harness/key_host.cpp walks a call the way the kernels do, work item by work item, with the header's own arithmetic) against
the numpy / Python-integer restatement (tests/key_ref.py) on every re, im, per-bin total, chroma word and result integer, with == on
the two confidences; the restatement against a float64 correlator with an exact cosine and an exact Hann window; what the definition
does to 24 cadences; "no key" and the limits; the relative-key shift; the struct layouts; the kernels' resources; the host functions
and the walk under the sanitizers (tests/cpp/key_check.cpp).  tests/test_key_gpu.py holds the kernels themselves to the restatement on
the GPU.  Every test but the first feeds the LIBRARY's table to the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import key_ref as kr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("hop", "max_frames", "a4_hz", "note_lo", "note_hi", "q", "gate")

_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_key_harness())
        l.zlky_sizes.argtypes = [C.c_void_p]
        l.zlky_match_shift.restype = C.c_int32
        l.zlky_match_shift.argtypes = [C.c_int32] * 4
        l.zlky_call.restype = C.c_int64
        l.zlky_call.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def request(f, first=0, n=1):
    return _abi.KeyRequest(0, first, n, f.get("hop", 0), f.get("max_frames", 0), f.get("a4_hz", 0.0), f.get("note_lo", 0), f.get("note_hi", 0), f.get("q", 0), f.get("gate", 0))


def table(rate, **f):
    """the library's table of a request at a rate, or None where the library refuses it"""
    return kr.library_table(zlhip(), rate, **f)


def want(x, rate, f):
    x = np.atleast_2d(x)
    first = f.get("first_frame", 0)
    bins, T = table(rate, **f)
    return kr.key(x, rate, bins, T, first, f.get("num_frames", x.shape[1] - first), f.get("hop", 0), f.get("max_frames", 0), f.get("gate", 0))


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000.0, 12000.0, 44100.0, 48000.0, 96000.0])
def test_the_table_equals_numpys_own(rate):
    """N and wstep equal, T equal at all 4096 entries, step within 1 (two exp2 implementations)"""
    for f in (dict(), dict(a4_hz=432.0, q=17), dict(note_lo=24, note_hi=100, q=50), dict(note_lo=60, note_hi=60, q=1, a4_hz=447.5)):
        got = table(rate, **f)
        q = kr.resolve(rate, **f)
        assert (got is None) == (q is None), (rate, f)
        if got is None:
            continue
        bins, T = kr.design(rate, q["a4_hz"], q["note_lo"], q["note_hi"], q["q"])
        assert [b[:2] + b[3:] for b in got[0]] == [b[:2] + b[3:] for b in bins]
        assert all(abs(a[2] - b[2]) <= 1 for a, b in zip(got[0], bins))
        assert np.array_equal(got[1], T) and T.dtype == np.int16
        assert all(b[1] % 2 == 0 and 32 <= b[1] <= 32768 and b[2] < 1 << 31 and b[3] * b[1] <= 1 << 32 for b in got[0])
    assert table(96000.0, note_lo=36, note_hi=36)[0][0][1] == 32768                   # 34 * 96000 / 65.4 = 49900: clamped


# ---- the harness against the restatement ----------------------------------------------------------------------------------------
def arena(x):
    """float32 [channels][frames] -> the arena's layout, padded with zeros to a whole 16-byte group"""
    flat = np.ascontiguousarray(np.asarray(x, np.float32).T).reshape(-1)
    return np.concatenate([flat, np.zeros(-len(flat) % 4, np.float32)])


def same_result(got, res, what):
    assert {k: int(getattr(got, k)) for k in kr.RESULT_INTS} == {k: int(res[k]) for k in kr.RESULT_INTS}, (what, res)
    assert tuple(int(v) for v in got.chroma) == res["chroma"], (what, res)
    assert got.confidence == res["confidence"] and got.second_confidence == res["second_confidence"], (what, got.confidence, res)


def call(requests):
    """requests: (x float32 [channels][frames], rate, dict of zlhip_key_request's fields but id).  Runs the harness walk over the whole
    call and holds re, im, the totals and every result to the restatement; returns (result, totals, frames) per request"""
    n = len(requests)
    reqs = (_abi.KeyRequest * n)()
    datas, refs = [], []
    for i, (x, rate, f) in enumerate(requests):
        x = np.atleast_2d(np.asarray(x, np.float32))
        first = f.get("first_frame", 0)
        reqs[i] = request(f, first, f.get("num_frames", x.shape[1] - first))
        datas.append(arena(x))
        refs.append(want(x, rate, f))
    data = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    length = np.array([np.atleast_2d(r[0]).shape[1] for r in requests], np.int32)
    channels = np.array([np.atleast_2d(r[0]).shape[0] for r in requests], np.int32)
    rate = np.array([r[1] for r in requests], np.float64)
    nb = sum(len(t) for _, t, _ in refs)
    nframes = sum(len(recs) for _, _, recs in refs)
    pairs = sum(len(recs) * len(t) for _, t, recs in refs)
    acc = np.full((pairs + 1, 2), 0x5A5A5A5A, np.int64)
    totals = np.full(nb + 1, 0xDEADBEEF, np.uint64)
    bins = (_abi.KeyBin * nb)()
    silent = np.full(nframes + 1, -7, np.int32)
    geom = np.zeros((n, 8), np.int32)
    base = np.zeros(n, np.int64)
    out = (_abi.Key * n)()
    sizes = np.zeros(4, np.int32)
    lib().zlky_sizes(sizes.ctypes.data)
    assert list(sizes) == [C.sizeof(_abi.Key), C.sizeof(_abi.KeyBin), 64, 16] and C.sizeof(_abi.Key) == 136 and C.sizeof(_abi.KeyBin) == 16
    walk = np.zeros(4, np.int64)
    used = lib().zlky_call(n, C.addressof(reqs), C.addressof(data), length.ctypes.data, channels.ctypes.data, rate.ctypes.data, acc.ctypes.data, pairs, totals.ctypes.data,
                           C.addressof(bins), nb, silent.ctypes.data, nframes, geom.ctypes.data, base.ctypes.data, C.addressof(out), walk.ctypes.data)
    assert used == pairs and int(acc[pairs, 0]) == 0x5A5A5A5A and int(totals[nb]) == 0xDEADBEEF and int(silent[nframes]) == -7
    terms, fb, bb, pb = 0, 0, 0, 0
    for i, (res, tot, recs) in enumerate(refs):
        L, K, hop, nbins, items, frame_base, bin_base, groups = (int(v) for v in geom[i])
        tb = table(float(rate[i]), **requests[i][2])[0]
        q = kr.resolve(float(rate[i]), **{k: v for k, v in requests[i][2].items() if k in FIELDS})
        assert [(b.note, b.n, b.step, b.wstep) for b in bins[bb:bb + nbins]] == tb and L == tb[0][1] and nbins == len(tot)
        assert (K, hop) == kr.frames_of(reqs[i].num_frames, L, q["hop"], q["max_frames"]) and K == len(recs)
        assert (frame_base, bin_base, int(base[i])) == (fb, bb, pb) and groups == -(-nbins // 8) and items == K * groups
        for k, rec in enumerate(recs):
            assert bool(silent[fb + k]) == rec["silent"], (i, k)
            a = acc[pb + k * nbins:pb + (k + 1) * nbins]
            assert [int(v) for v in a[:, 0]] == rec["re"] and [int(v) for v in a[:, 1]] == rec["im"], (i, k)
            terms += 0 if rec["silent"] else sum(b[1] for b in tb)
        assert [int(v) for v in totals[bb:bb + nbins]] == tot, i
        same_result(out[i], res, i)
        fb, bb, pb = fb + K, bb + nbins, pb + K * nbins
    assert list(walk) == [terms, 0, 0, 0], walk
    return refs


def tone(ch, length, rate, notes, seed=0, level=0.3):
    """a few notes with two harmonics each and a little noise; the channels differ"""
    rng = np.random.default_rng(seed)
    t = np.arange(length) / rate
    y = np.stack([sum(np.sin(2 * np.pi * kr.hz_of(n) * t + 0.4 * c + n) + 0.5 * np.sin(4 * np.pi * kr.hz_of(n) * t + c) for n in notes) for c in range(ch)])
    return (level * (y / (1.5 * len(notes)) + 0.003 * rng.standard_normal((ch, length)))).astype(np.float32)


NARROW = dict(note_lo=57, note_hi=80, q=17)                                          # 8 kHz: L = 618, three bin groups
INPUTS = None


def inputs():
    """the inputs of the harness test and of the float64 comparison: (x, rate, fields)"""
    global INPUTS
    if INPUTS is None:
        rng = np.random.default_rng(5)
        loud = rng.choice([-9.0, 9.0], (2, 3000)).astype(np.float32)
        gaps = tone(1, 6000, 8000.0, (60, 64, 67), 3)
        gaps[:, :1500] = 0.0
        gaps[:, 3000:4500] = 0.0
        INPUTS = [(tone(1, 5000, 8000.0, (57, 61, 64), 1), 8000.0, dict(NARROW, hop=700)),
                  (tone(2, 5000, 8000.0, (62, 66, 69), 2), 8000.0, dict(NARROW, hop=512, first_frame=3, num_frames=4990, max_frames=4)),
                  (tone(2, 9000, 11025.0, (50, 57, 65), 4), 11025.0, dict(note_lo=45, note_hi=70, q=20, hop=1111, first_frame=1)),
                  (loud, 8000.0, dict(NARROW, hop=900)),
                  (gaps, 8000.0, dict(NARROW, hop=750)),
                  (tone(1, 2000, 8000.0, (52,), 6), 8000.0, dict(note_lo=47, note_hi=59, q=1, hop=64, max_frames=5)),           # the shortest N the resolve takes
                  (tone(1, 40000, 96000.0, (36, 43), 7, level=2.0), 96000.0, dict(note_lo=36, note_hi=36, hop=5000, max_frames=2)),   # N clamped to 32768
                  (tone(1, 3000, 8000.0, (100, 107), 8), 8000.0, dict(note_lo=100, note_hi=106, q=34, hop=500, a4_hz=470.0))]                   # the top bin just under rate / 2
    return INPUTS


def test_the_harness_equals_the_restatement():
    refs = call(inputs())
    assert [r[0]["frames"] for r in refs] == [7, 4, 7, 3, 8, 5, 2, 6]
    assert refs[3][0]["sounding"] == 3 and max(max(abs(v) for v in rec["re"] + rec["im"]) for rec in refs[3][2]) > 1 << 34
    assert [rec["silent"] for rec in refs[4][2]] == [True, True, False, False, True, True, False, False]
    assert table(8000.0, **inputs()[5][2])[0][-1][1] == 32 and table(8000.0, **inputs()[7][2])[0][-1][2] > 0.99 * (1 << 31)
    assert refs[0][0]["tonic"] == 9 and refs[0][0]["mode"] == 0 and refs[1][0]["tonic"] == 2                 # an A major and a D major triad


def test_a_batch_shares_nothing_between_its_requests():
    """the same requests alone and in one call, in another order: every one equals the restatement (call() checks it) and its bases"""
    ins = inputs()
    call([ins[1], ins[5], ins[0]])
    call([ins[4]])


def test_the_restatement_against_an_exact_correlator():
    """Per frame and bin |re + i im| against float64 sums with an exact cosine and an exact Hann window over the same mixed samples,
    relative to the frame's strongest bin (a bin with nothing in it holds only the tables' rounding, which is what is measured).
    Measured over these inputs: the worst relative difference is 1.223e-3 (MEASURED_WORST; on the bin just under rate / 2; 6.3e-4 without it; the 4096-entry cosine's phase step, 2 pi / 4096 / 2 on
    average, is the main term); allowed: twice that, for table quantisation only.  Python integers check that no input reaches the
    overflow bounds (key_ref.correlate, energy and key assert them)."""
    worst = 0.0
    for x, rate, f in inputs():
        x = np.atleast_2d(x)
        bins, T = table(rate, **f)
        first = f.get("first_frame", 0)
        n = f.get("num_frames", x.shape[1] - first)
        res, _, recs = want(x, rate, f)
        L = bins[0][1]
        K, hop = kr.frames_of(n, L, f.get("hop", 0) or 8192, f.get("max_frames", 0) or 256)
        m = kr.quantise(x[:, first:first + n]).astype(np.float64)
        a4 = kr.resolve(rate, **{k: v for k, v in f.items() if k in FIELDS})["a4_hz"]
        for k, rec in enumerate(recs):
            if rec["silent"]:
                continue
            seg = m[k * hop:k * hop + L]
            exact = [kr.exact_bin(seg[(L - b[1]) // 2:(L - b[1]) // 2 + b[1]], b[0], b[1], rate, a4) for b in bins]
            got = [abs(complex(re, im)) for re, im in zip(rec["re"], rec["im"])]
            rel = max(abs(g - e) for g, e in zip(got, exact)) / max(exact)
            worst = max(worst, rel)
    print("worst relative difference", worst)
    assert worst <= 2 * MEASURED_WORST


MEASURED_WORST = 1.223e-3


# ---- what the definition does to sound ------------------------------------------------------------------------------------------
RATE = 12000.0
_CAD = {}


def cadence_result(tonic, minor):
    if (tonic, minor) not in _CAD:
        _CAD[(tonic, minor)] = want(kr.cadence(RATE, tonic, minor), RATE, {})[0]
    return _CAD[(tonic, minor)]


@pytest.mark.parametrize("minor", [0, 1], ids=["major", "minor"])
def test_the_24_cadences_give_their_key(minor):
    """I-IV-V-I in every major key and i-iv-v-i (natural minor) in every minor key, 0.75 s a chord, 12 kHz, the defaults: the right tonic
    and mode in all 24, the best r at least 0.80 and the runner-up at least 0.03 behind; a major cadence's runner-up is a fifth-related
    or the relative key"""
    for tonic in range(12):
        res = cadence_result(tonic, minor)
        print(tonic, minor, res["confidence"], res["second_confidence"], res["second_tonic"], res["second_mode"])
        assert (res["tonic"], res["mode"]) == (tonic, minor), res
        assert res["confidence"] >= 0.80 and res["confidence"] - res["second_confidence"] >= 0.03, res
        assert res["frames"] == 4 and res["sounding"] == 4
        if not minor:
            assert (res["second_tonic"], res["second_mode"]) in (((tonic + 7) % 12, 0), ((tonic + 5) % 12, 0), ((tonic + 9) % 12, 1)), res


def test_a_repitch_of_two_semitones_moves_the_tonic_by_two():
    for tonic, minor in ((0, 0), (7, 0), (9, 1), (11, 1)):
        res = want(kr.repitch(kr.cadence(RATE, tonic, minor), 2.0), RATE, {})[0]
        assert (res["tonic"], res["mode"]) == ((tonic + 2) % 12, minor), res


def test_silence_dc_a_short_clip_and_gated_frames_give_no_key():
    bins, _ = table(RATE)
    L = bins[0][1]
    nokey = dict(tonic=-1, mode=0, second_tonic=0, second_mode=0, sounding=0, confidence=0.0, second_confidence=0.0, chroma=(0,) * 12)
    cad = kr.cadence(RATE, 4, 0)
    for x, frames, f in ((np.zeros((1, 36000), np.float32), 4, {}), (np.full((2, 36000), 0.3, np.float32), 4, {}), (cad[:, :L - 1], 0, {}),
                         (cad, 4, dict(gate=32767))):
        refs = call([(x, RATE, f)])
        res = refs[0][0]
        assert res == dict(nokey, frames=frames), res
    # DC sounds (it is not gated) and reads as no key because the correlators of a constant are flat to the integer; one sample more
    # and the cadence is there
    assert all(not r["silent"] for r in want(np.full((2, 36000), 0.3, np.float32), RATE, {})[2])
    assert want(cad[:, :L], RATE, {})[0]["frames"] == 1


def test_the_limits():
    z = zlhip()
    ok = dict()

    def resolves(rate, **f):
        r = request(f, f.get("first_frame", 0), f.get("num_frames", 100000))
        rc = z.zlhip_key_resolve(rate, C.byref(r))
        mine = kr.resolve(rate, **f)
        assert (rc == 0) == (mine is not None), (rate, f)
        if rc == 0:
            assert {k: getattr(r, k) for k in FIELDS} == mine
        else:
            assert rc == _abi.ZLHIP_ERR_INVALID
        return rc == 0

    assert resolves(48000.0, **ok) and resolves(8000.0, **NARROW)
    assert not resolves(1760.0, note_hi=81) and resolves(1761.0, note_hi=81)                   # the top bin at rate / 2
    assert not resolves(48000.0, note_lo=10, note_hi=106) and resolves(48000.0, note_lo=10, note_hi=105)       # 97 and 96 bins
    assert not resolves(48000.0, a4_hz=float("nan")) and not resolves(48000.0, a4_hz=float("inf")) and not resolves(float("nan"))
    assert not resolves(48000.0, max_frames=257) and resolves(48000.0, max_frames=256)
    assert not resolves(48000.0, q=257) and not resolves(48000.0, hop=(1 << 24) + 1) and not resolves(48000.0, gate=32768)
    assert not resolves(48000.0, note_lo=70, note_hi=60) and not resolves(48000.0, note_hi=128) and not resolves(48000.0, q=-1)
    assert not resolves(8000.0, note_lo=47, note_hi=60, q=1) and resolves(8000.0, note_lo=47, note_hi=59, q=1)   # the top bin shorter than 32 samples
    assert not resolves(48000.0, first_frame=-1) and not resolves(48000.0, num_frames=0)
    assert z.zlhip_key_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID and z.zlhip_key_design(48000.0, None, None, 0, None, None) == _abi.ZLHIP_ERR_INVALID
    r = request({})
    bins = (_abi.KeyBin * 60)()
    n = C.c_int32(0)
    assert z.zlhip_key_design(48000.0, C.byref(r), C.addressof(bins), 59, C.byref(n), None) == _abi.ZLHIP_ERR_CAPACITY and n.value == 60


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = request({}, 0, 100000)
    out = (_abi.Key * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert z.zlhip_sound_key(None, C.byref(r), out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_key_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_key_bins(None, 0, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_key_frame(None, 0, 0, None, None, 0, C.byref(n), C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_key_timings(None, None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_key_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * 136 and n.value == -7
    from libzl_amd import libzl
    lz = C.CDLL(build.build_engine())
    for name in ("libzl_hotpath_clip_key", "libzl_hotpath_clips_keys", "libzl_hotpath_clip_match_key"):
        getattr(lz, name).restype, getattr(lz, name).argtypes = libzl.SIGNATURES[name]
    assert lz.libzl_hotpath_clip_key(None, None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clip_match_key(None, 0, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID and n.value == -7
    assert lz.libzl_hotpath_clips_keys(None, 1, None, None, None) == _abi.ZLHIP_ERR_INVALID


def test_the_relative_key_shift_over_all_pairs():
    """24 x 24 (clip key, session key) pairs against the rule in three lines; always within -6 .. +5"""
    for a in range(24):
        for b in range(24):
            src = a % 12 if a // 12 == b // 12 else (a % 12 + (9 if a < 12 else 3)) % 12
            shift = (b % 12 - src + 6) % 12 - 6
            assert lib().zlky_match_shift(a % 12, a // 12, b % 12, b // 12) == shift == kr.match_shift(a % 12, a // 12, b % 12, b // 12) and -6 <= shift <= 5
    assert lib().zlky_match_shift(0, 0, 2, 0) == 2 and lib().zlky_match_shift(0, 0, 9, 1) == 0 and lib().zlky_match_shift(9, 1, 0, 0) == 0


def test_key_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_key_request", _abi.KeyRequest), ("zlhip_key", _abi.Key), ("zlhip_key_bin", _abi.KeyBin))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:3] == [40, 136, 16]
    assert got[3:] == list(range(0, 40, 4)) + list(range(0, 24, 4)) + [24, 32, 40] + [0, 4, 8, 12]


def test_key_kernels_resources(built):
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_key_kernel_resources.txt")
    assert os.path.exists(path), "no zl_key kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    gate = [r for n, r in rows.items() if "zl_k_key_gate" in n]
    corr = [r for n, r in rows.items() if "zl_k_key_correlate" in n]
    fold = [r for n, r in rows.items() if "zl_k_key_fold" in n]
    assert len(gate) == 1 and len(corr) == 1 and len(fold) == 1 and len(rows) == 3, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    # the paired table (4096 words) and a chunk of 2048 mixed samples: six workgroups a CU, which is what bounds the waves
    assert corr[0]["lds"] == 4 * 4096 + 4 * 2048, rows
    assert corr[0]["vgprs"] <= 64 and corr[0]["waves"] >= 6, rows
    assert gate[0]["lds"] == 32 and fold[0]["lds"] == 8 * 96 + 4 * 96, rows


# ---- the host functions and the walk under the sanitizers -----------------------------------------------------------------------
def test_host_functions_and_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/key_check.cpp: resolve, design, frames, finish and the relative-key shift on their edges, then the harness walk over
    random calls with buffers of exactly the size needed, built with AddressSanitizer and UBSan.  The sanitizers' runtimes are linked
    into the program (-static-lib*san), so it runs whatever else the environment loads in front of it."""
    exe = str(tmp_path / "key_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "key_check.cpp"), "-o", exe])
    for args in (["1", "10"], ["2", "10"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "key check ok" in rc.stdout
