"""Tempo estimate, CPU tier: the host build of libzl_amd/csrc/zl_tempo.h (tests/cpu_harness/tempo_host.cpp walks a call the way the
kernels do, work item by work item, with the header's own arithmetic) against the numpy / Python-integer restatement
(tests/tempo_ref.py) on every integer and with == on bpm and confidence; what the definition does to sound, with the restatement
alone; the defaults and the limits; the new kernels' resources; the walk under the sanitizers (tests/cpp/tempo_check.cpp).
The tie cases that reach the kernels as clips (tests/tempo_cases.py): every predicate, and the list through the walk.
tests/test_tempo_gpu.py and tests/test_tempo_edges_gpu.py hold the kernels themselves to the restatement on the GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import tempo_cases as tc
import tempo_ref as tr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("lag_coarse", "lag_fine", "doublings", "shift", "hops", "acf_lo", "acf_mid", "acf_hi", "acf_zero", "sum")

_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_tempo_harness())
        l.zltp_isqrt.restype = C.c_uint64
        l.zltp_isqrt.argtypes = [C.c_uint64]
        l.zltp_resolve.restype = C.c_int32
        l.zltp_resolve.argtypes = [C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        l.zltp_result_bytes.restype = C.c_int32
        l.zltp_call.restype = C.c_int64
        l.zltp_call.argtypes = [C.c_int32] + [C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 4
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


# ---- the integer square root --------------------------------------------------------------------------------------------------------
def test_isqrt_is_exact_around_squares():
    l = lib()
    for centre in (2 ** 22, 2 ** 32, 2 ** 44):
        k0 = math.isqrt(centre)
        for k in list(range(k0 - 40, k0 + 41)) + [k0 * 2 - 1, k0 // 2 + 1]:
            for x in (k * k - 1, k * k, k * k + 1):
                assert l.zltp_isqrt(x) == math.isqrt(x) == tr.isqrt(x), x
    for x in (0, 1, 2, 3, 4, 2 ** 44 - 1, 2 ** 53 + 1, (2 ** 26 + 1) ** 2 - 1, 2 ** 62 - 1):
        assert l.zltp_isqrt(x) == math.isqrt(x), x
    rng = np.random.default_rng(1)
    for x in rng.integers(0, 2 ** 44, 2000):
        assert l.zltp_isqrt(int(x)) == math.isqrt(int(x))


# ---- the harness against the restatement --------------------------------------------------------------------------------------------
def call(requests, count_limit=8 << 20):
    """requests: (E uint64 [hops], rate, hop, bpm_min, bpm_max).  Runs the harness walk over the whole call and holds every request to
    the restatement; returns the records as dicts and the geometries"""
    n = len(requests)
    hops = np.array([len(r[0]) for r in requests], np.int32)
    rate = np.array([r[1] for r in requests], np.float64)
    hop = np.array([r[2] for r in requests], np.int32)
    lo = np.array([r[3] for r in requests], np.float32)
    hi = np.array([r[4] for r in requests], np.float32)
    E = np.concatenate([np.asarray(r[0], np.uint64) for r in requests])
    W = np.full(int(hops.sum()), 0xFFFF, np.uint16)
    capacity = int(sum(min(8200, h // 2 + 2) for h in hops))
    A = np.full(capacity + 1, 0xDEADBEEF, np.uint64)
    geom = np.zeros((n, 8), np.int32)
    out = (_abi.Tempo * n)()
    assert lib().zltp_result_bytes() == C.sizeof(_abi.Tempo) == 72
    refs = [tr.tempo_from_energy(r[0], r[1], r[2], r[3], r[4]) for r in requests]
    bufs = [np.zeros((len(ref[3]), int(h)), np.uint8) if 0 < len(ref[3]) * int(h) <= count_limit else None for ref, h in zip(refs, hops)]
    counts = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bufs])
    walk = np.zeros(3, np.int64)
    used = lib().zltp_call(n, hops.ctypes.data, rate.ctypes.data, hop.ctypes.data, lo.ctypes.data, hi.ctypes.data, E.ctypes.data, W.ctypes.data,
                           A.ctypes.data, capacity, geom.ctypes.data, C.addressof(out), C.addressof(counts), walk.ctypes.data)
    assert 0 <= used <= capacity and int(A[used]) == 0xDEADBEEF
    products, recs, at = 0, [], 0
    for i, (rec, rW, first, rA) in enumerate(refs):
        lmin, lmax, cap, first_lag, nlags, acf_base, items, nsegs = (int(v) for v in geom[i])
        assert (lmin, lmax, cap) == tuple(min(v, 10 ** 6) for v in tr.lags(float(rate[i]), int(hop[i]), float(lo[i]), float(hi[i]), int(hops[i])))
        assert nlags == len(rA) and (nlags == 0 or first_lag == first), (i, nlags, len(rA))
        assert items == -(-nlags // 256) * nsegs and nsegs == -(-int(hops[i]) // 4096)
        assert np.array_equal(W[at:at + hops[i]], rW), i
        assert [int(v) for v in A[acf_base:acf_base + nlags]] == rA, i
        got = {k: getattr(out[i], k) for k in INTS}
        assert got == {k: rec[k] for k in INTS}, (i, got, rec)
        assert np.float32(out[i].bpm) == rec["bpm"] and np.float32(out[i].confidence) == rec["confidence"], (i, out[i].bpm, rec)
        assert out[i].reserved == 0
        if bufs[i] is not None:
            want = np.zeros_like(bufs[i])
            for l in range(nlags):
                want[l, first_lag + l:] = 1
            assert np.array_equal(bufs[i], want), (i, "a product enters twice or not at all")
        products += sum(int(hops[i]) - (first_lag + l) for l in range(nlags))
        recs.append(dict(got, bpm=out[i].bpm, confidence=out[i].confidence))
        at += int(hops[i])
    assert [int(v) for v in walk] == [products, 0, 0], walk        # every product once; no index outside a request's W; the staged word is the lane's hop
    return recs, geom


def noise_energy(rng, hops, top):
    return rng.integers(0, top, hops).astype(np.uint64)


def pulses(rng, hops, period, high, low=4096):
    E = rng.integers(0, low, hops).astype(np.uint64)
    E[::period] = high + rng.integers(0, 1000, len(E[::period])).astype(np.uint64)
    return E


def test_random_energies_quiet_and_loud():
    rng = np.random.default_rng(2)
    recs, _ = call([(noise_energy(rng, 700, 10 ** 5), 48000.0, 256, 75.0, 150.0),
                    (noise_energy(rng, 700, 2 ** 44), 48000.0, 256, 75.0, 150.0),
                    (pulses(rng, 1500, 94, 2 ** 30), 48000.0, 256, 75.0, 150.0),
                    (pulses(rng, 1500, 94, 2 ** 43), 44100.0, 240, 60.0, 200.0)])
    assert recs[0]["shift"] == 0 and recs[1]["shift"] == 6 and recs[2]["shift"] == 0 and recs[3]["shift"] > 0
    assert recs[2]["lag_coarse"] == 94 and recs[2]["doublings"] == 2 and recs[2]["lag_fine"] == 376
    assert abs(recs[2]["bpm"] - 60 * 48000 / (256 * 94)) < 0.05 and recs[2]["confidence"] > 0.9


def test_hops_of_one_two_and_three_and_lags_at_both_ends():
    rng = np.random.default_rng(3)
    # 8 kHz, hop 4096, 20 .. 400 bpm: l_min = 1, l_max = 5 before the cut
    reqs = [(noise_energy(rng, h, 10 ** 6) + np.uint64(1), 8000.0, 4096, 20.0, 400.0) for h in (1, 2, 3, 4, 5, 6, 7, 12, 13)]
    recs, geom = call(reqs)
    assert [r["lag_fine"] for r in recs[:2]] == [0, 0] and [int(g[2]) for g in geom[:3]] == [0, 0, 1]
    assert all(r["acf_zero"] > 0 and r["sum"] > 0 for r in recs)   # no tempo keeps hops, shift, sum and acf_zero
    # hops 3: cap = 1, so m = 1: acf_lo is A[0] (m - 1 < l_min) and acf_hi is A[cap + 1]
    assert recs[2]["lag_fine"] == 1 and recs[2]["acf_lo"] == recs[2]["acf_zero"] and int(geom[2][3]) == 1 and int(geom[2][4]) == 2


def test_ties_go_to_the_smaller_lag():
    # W[h] = c for every hop: A[l] = (hops - l) c^2, so every lag ties with every other in the order
    c, hops = 10, 700
    E = np.array([(c * (h + 1)) ** 2 for h in range(hops)], np.uint64)
    recs, geom = call([(E, 48000.0, 256, 75.0, 150.0)])
    lmin = int(geom[0][0])
    assert recs[0]["lag_coarse"] == lmin == 75 and recs[0]["doublings"] == 2 and recs[0]["lag_fine"] == 4 * lmin - 3
    assert recs[0]["acf_mid"] == (hops - recs[0]["lag_fine"]) * c * c and recs[0]["confidence"] == 0.0
    # a period of exactly 100 hops of equal pulses: 100, 200 and 300 tie only where the counts allow; the restatement decides, the harness agrees
    E = np.zeros(801, np.uint64); E[::100] = 10 ** 8
    recs, _ = call([(E, 48000.0, 256, 75.0, 150.0)])
    assert recs[0]["lag_coarse"] == 100


def test_segment_and_lag_tile_edges():
    rng = np.random.default_rng(4)
    # 48 kHz, hop 256, defaults: first lag 74, cap + 1 binds: 255, 256 and 257 lags at 655, 657 and 659 hops
    recs, geom = call([(pulses(rng, h, 90, 2 ** 34), 48000.0, 256, 75.0, 150.0) for h in (655, 657, 659)])
    assert [int(g[4]) for g in geom] == [255, 256, 257] and [int(g[6]) for g in geom] == [1, 1, 2]
    # hop 64: segments of 4096 hops
    recs, geom = call([(pulses(rng, h, 377, 2 ** 30), 48000.0, 64, 75.0, 150.0) for h in (4095, 4096, 4097, 8192, 8193)], count_limit=40 << 20)
    assert [int(g[7]) for g in geom] == [1, 1, 2, 2, 3]
    assert all(r["lag_coarse"] == 377 for r in recs)


def test_a_call_with_silence_and_too_short_requests_between_the_others():
    rng = np.random.default_rng(5)
    reqs = [(np.zeros(2, np.uint64), 48000.0, 256, 75.0, 150.0),                  # too short, first
            (pulses(rng, 900, 80, 2 ** 36), 48000.0, 256, 75.0, 150.0),
            (np.zeros(900, np.uint64), 48000.0, 256, 75.0, 150.0),                # silence: lags evaluated, no tempo
            (noise_energy(rng, 90, 10 ** 6), 48000.0, 256, 75.0, 150.0),          # too short for the range: no lags
            (pulses(rng, 4200, 500, 2 ** 36), 48000.0, 64, 75.0, 150.0),
            (noise_energy(rng, 1, 10 ** 6), 48000.0, 256, 75.0, 150.0)]           # too short, last
    recs, geom = call(reqs)
    assert [r["lag_fine"] == 0 for r in recs] == [True, False, True, True, False, True]
    assert recs[2]["acf_zero"] == 0 and int(geom[2][4]) > 0 and int(geom[3][4]) == 0 and recs[3]["acf_zero"] > 0
    for r in (recs[0], recs[2], recs[3], recs[5]):
        assert r["bpm"] == 0.0 and r["confidence"] == 0.0 and r["lag_coarse"] == 0 and r["doublings"] == 0 and r["acf_mid"] == 0


def test_the_largest_request():
    # 65536 hops at hop 64 and l_max = 1024: 16 segments x 31 tiles of the lags 299 .. 8200
    rng = np.random.default_rng(6)
    E = pulses(rng, 65536, 700, 2 ** 38, low=2 ** 20)
    recs, geom = call([(E, 48000.0, 64, 43.945, 150.0)])
    assert int(geom[0][1]) == 1024 and int(geom[0][3]) + int(geom[0][4]) - 1 == 8200 and int(geom[0][6]) == 16 * 31
    assert recs[0]["lag_coarse"] == 700 and recs[0]["doublings"] == 3


# ---- the tie cases that reach the device as clips (tests/tempo_cases.py) --------------------------------------------------------------
def test_every_tie_case_hits_its_edge():
    """by the restatement alone: a case whose lags stop tying where it says fails here, without a GPU"""
    cases = tc.cases()
    for c in cases:
        tc.holds(c)
    names = " | ".join(c["name"] for c in cases)
    for kind in ("every lag ties", "neighbouring lanes", "all four waves", "successive passes", "doubling's triple"):
        assert kind in names, kind
    assert len(cases) == 5
    for c in tc.too_short():
        rec, W, first_lag, A = tc.want(c)
        assert A == [] and rec["lag_coarse"] == 0 and rec["lag_fine"] == 0 and rec["bpm"] == 0.0


def test_the_tie_cases_through_the_harness():
    """the whole list in one call of the host walk (the energies are the restatement's), requests without a lag first, last and twice
    in a row in the middle"""
    import onset_ref as onr
    cases, (s0, s1) = tc.cases(), tc.too_short()
    half = len(cases) // 2
    order = [s0] + cases[:half] + [s1, s0] + cases[half:] + [s1]
    recs, geom = call([(onr.energy(c["x"], c["req"][0], c["req"][1], c["req"][2]), c["rate"]) + c["req"][2:] for c in order], count_limit=40 << 20)
    for c, rec, g in zip(order, recs, geom):
        if "pred" in c:
            tc.literal(c, rec)
            assert (int(g[0]), int(g[1]), int(g[2])) == tc.lags_of(c)
        else:
            assert int(g[4]) == 0 and rec["lag_fine"] == 0


# ---- what the definition does to sound (the restatement alone) ----------------------------------------------------------------------
TEMPI = (76, 85, 90, 100, 110, 120, 128, 133.3, 140, 149)


@pytest.mark.parametrize("level", [1.0, 0.01], ids=["full", "minus40dB"])
@pytest.mark.parametrize("rate", [48000.0, 44100.0])
@pytest.mark.parametrize("pattern", [tr.pattern_a, tr.pattern_b], ids=["A", "B"])
def test_patterns_give_their_tempo(pattern, rate, level):
    """measured over these 80 cases: |bpm - true| <= 0.046, confidence >= 0.53"""
    for bpm in TEMPI:
        x = pattern(rate, 8.0, bpm) * np.float32(level)
        rec = tr.tempo(x, rate)[0]
        print(pattern.__name__, rate, level, bpm, float(rec["bpm"]), float(rec["confidence"]))
        assert abs(float(rec["bpm"]) - bpm) <= 0.25, (bpm, rec)
        assert rec["confidence"] >= 0.4, (bpm, rec)


@pytest.mark.parametrize("rate", [48000.0, 44100.0])
def test_white_noise_has_no_confidence(rate):
    x = np.random.default_rng(7).uniform(-0.5, 0.5, (1, int(8 * rate))).astype(np.float32)
    rec = tr.tempo(x, rate)[0]
    print(rate, float(rec["bpm"]), float(rec["confidence"]))
    assert rec["confidence"] <= 0.2


def test_silence_and_a_short_clip_give_no_tempo():
    for x in (np.zeros((1, 8 * 48000), np.float32), tr.pattern_a(48000.0, 0.5, 120)):
        rec = tr.tempo(x, 48000.0)[0]
        assert rec["bpm"] == 0.0 and rec["confidence"] == 0.0 and rec["lag_fine"] == 0 and rec["lag_coarse"] == 0 and rec["doublings"] == 0
        assert rec["hops"] == -(-x.shape[1] // 256)
    assert tr.tempo(np.zeros((1, 8 * 48000), np.float32), 48000.0)[0]["acf_zero"] == 0
    assert tr.tempo(tr.pattern_a(48000.0, 0.5, 120), 48000.0)[0]["acf_zero"] > 0


# ---- defaults and limits ------------------------------------------------------------------------------------------------------------
def resolve(sr, num_frames=1000, hop=0, bpm_min=0.0, bpm_max=0.0, first_frame=0):
    r = _abi.TempoRequest(0, first_frame, num_frames, hop, bpm_min, bpm_max)
    before = bytes(r)
    rc = zlhip().zlhip_tempo_resolve(sr, C.byref(r))
    want = tr.resolve(sr, num_frames, hop, bpm_min, bpm_max, first_frame)
    if rc != 0:
        assert rc == _abi.ZLHIP_ERR_INVALID and bytes(r) == before and want is None      # a refused request is left as it was
        return None
    got = dict(hop=r.hop_frames, bpm_min=r.bpm_min, bpm_max=r.bpm_max)
    assert got == want, (got, want)
    h, a, b = C.c_int32(hop), C.c_float(bpm_min), C.c_float(bpm_max)
    assert lib().zltp_resolve(sr, C.byref(h), C.byref(a), C.byref(b)) == 0 and (h.value, a.value, b.value) == (r.hop_frames, r.bpm_min, r.bpm_max)
    return got


def test_defaults():
    for sr, hop in {8000: 64, 44100: 240, 48000: 256, 96000: 512, 192000: 1024}.items():
        assert resolve(float(sr)) == dict(hop=hop, bpm_min=75.0, bpm_max=150.0)
    assert resolve(48000.0, hop=64, bpm_max=200.0) == dict(hop=64, bpm_min=75.0, bpm_max=200.0)
    assert resolve(48000.0, bpm_min=100.0) == dict(hop=256, bpm_min=100.0, bpm_max=150.0)
    # the rate is always needed: the lags come from it
    assert resolve(0.0, hop=64) is None and resolve(float("nan")) is None and resolve(-48000.0) is None


def test_every_limit_either_side():
    ok = dict(hop=256, bpm_min=75.0, bpm_max=150.0)
    for hop in (64, 80, 4080, 4096):
        assert resolve(48000.0, **dict(ok, hop=hop)) == dict(ok, hop=hop)
    for hop in (48, 63, 65, 72, 4097, 4112, -256):
        assert resolve(48000.0, **dict(ok, hop=hop)) is None
    assert resolve(48000.0, hop=256, bpm_min=20.0, bpm_max=400.0) == dict(hop=256, bpm_min=20.0, bpm_max=400.0)
    for lo, hi in ((19.99, 150.0), (75.0, 400.01), (150.0, 150.0), (150.0, 75.0), (-75.0, 150.0), (float("nan"), 150.0), (75.0, float("nan")),
                   (75.0, float("inf")), (float("-inf"), 150.0)):
        assert resolve(48000.0, hop=256, bpm_min=lo, bpm_max=hi) is None, (lo, hi)
    # l_max <= 1024 before the cut to cap: 60 * 48000 / (64 * bpm_min)
    assert resolve(48000.0, hop=64, bpm_min=43.945, bpm_max=150.0) is not None
    assert tr.lags(48000.0, 64, float(np.float32(43.945)), 150.0, 10 ** 6)[1] == 1024
    assert resolve(48000.0, hop=64, bpm_min=43.9, bpm_max=150.0) is None
    assert resolve(192000.0, hop=64, bpm_min=75.0, bpm_max=150.0) is None
    assert resolve(48000.0, num_frames=1, **ok) == ok and resolve(48000.0, num_frames=0, **ok) is None and resolve(48000.0, num_frames=-5, **ok) is None
    assert resolve(48000.0, first_frame=-1, **ok) is None
    small = dict(ok, hop=64)
    assert resolve(48000.0, num_frames=65536 * 64, **small) == small and resolve(48000.0, num_frames=65536 * 64 + 1, **small) is None
    assert zlhip().zlhip_tempo_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = _abi.TempoRequest(0, 0, 100, 0, 0.0, 0.0)
    out = (_abi.Tempo * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert z.zlhip_sound_tempo(None, C.byref(r), out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_tempo_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_tempo_acf(None, 0, None, None, 0, C.byref(n), C.byref(n), C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_tempo_timings(None, None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_tempo_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * 72 and n.value == -7


def test_tempo_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    rf = ["id", "first_frame", "num_frames", "hop_frames", "bpm_min", "bpm_max"]
    tf = [name for name, _ in _abi.Tempo._fields_]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){printf("%d %d",(int)sizeof(zlhip_tempo_request),(int)sizeof(zlhip_tempo));'
                    + "".join('printf(" %%d",(int)offsetof(zlhip_tempo_request,%s));' % f for f in rf)
                    + "".join('printf(" %%d",(int)offsetof(zlhip_tempo,%s));' % f for f in tf) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, T = _abi.TempoRequest, _abi.Tempo
    assert got == [C.sizeof(R), C.sizeof(T)] + [getattr(R, f).offset for f in rf] + [getattr(T, f).offset for f in tf]
    assert got == [24, 72, 0, 4, 8, 12, 16, 20, 0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]


def test_tempo_kernels_resources(built):
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_tempo_kernel_resources.txt")
    assert os.path.exists(path), "no zl_tempo kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    flux = [r for n, r in rows.items() if "zl_k_tempo_flux" in n]
    acf = [r for n, r in rows.items() if "zl_k_tempo_acf" in n]
    pick = [r for n, r in rows.items() if "zl_k_tempo_pick" in n]
    assert len(flux) == 1 and len(acf) == 1 and len(pick) == 1 and len(rows) == 3, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    # the segment's W[h] and the tile's lagged window as uint16: 2 * (4096 + 4096 + 256) bytes; nine workgroups of it fit a CU's 160 KB
    assert acf[0]["lds"] == 2 * (4096 + 4096 + 256), rows
    assert acf[0]["vgprs"] <= 64 and acf[0]["waves"] >= 8, rows
    assert flux[0]["lds"] <= 64 and pick[0]["lds"] <= 64, rows


# ---- the walk under the sanitizers --------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/tempo_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with
    AddressSanitizer and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the
    environment loads in front of it."""
    exe = str(tmp_path / "tempo_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tempo_check.cpp"), "-o", exe])
    for args in (["1", "6"], ["2", "6"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "tempo check ok" in rc.stdout
