"""Loudness measurement, CPU tier: the numpy restatement (tests/loudness_ref.py) against ITU-R BS.1770's tables and a plain serial
scipy.signal.lfilter BS.1770, and the host build of the product's header (tests/cpu_harness/loudness_host.cpp over
libzl_amd/csrc/zl_loudness.h, walked item by item as the kernel walks a call) against the restatement, bit for bit."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import loudness_ref as lr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SUBREC = np.dtype([("sum", np.float64, 2), ("peak", f32, 2)])
_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_loudness_harness())
        l.zlld_design.restype = C.c_int
        l.zlld_design.argtypes = [C.c_double, C.c_void_p]
        l.zlld_call.restype = C.c_int64
        l.zlld_call.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        l.zlld_bank.restype = C.c_int64
        l.zlld_bank.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def coeffs(rate):
    c = (C.c_double * 10)()
    assert zlhip().zlhip_loudness_design(rate, c) == 0
    return list(c)


# ---- the design ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000.0, 22050.0, 44100.0, 48000.0, 88200.0, 96000.0, 192000.0])
def test_the_restatements_design_equals_the_librarys(rate):
    got, want = coeffs(rate), lr.design(rate)
    assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, want)), (got, want)
    h = (C.c_double * 10)()
    assert lib().zlld_design(rate, h) == 0 and list(h) == got      # the harness and the library: one header
    assert got[5:8] == [1.0, -2.0, 1.0]


def test_the_design_reproduces_bs1770s_tables_at_48k():
    d = lr.design(48000.0)
    mine = (d[0], d[1], d[2], d[3], d[4], d[8], d[9])
    worst = max(abs(a - b) for a, b in zip(mine, lr.BS1770_48K))
    print("largest difference from the tables:", worst)
    assert worst <= 1e-12
    z = zlhip()
    assert z.zlhip_loudness_design(0.0, (C.c_double * 10)()) == _abi.ZLHIP_ERR_INVALID and z.zlhip_loudness_design(float("nan"), (C.c_double * 10)()) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_loudness_design(48000.0, None) == _abi.ZLHIP_ERR_INVALID


# ---- the restatement against a plain serial BS.1770 ------------------------------------------------------------------------------------
def serial_bs1770(src, rate):
    """ITU-R BS.1770-4 with one filter pass over the whole signal: (lufs, blocks, above_relative)"""
    from scipy.signal import lfilter
    c = lr.design(rate)
    y = lfilter(c[5:8], [1.0, c[8], c[9]], lfilter(c[0:3], [1.0, c[3], c[4]], src.astype(np.float64), axis=1), axis=1)
    sub = lr.default_sub(rate)
    S = src.shape[1] // sub
    u = (y[:, :S * sub] ** 2).reshape(src.shape[0], S, sub).sum(2).sum(0)
    z = np.array([u[j:j + 4].sum() / (4 * sub) for j in range(S - 3)])
    a = z[z > lr.GATE_ABS]
    b = z[(z > lr.GATE_ABS) & (z > a.mean() / 10.0)]
    return -0.691 + 10.0 * math.log10(b.mean()), len(z), len(b)


def sine(rate, seconds, hz, dbfs, channels=1):
    t = np.arange(int(rate * seconds))
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * hz * t / rate)).astype(f32)[None, :].repeat(channels, 0)


CASES = {
    "stereo 1 kHz at -23 dBFS, 20 s": (lambda r: sine(r, 20, 1000.0, -23.0, 2), -23.0),
    "-36 / -23 / -36 dBFS, 10 / 60 / 10 s": (lambda r: np.concatenate([sine(r, 10, 1000.0, -36.0, 2), sine(r, 60, 1000.0, -23.0, 2), sine(r, 10, 1000.0, -36.0, 2)], 1), -23.0),
    "mono 997 Hz at 0 dBFS": (lambda r: sine(r, 5, 997.0, 0.0), -3.01),
    "30 Hz plus DC": (lambda r: (sine(r, 5, 30.0, -6.0) + f32(0.25)).astype(f32), None),
}


@pytest.mark.parametrize("rate", [44100.0, 48000.0, 96000.0])
@pytest.mark.parametrize("case", list(CASES))
def test_the_restatement_equals_a_serial_bs1770(case, rate):
    make, expect = CASES[case]
    src = make(rate)
    got = lr.measure(src, rate)[0]
    lufs, blocks, passed = serial_bs1770(src, rate)
    print(case, rate, "restatement", got["lufs"], "serial", lufs, "difference", got["lufs"] - lufs)
    assert abs(got["lufs"] - lufs) <= 1e-6
    assert (got["blocks"], got["above_relative"]) == (blocks, passed)
    if expect is not None:
        assert abs(got["lufs"] - expect) <= 0.1                    # EBU Tech 3341's own tolerance
    if case.startswith("-36") and rate == 48000.0:
        assert blocks == 797 and blocks - passed == 194            # the relative gate drops the quiet ends


# ---- the harness (the product's header, walked as the kernel walks a call) against the restatement ------------------------------------------
def clip(ch, length, seed, level=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    return (level * (np.stack([np.sin(2 * np.pi * t / 48.3 + 0.7 * c) for c in range(ch)]) + 0.2 * rng.standard_normal((ch, length)))).astype(f32)


def call(requests):
    """requests: (src planar, rate, first, num, sub) -> (items, results as dicts, per request (sums, peaks), walk)"""
    n = len(requests)
    inter = [np.ascontiguousarray(r[0].T).ravel() for r in requests]           # the arena's layout, exactly length * channels floats
    reqs = (_abi.LoudnessRequest * n)(*[_abi.LoudnessRequest(0, r[2], r[3], r[4]) for r in requests])
    data = (C.c_void_p * n)(*[x.ctypes.data for x in inter])
    length = (C.c_int32 * n)(*[r[0].shape[1] for r in requests])
    chans = (C.c_int32 * n)(*[r[0].shape[0] for r in requests])
    rate = (C.c_double * n)(*[r[1] for r in requests])
    cap = sum(lr.items_of(r[3], lr.resolve(r[1], r[2], r[3], r[4])) for r in requests)
    subs = np.zeros(cap + 1, SUBREC)
    subs["sum"][cap] = -1.0                                        # a sentinel behind the call's records
    base = (C.c_int32 * n)()
    out = (_abi.Loudness * n)()
    walk = (C.c_int64 * 6)()
    items = lib().zlld_call(n, reqs, data, length, chans, rate, subs.ctypes.data, cap, base, out, walk)
    assert items == cap and subs["sum"][cap, 0] == -1.0
    res = [{k: (tuple(out[i].peak) if k == "peak" else getattr(out[i], k)) for k, _ in _abi.Loudness._fields_} for i in range(n)]
    recs = [(subs["sum"][base[i]:(base[i + 1] if i + 1 < n else cap)], subs["peak"][base[i]:(base[i + 1] if i + 1 < n else cap)]) for i in range(n)]
    return items, res, recs, list(walk)


def check(requests):
    items, res, recs, walk = call(requests)
    wants = lr.measure_batch([(r[0], r[1], r[2], r[3], r[4], coeffs(r[1])) for r in requests])
    for r, got, (gs, gp), (want, sums, peaks) in zip(requests, res, recs, wants):
        assert np.array_equal(gs.view(np.uint64), sums.view(np.uint64)) and np.array_equal(gp.view(np.uint32), peaks.view(np.uint32)), r[1:]
        assert lr.same(got, want), (r[1:], got, want)
    summed = 0
    for r in requests:
        sub = lr.resolve(r[1], r[2], r[3], r[4])
        S = r[3] // sub
        summed += (S * sub if S >= 4 else r[3]) * r[0].shape[0]
    # every frame a request sums is summed exactly once, no float outside a request is used, every lane runs exactly its own steps
    assert walk[0] == summed and walk[1] == 0 and walk[2] == 0 and walk[3] == 0 and walk[5] == -(-items // 64), walk
    return res, walk


def test_the_harness_equals_the_restatement_over_the_grid():
    """mono and stereo; first frame 1, 3, 5; sub-blocks 64, 100 and the default; S = 1, 2, 3 (the short rule), 4, 5, 9; remainder 0 and 37"""
    for ch in (1, 2):
        src = clip(ch, 47000, 10 + ch)
        reqs = [(src, 48000.0, first, S * (sub or 4800) + rem, sub) for sub in (64, 100, 0) for first in (1, 3, 5) for S in (1, 2, 3, 4, 5, 9) for rem in (0, 37)]
        res, _ = check(reqs)
        assert [(o["sub_blocks"], o["blocks"]) for o in res[:12]] == [(1, 1), (2, 1), (2, 1), (3, 1), (3, 1), (4, 1), (4, 1), (4, 1), (5, 2), (5, 2), (9, 6), (9, 6)]


def test_a_mixed_call_shares_groups_between_different_trip_counts():
    rng = np.random.default_rng(7)
    srcs = [(clip(1 + i % 2, int(rng.integers(5000, 9000)), 100 + i, float(rng.uniform(0.01, 0.9))), (44100.0, 48000.0)[(i // 2) % 2]) for i in range(6)]
    reqs = []
    for i in range(90):
        src, rate = srcs[i % 6]
        length = src.shape[1]
        sub = int(rng.choice([16, 17, 64, 100, 441, 0]))
        first = int(rng.integers(0, length // 4))
        n = 1 if i % 5 == 0 else int(rng.integers(1, length - first + 1))
        reqs.append((src, rate, first, n, sub))
    res, walk = check(reqs)
    assert walk[4] > 0 and walk[5] >= 10                           # lanes idled while their group's longest item went on
    assert sum(o["sub_blocks"] == 1 for o in res) >= 18


def test_special_values_and_no_loudness():
    rng = np.random.default_rng(3)
    special = np.array([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF,
                        0x3F800000, 0xBF800000, 0x3DCCCCCD, 0xBDCCCCCD], np.uint32)
    for ch in (1, 2):
        mixed = rng.permutation(np.tile(special, 400))[:3000 * ch].reshape(ch, -1).view(f32).copy()
        tiny = np.full((ch, 3000), 1e-40, f32)
        res, _ = check([(mixed, 48000.0, 1, 2990, 100), (tiny, 48000.0, 3, 2990, 100), (np.zeros((ch, 3000), f32), 48000.0, 0, 3000, 0), (clip(ch, 3000, 1, 1e-5), 48000.0, 0, 3000, 64)])
        assert math.isfinite(res[0]["lufs"]) and max(res[0]["peak"]) == 1.0
        for o in res[1:]:
            assert o["lufs"] == -math.inf and o["above_absolute"] == 0 and o["mean_square"] == 0.0 and o["relative_gate"] == 0.0
        assert res[1]["peak"][0] == float(f32(1e-40)) and res[2]["peak"] == (0.0, 0.0)


def test_the_host_route_equals_the_walk():
    srcs = [clip(1 + i % 2, 30000 + 777 * i, 60 + i) for i in range(5)]
    n = len(srcs)
    L = (C.c_void_p * n)(*[s[0].ctypes.data for s in srcs])
    R = (C.c_void_p * n)(*[s[1].ctypes.data if s.shape[0] == 2 else None for s in srcs])
    length = (C.c_int32 * n)(*[s.shape[1] for s in srcs])
    rate = (C.c_double * n)(*[48000.0] * n)
    subs = np.zeros(64, SUBREC)
    base = (C.c_int64 * n)()
    out = (_abi.Loudness * n)()
    items = lib().zlld_bank(n, L, R, length, rate, 3, subs.ctypes.data, 64, base, out)
    _, res, recs, _ = call([(s, 48000.0, 0, s.shape[1], 0) for s in srcs])
    assert items == sum(len(r[0]) for r in recs)
    for i in range(n):
        assert np.array_equal(subs["sum"][base[i]:base[i] + len(recs[i][0])], recs[i][0]) and out[i].mean_square == res[i]["mean_square"] and out[i].lufs == res[i]["lufs"]


# ---- defaults, limits, layouts --------------------------------------------------------------------------------------------------------
def resolve(rate, first, num, sub):
    r = _abi.LoudnessRequest(0, first, num, sub)
    rc = zlhip().zlhip_loudness_resolve(rate, C.byref(r))
    if rc != 0:
        assert rc == _abi.ZLHIP_ERR_INVALID and (r.first_frame, r.num_frames, r.sub_frames) == (first, num, sub)      # a refused request is left as it was
        return None
    return r.sub_frames


def test_defaults_and_every_limit_either_side():
    assert [resolve(r, 0, 1000, 0) for r in (8000.0, 44100.0, 48000.0, 96000.0, 11025.0, 22050.0)] == [800, 4410, 4800, 9600, 1103, 2205]
    assert all(resolve(r, 0, 1000, 0) == lr.resolve(r, 0, 1000, 0) for r in (8000.0, 11025.0, 44100.0, 47999.0, 192000.0))
    assert resolve(48000.0, 0, 1, 0) == 4800 and resolve(48000.0, 0, 0, 0) is None and resolve(48000.0, 0, -1, 0) is None
    assert resolve(48000.0, -1, 10, 0) is None and resolve(48000.0, 2 ** 31 - 11, 10, 0) == 4800
    assert resolve(48000.0, 0, 100, 16) == 16 and resolve(48000.0, 0, 100, 15) is None and resolve(48000.0, 0, 100, -16) is None
    assert resolve(48000.0, 0, 100, 131072) == 131072 and resolve(48000.0, 0, 100, 131073) is None
    assert resolve(48000.0, 0, 16 * 65536 + 15, 16) == 16 and resolve(48000.0, 0, 16 * 65537, 16) is None           # 65536 sub-blocks, 65537
    assert resolve(154.0, 0, 100, 0) is None and resolve(155.0, 0, 100, 0) == 16                                   # the default's own limits
    assert resolve(1310724.0, 0, 100, 0) == 131072 and resolve(1310726.0, 0, 100, 0) is None
    assert resolve(0.0, 0, 100, 64) is None and resolve(float("nan"), 0, 100, 64) is None and resolve(float("inf"), 0, 100, 64) is None
    assert zlhip().zlhip_loudness_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID
    # the short rule's items
    assert [lr.items_of(n, 100) for n in (1, 100, 101, 399, 400, 437, 499, 500)] == [1, 1, 2, 4, 4, 4, 4, 5]


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = _abi.LoudnessRequest(0, 0, 1000, 0)
    out = (_abi.Loudness * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert z.zlhip_sound_loudness(None, C.byref(r), out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_loudness_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_loudness_subs(None, 0, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_loudness_timings(None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_loudness_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * 48 and n.value == -7
    lz = C.CDLL(build.build_engine())
    for name, args in (("libzl_hotpath_clip_loudness", [C.c_void_p, C.c_void_p, C.c_void_p]), ("libzl_hotpath_clip_normalize", [C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
                       ("libzl_hotpath_clips_level", [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p])):
        getattr(lz, name).restype = C.c_int
        getattr(lz, name).argtypes = args
    assert lz.libzl_hotpath_clip_loudness(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clip_normalize(None, -16.0, -1.0, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clips_level(None, 2, -16.0, -1.0, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clips_level(None, -1, -16.0, -1.0, None) == _abi.ZLHIP_ERR_INVALID


def test_loudness_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_loudness_request", _abi.LoudnessRequest), ("zlhip_loudness", _abi.Loudness), ("zlhip_loudness_sub", _abi.LoudnessSub))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:3] == [16, 48, 24]
    assert got[3:] == [0, 4, 8, 12] + [0, 8, 16, 24, 32, 36, 40, 44] + [0, 16]
    assert SUBREC.itemsize == 24


def test_loudness_kernel_resources(built):
    """one kernel, no scratch memory, no spills, no LDS; 112 VGPRs (four waves per SIMD) as this is written"""
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_loudness_kernel_resources.txt")
    assert os.path.exists(path), "no zl_loudness kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    assert len(rows) == 1 and "zl_k_loudness" in next(iter(rows)), rows
    r = next(iter(rows.values()))
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, rows
    assert r["vgprs"] <= 128 and r["waves"] >= 4, rows


# ---- the walk under the sanitizers --------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/loudness_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with
    AddressSanitizer and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the
    environment loads in front of it."""
    exe = str(tmp_path / "loudness_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-pthread", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loudness_check.cpp"), "-o", exe])
    for args in (["1", "10"], ["2", "10"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "loudness check ok" in rc.stdout
