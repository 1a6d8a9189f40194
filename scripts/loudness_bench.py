"""Loudness measurement (zlhip_sound_loudness_batch): one call over 64 stereo clips of 10 s at 48 kHz with the default sub-block
(4800 frames: 100 sub-blocks per clip), median of 5 after a warm-up call, profiling on -- the device time of the kernel
(zlhip_debug_loudness_timings), the host wall time of the call, and the biquad samples per second of the kernel (a sample of one
channel through both biquads and the square; the warm-up sub-block makes them about twice the clip's).
In the same session and on the same clips:
    host       zlhip_sound_read of every clip plus a 16-thread host build of the same header (tests/cpu_harness/loudness_host.cpp,
               zlld_bank), whose records must equal the device's
Prints one JSON line.

    python scripts/loudness_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clip(rng, n, sr):
    """a clip at a level of its own between -40 and -6 dBFS: a decaying tone over brown noise, the channels differ"""
    level = 10.0 ** (rng.uniform(-40.0, -6.0) / 20.0)
    t = np.arange(n) / sr
    f = rng.uniform(60.0, 2000.0)
    x = np.cumsum(rng.standard_normal((2, n)), 1)
    x = 0.2 * x / np.abs(x).max(1, keepdims=True)
    for c in range(2):
        x[c] += 0.8 * np.sin(2.0 * np.pi * f * t + rng.uniform(0.0, 6.28)) * np.exp(-0.3 * t)
    return (level * x).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()

    from libzl_amd import SamplerSynth, _abi, build
    n = int(a.seconds * a.sr)
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=a.clips + 8, sound_arena_bytes=(n + 16) * 8 * a.clips + (1 << 20))
    lib, e = syn._lib, syn._e
    rng = np.random.default_rng(a.seed)
    made = [clip(rng, n, a.sr) for _ in range(a.clips)]
    ids = [syn.register_clip(x[0], x[1], a.sr) for x in made]
    syn.set_profiling(True)
    q = _abi.LoudnessRequest(0, 0, n, 0)
    assert lib.zlhip_loudness_resolve(a.sr, C.byref(q)) == 0
    sub = q.sub_frames

    kern, wall = [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the call's buffers)
        t0 = time.perf_counter()
        got = syn.clip_loudness_batch([(cid,) for cid in ids])
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            kern.append(syn.loudness_timings())
    km = float(np.median(kern))
    items = sum(g["sub_blocks"] for g in got)
    walked = sum(2 * ((g["sub_blocks"] * 2 - 1) * sub + (n - n // sub * sub)) for g in got)      # channel samples filtered, warm-up included
    recs = [syn.loudness_subs(i) for i in range(a.clips)]
    res = dict(metric="sound_loudness", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, reps=a.reps, sub_frames=sub,
               items=items, lanes=-(-items // 64) * 64, steps_per_lane=sub, clip_bytes=a.clips * n * 8, samples_filtered=walked,
               kernel_ms=km, call_ms=float(np.median(wall)), kernel_ms_all=kern, call_ms_all=wall,
               kernel_Gsamples=walked / (km * 1e-3) / 1e9, kernel_read_GBs=walked * 4 / (km * 1e-3) / 1e9, host_bytes=24 * items,
               lufs_min=float(min(g["lufs"] for g in got)), lufs_max=float(max(g["lufs"] for g in got)))

    # the route without the call: every clip over PCIe (zlhip_sound_read), then the same header on the host
    h = C.CDLL(build.build_loudness_harness())
    h.zlld_bank.restype = C.c_int64
    h.zlld_bank.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    Ls = [np.empty(n, np.float32) for _ in ids]; Rs = [np.empty(n, np.float32) for _ in ids]; ln = C.c_int32(0)
    Lp = (C.c_void_p * a.clips)(*[x.ctypes.data for x in Ls]); Rp = (C.c_void_p * a.clips)(*[x.ctypes.data for x in Rs])
    lens = (C.c_int32 * a.clips)(*[n] * a.clips); rates = (C.c_double * a.clips)(*[a.sr] * a.clips)
    subs = np.zeros(items, np.dtype([("sum", np.float64, 2), ("peak", np.float32, 2)]))
    base = (C.c_int64 * a.clips)()
    out = (_abi.Loudness * a.clips)()

    def host():
        t0 = time.perf_counter()
        for i, cid in enumerate(ids):
            assert lib.zlhip_sound_read(e, cid, Ls[i].ctypes.data, Rs[i].ctypes.data, n, C.byref(ln)) == 2
        t_read = time.perf_counter() - t0
        assert h.zlld_bank(a.clips, Lp, Rp, lens, rates, a.threads, subs.ctypes.data, items, base, out) == items
        return (time.perf_counter() - t0) * 1e3, t_read * 1e3
    host()
    runs = [host() for _ in range(3)]
    for i in range(a.clips):                                       # the figures are of two routes that compute the same thing
        m = got[i]["sub_blocks"]
        assert np.array_equal(subs["sum"][base[i]:base[i] + m], recs[i][0]) and np.array_equal(subs["peak"][base[i]:base[i] + m], recs[i][1]), i
        assert out[i].mean_square == got[i]["mean_square"] and out[i].above_relative == got[i]["above_relative"] and abs(out[i].lufs - got[i]["lufs"]) <= 1e-9, i
    total = float(np.median([r[0] for r in runs]))
    res["host"] = dict(route="zlhip_sound_read + zl_loudness.h on the host", host_threads=a.threads, total_ms=total,
                       read_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs], ratio_to_call=total / res["call_ms"],
                       records_equal=True)
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
