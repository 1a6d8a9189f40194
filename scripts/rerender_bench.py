"""Clip re-render throughput: one zlhip_sound_rerender_batch call of 64 stereo clips x 10 s at 48 kHz (speed 1.25, pitch +3), device
time of the seek and the synthesis launch (HIP events, zlhip_set_profiling) and the wall time of the call; next to it the host build
of the same text (tests/cpu_harness/stretch_host.cpp, built by libzl_amd/build.py) on 16 threads.  Prints one JSON line.

    python scripts/rerender_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16] [--no-host]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--speed", type=float, default=1.25)
    ap.add_argument("--pitch", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    from libzl_amd import SamplerSynth
    n = int(a.seconds * a.sr)
    rng = np.random.default_rng(1)
    t = np.arange(n) / a.sr
    srcs = [(0.5 * np.sin(2 * np.pi * (220.0 + 10 * i) * t)[None, :] + rng.uniform(-0.3, 0.3, (2, n))).astype(np.float32) for i in range(a.clips)]
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=max(8, a.clips), sound_arena_bytes=4 * n * 2 * a.clips * 3)
    ids = [syn.register_clip(s[0], s[1], a.sr) for s in srcs]
    syn.set_profiling(True)
    syn.rerender_clips(ids, 0.0, a.pitch, a.speed)                 # warm-up (code objects, buffers)
    seek, synth, wall = [], [], []
    for r in range(a.reps):
        # alternate two gains so that every call renders (identity would not)
        g = 0.0 if r % 2 else -1.0
        t0 = time.perf_counter()
        syn.rerender_clips(ids, g, a.pitch, a.speed)
        wall.append((time.perf_counter() - t0) * 1e3)
        s, y = syn.rerender_timings()
        seek.append(s); synth.append(y)
    out_frames = len(syn.read_clip(ids[0])[0])
    res = dict(metric="rerender_batch", clips=a.clips, seconds=a.seconds, sr=a.sr, speed=a.speed, pitch=a.pitch, device=syn.device_name(),
               seek_ms_median=float(np.median(seek)), synth_ms_median=float(np.median(synth)), call_ms_median=float(np.median(wall)),
               seek_ms=seek, synth_ms=synth, call_ms=wall, out_frames_per_clip=out_frames)
    syn.close()
    if not a.no_host:
        lib = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "_build", "libzl_stretch_host.so"))
        lib.zlst_render_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_int64, C.c_double, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int]
        inter = np.stack([np.stack([s[0], s[1]], axis=1).reshape(-1) for s in srcs])
        out = np.zeros((a.clips, out_frames * 2), np.float32)
        host = []
        for r in range(2):
            t0 = time.perf_counter()
            assert lib.zlst_render_batch(inter.ctypes.data, a.clips, 2, n, a.sr, -1.0, a.pitch, a.speed, out.ctypes.data, a.threads) == 0
            host.append((time.perf_counter() - t0) * 1e3)
        res.update(host_threads=a.threads, host_ms=host, host_ms_min=min(host))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
