"""Loop finder (zlhip_sound_loop_batch): one call over 64 stereo clips of 10 s at 48 kHz with the defaults (480 frames of search around
each point, a window of 256: 961 x 961 pairs per clip), median of 5 after a warm-up call, profiling on -- the device time of the pairs
kernel and of the rest (zlhip_debug_loop_timings), the host wall time of the call and the terms (one difference, one multiply-add) per
second of the pairs kernel.  In the same session and on the same clips:
    host       zlhip_sound_read of every clip plus a 16-thread host build of the same header (tests/cpu_harness/loop_host.cpp,
               zllp_run_planar), whose records must equal the device's
Prints one JSON line.

    python scripts/loop_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16] [--host-clips 8]
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
    """a sustained tone at a note of its own between MIDI 36 and 84: a stack of six harmonics under one slow decay, the channels' phases
    a little apart, over a quiet noise floor"""
    note = rng.uniform(36.0, 84.0)
    f = 440.0 * 2.0 ** ((note - 69.0) / 12.0)
    t = np.arange(n) / sr
    x = rng.uniform(-0.001, 0.001, (2, n))
    for c in range(2):
        for h in range(1, 7):
            x[c] += (0.3 / h) * np.sin(2.0 * np.pi * h * f * t + rng.uniform(0.0, 6.28)) * np.exp(-0.02 * t)
    return x.astype(np.float32), sr / f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-clips", type=int, default=8, help="clips the host route is timed on (its time is scaled to the bank)")
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()

    from libzl_amd import SamplerSynth, _abi, build
    n = int(a.seconds * a.sr)
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=a.clips + 8, sound_arena_bytes=(n + 16) * 8 * a.clips + (1 << 20))
    lib, e = syn._lib, syn._e
    rng = np.random.default_rng(a.seed)
    made = [clip(rng, n, a.sr) for _ in range(a.clips)]
    ids = [syn.register_clip(x[0], x[1], a.sr) for x, _ in made]
    syn.set_profiling(True)
    s0, e0 = int(0.25 * n), int(0.75 * n) + 57                     # a sustain loop over the middle half of every clip
    q = _abi.LoopRequest(0, s0, e0, 0, 0, 0, 0)
    assert lib.zlhip_loop_resolve(a.sr, C.byref(q)) == 0
    reqs = [(cid, s0, e0) for cid in ids]

    pairs_ms, rest_ms, wall = [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the call's buffers)
        t0 = time.perf_counter()
        got = syn.clip_loop_batch(reqs)
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            t = syn.loop_timings()
            pairs_ms.append(t[0]); rest_ms.append(t[1])
    terms = sum(g["starts"] * g["ends"] for g in got) * q.window
    pm = float(np.median(pairs_ms))
    periods = [(g["stop_frame"] - g["start_frame"]) / p for g, (_, p) in zip(got, made)]
    res = dict(metric="sound_loop", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, reps=a.reps,
               request=dict(start_search=q.start_search, stop_search=q.stop_search, window=q.window, min_length=q.min_length),
               pairs=sum(g["pairs"] for g in got), work_items=sum(-(-g["starts"] // 64) * -(-g["ends"] // 64) for g in got), terms=terms,
               pairs_ms=pm, rest_ms=float(np.median(rest_ms)), call_ms=float(np.median(wall)), pairs_ms_all=pairs_ms, rest_ms_all=rest_ms, call_ms_all=wall,
               pairs_Gterms=terms / (pm * 1e-3) / 1e9,
               host_bytes=80 * a.clips, found=sum(g["found"] for g in got), worst_period_error=float(max(abs(v - round(v)) for v in periods)),
               min_improvement_db=float(min(g["improvement_db"] for g in got)), max_seam_db=float(max(g["seam_db"] for g in got)))

    # the route without the call: the clip over PCIe (zlhip_sound_read), then the same header on the host
    h = C.CDLL(build.build_loop_harness())
    h.zllp_run_planar.restype = C.c_int32
    h.zllp_run_planar.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(_abi.LoopRequest), C.c_double, C.c_int32, C.POINTER(_abi.Loop)]
    L = np.empty(n, np.float32); R = np.empty(n, np.float32); ln = C.c_int32(0)
    out = _abi.Loop()
    hq = _abi.LoopRequest(0, s0, e0, 0, 0, 0, 0)
    hc = max(1, min(a.host_clips, a.clips))

    def host():
        t0 = time.perf_counter(); t_read = 0.0
        for i, cid in enumerate(ids[:hc]):
            t1 = time.perf_counter()
            assert lib.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data, n, C.byref(ln)) == 2
            t_read += time.perf_counter() - t1
            assert h.zllp_run_planar(L.ctypes.data, R.ctypes.data, n, C.byref(hq), a.sr, a.threads, C.byref(out)) == 0
            assert all(getattr(out, k) == got[i][k] for k in got[i]), i      # the figures are of two routes that compute the same thing
        return (time.perf_counter() - t0) * 1e3, t_read * 1e3
    host()
    runs = [host() for _ in range(3)]
    total = float(np.median([r[0] for r in runs])) * a.clips / hc
    res["host"] = dict(route="zlhip_sound_read + zl_loop.h on the host", host_threads=a.threads, clips_timed=hc, total_ms=total,
                       read_ms=float(np.median([r[1] for r in runs])) * a.clips / hc, total_ms_all=[r[0] * a.clips / hc for r in runs],
                       Gterms=terms / (total * 1e-3) / 1e9, ratio_to_call=total / res["call_ms"])
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
