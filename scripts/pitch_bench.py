"""Pitch detection (zlhip_sound_pitch_batch): one call over 64 stereo clips of 10 s at 48 kHz with the defaults (64 frames per clip),
median of 5 after a warm-up call, profiling on -- the device time of the difference-function kernel and of the rest
(zlhip_debug_pitch_timings), the host wall time of the call and the integer multiply-adds per second of the difference-function kernel.
In the same session and on the same clips:
    host       zlhip_sound_read of every clip plus a 16-thread host build of the same header (tests/cpu_harness/pitch_host.cpp,
               zlpt_run_planar), whose records must equal the device's
Prints one JSON line.

    python scripts/pitch_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clip(rng, n, sr):
    """a pitched one-shot at a note of its own between MIDI 36 and 84: a decaying stack of eight harmonics, a little detuned between the
    channels' phases, over a quiet noise floor"""
    note = rng.uniform(36.0, 84.0)
    f = 440.0 * 2.0 ** ((note - 69.0) / 12.0)
    t = np.arange(n) / sr
    x = rng.uniform(-0.002, 0.002, (2, n))
    for c in range(2):
        for h in range(1, 9):
            x[c] += (0.4 / h) * np.sin(2.0 * np.pi * h * f * t + rng.uniform(0.0, 6.28)) * np.exp(-0.25 * h * t)
    return x.astype(np.float32), note


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
    ids = [syn.register_clip(x[0], x[1], a.sr) for x, _ in made]
    syn.set_profiling(True)
    q = _abi.PitchRequest(0, 0, n, 0, 0, 0.0, 0.0, 0, 0)
    assert lib.zlhip_pitch_resolve(a.sr, C.byref(q)) == 0
    tmax = math.floor(a.sr / q.f_min)

    diff, rest, wall = [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the call's buffers)
        t0 = time.perf_counter()
        got = syn.clip_pitch_batch([(cid,) for cid in ids])
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            t = syn.pitch_timings()
            diff.append(t[0]); rest.append(t[1])
    dm, rm = float(np.median(diff)), float(np.median(rest))
    frames = sum(g["frames"] for g in got)
    terms = frames * (tmax + 1) * q.window                         # one subtraction and one multiply-add each
    span_bytes = frames * (q.window + tmax + 1) * 8
    cents = [100.0 * abs(g["note"] - note) for g, (_, note) in zip(got, made)]
    res = dict(metric="sound_pitch", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, reps=a.reps,
               request=dict(window=q.window, max_frames=q.max_frames, f_min=q.f_min, f_max=q.f_max, threshold=q.threshold, gate=q.gate), t_max=tmax,
               frames=frames, lags=frames * (tmax + 1), work_items=frames * -(-(tmax + 1) // 256), terms=terms, span_bytes=span_bytes,
               diff_ms=dm, rest_ms=rm, call_ms=float(np.median(wall)), diff_ms_all=diff, rest_ms_all=rest, call_ms_all=wall,
               diff_Gmacs=terms / (dm * 1e-3) / 1e9, host_bytes=80 * a.clips, worst_cents_error=float(max(cents)),
               wrong_root_notes=int(sum(g["root_note"] != int(np.rint(note)) for g, (_, note) in zip(got, made))),
               min_confidence=float(min(g["confidence"] for g in got)))

    # the route without the call: every clip over PCIe (zlhip_sound_read), then the same header on the host
    h = C.CDLL(build.build_pitch_harness())
    h.zlpt_run_planar.restype = C.c_int32
    h.zlpt_run_planar.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.PitchRequest), C.c_double, C.c_int32, C.c_void_p, C.POINTER(_abi.Pitch)]
    L = np.empty(n, np.float32); R = np.empty(n, np.float32); ln = C.c_int32(0)
    out = _abi.Pitch()
    hq = _abi.PitchRequest(0, 0, n, 0, 0, 0.0, 0.0, 0, 0)

    def host():
        t0 = time.perf_counter(); t_read = 0.0
        for i, cid in enumerate(ids):
            t1 = time.perf_counter()
            assert lib.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data, n, C.byref(ln)) == 2
            t_read += time.perf_counter() - t1
            assert h.zlpt_run_planar(L.ctypes.data, R.ctypes.data, C.byref(hq), a.sr, a.threads, None, C.byref(out)) == 0
            assert all(getattr(out, k) == got[i][k] for k in got[i]), i      # the figures are of two routes that compute the same thing
        return (time.perf_counter() - t0) * 1e3, t_read * 1e3
    host()
    runs = [host() for _ in range(3)]
    total = float(np.median([r[0] for r in runs]))
    res["host"] = dict(route="zlhip_sound_read + zl_pitch.h on the host", host_threads=a.threads, total_ms=total,
                       read_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs], ratio_to_call=total / res["call_ms"])
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
