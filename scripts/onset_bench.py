"""Transient detection (zlhip_sound_onsets_batch): one call over 64 stereo clips of 10 s at 48 kHz with the defaults, median of 5 after
a warm-up call, profiling on -- the device time of the energy pass and of the rest (zlhip_debug_onset_timings), the host wall time of
the call and the GB/s of clip bytes the energy pass reads.  In the same session and on the same clips:
    overview   zlhip_sound_overview_batch with one column per hop (a column is one piece: the same bytes in the same 16-byte groups,
               one wavefront per 256 frames), its device time (zlhip_debug_overview_timings: the memset, the reduce and the finish)
    host       zlhip_sound_read of every clip plus a 16-thread host build of the same header (tests/cpu_harness/onset_host.cpp,
               zlon_run_planar), whose onsets must equal the device's
Prints one JSON line.

    python scripts/onset_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16]
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
    """a drum-loop-like clip: decaying noise hits every 0.2 - 0.6 s over a quiet noise floor"""
    x = rng.uniform(-0.003, 0.003, (2, n))
    at = 0
    while at < n:
        m = min(n - at, int(0.15 * sr))
        x[:, at:at + m] += rng.uniform(-0.6, 0.6, (2, m)) * np.exp(-np.arange(m) / (0.02 * sr))
        at += int(rng.uniform(0.2, 0.6) * sr)
    return x.astype(np.float32)


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
    ids = [syn.register_clip(*clip(rng, n, a.sr), a.sr) for _ in range(a.clips)]
    syn.set_profiling(True)
    q = _abi.OnsetRequest(0, 0, n, 0, 0, 0, 0, 0)
    assert lib.zlhip_onset_resolve(a.sr, C.byref(q)) == 0
    src_bytes = a.clips * n * 8

    energy, rest, wall = [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the call's buffers)
        t0 = time.perf_counter()
        got = syn.clip_onsets_batch([(cid,) for cid in ids])
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            t = syn.onset_timings()
            energy.append(t[0]); rest.append(t[1])
    em, rm = float(np.median(energy)), float(np.median(rest))
    res = dict(metric="sound_onsets", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, reps=a.reps,
               request=dict(hop=q.hop_frames, gate=q.gate, threshold=q.threshold, min_gap=q.min_gap_hops, max_onsets=q.max_onsets),
               hops=a.clips * -(-n // q.hop_frames), onsets=int(sum(len(g) for g in got)), source_bytes=src_bytes,
               energy_ms=em, rest_ms=rm, call_ms=float(np.median(wall)), energy_ms_all=energy, rest_ms_all=rest, call_ms_all=wall,
               energy_GBs=src_bytes / (em * 1e-3) / 1e9, host_bytes=int(sum(8 * len(g) + 4 for g in got)))

    # the overview's reduce over the same bytes: one column per hop
    cols = min(4096, -(-n // q.hop_frames))
    ov = []
    for r in range(a.reps + 1):
        syn.clip_overviews([(cid, cols) for cid in ids])
        if r:
            ov.append(syn.overview_timings())
    om = float(np.median(ov))
    res["overview"] = dict(columns=cols, device_ms=om, device_ms_all=ov, source_GBs=src_bytes / (om * 1e-3) / 1e9)
    res["energy_rate_over_overview_rate"] = om / em

    # the route without the call: every clip over PCIe (zlhip_sound_read), then the same header on the host
    h = C.CDLL(build.build_onset_harness())
    h.zlon_run_planar.restype = C.c_int32
    h.zlon_run_planar.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 8 + [C.c_void_p]
    L = np.empty(n, np.float32); R = np.empty(n, np.float32); ln = C.c_int32(0)
    out = np.zeros((q.max_onsets, 2), np.int32)

    def host():
        t0 = time.perf_counter(); t_read = 0.0
        for i, cid in enumerate(ids):
            t1 = time.perf_counter()
            assert lib.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data, n, C.byref(ln)) == 2
            t_read += time.perf_counter() - t1
            k = h.zlon_run_planar(L.ctypes.data, R.ctypes.data, 0, n, q.hop_frames, q.gate, q.threshold, q.min_gap_hops, q.max_onsets, a.threads, out.ctypes.data)
            assert np.array_equal(out[:k], got[i]), i              # the figures are of two routes that compute the same thing
        return (time.perf_counter() - t0) * 1e3, t_read * 1e3
    host()
    runs = [host() for _ in range(3)]
    total = float(np.median([r[0] for r in runs]))
    res["host"] = dict(route="zlhip_sound_read + zl_onset.h on the host", host_threads=a.threads, total_ms=total,
                       read_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs], ratio_to_call=total / res["call_ms"])
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
