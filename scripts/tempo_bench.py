"""Tempo estimate (zlhip_sound_tempo_batch): one call over 64 stereo clips of 10 s at 48 kHz with the defaults, median of 5 after a
warm-up call, profiling on -- the device time of the energy pass, of the autocorrelation kernel and of the rest
(zlhip_debug_tempo_timings), the host wall time of the call and the integer multiply-adds per second of the autocorrelation kernel --
and one request of 65536 hops (hop 64, the defaults' range: 16 segments x 18 tiles of lags).  In the same session and on the same clips:
    host       zlhip_sound_read of every clip plus a 16-thread host build of the same header (tests/cpu_harness/tempo_host.cpp,
               zltp_run_planar), whose records must equal the device's
Prints one JSON line.

    python scripts/tempo_bench.py [--clips 64] [--seconds 10] [--reps 5] [--threads 16]
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
    """a drum-loop-like clip at a tempo of its own between 80 and 145 bpm: decaying noise hits on the beats and, more quietly, on the
    eighths, over a quiet noise floor"""
    bpm = rng.uniform(80.0, 145.0)
    x = rng.uniform(-0.003, 0.003, (2, n))
    beat = 60.0 * sr / bpm
    k = 0
    while int(k * beat / 2) < n:
        at = int(k * beat / 2)
        m = min(n - at, int(0.15 * sr))
        x[:, at:at + m] += (0.6 if k % 2 == 0 else 0.15) * rng.uniform(-1.0, 1.0, (2, m)) * np.exp(-np.arange(m) / (0.02 * sr))
        k += 1
    return x.astype(np.float32), bpm


def macs(rec_hops, first_lag, nlags):
    """the products the definition asks for: the sum over the lags of hops - lag"""
    return sum(rec_hops - (first_lag + l) for l in range(nlags))


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
    big = 65536 * 64
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=a.clips + 8, sound_arena_bytes=(n + 16) * 8 * a.clips + (big + 16) * 4 + (1 << 20))
    lib, e = syn._lib, syn._e
    rng = np.random.default_rng(a.seed)
    made = [clip(rng, n, a.sr) for _ in range(a.clips)]
    ids = [syn.register_clip(x[0], x[1], a.sr) for x, _ in made]
    syn.set_profiling(True)
    q = _abi.TempoRequest(0, 0, n, 0, 0.0, 0.0)
    assert lib.zlhip_tempo_resolve(a.sr, C.byref(q)) == 0
    src_bytes = a.clips * n * 8

    energy, acf, rest, wall = [], [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the call's buffers)
        t0 = time.perf_counter()
        got = syn.clip_tempo_batch([(cid,) for cid in ids])
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(dt)
            t = syn.tempo_timings()
            energy.append(t[0]); acf.append(t[1]); rest.append(t[2])
    em, am, rm = float(np.median(energy)), float(np.median(acf)), float(np.median(rest))
    geo = [syn.tempo_acf(i) for i in range(a.clips)]
    products = sum(macs(g["hops"], first, len(A)) for g, (W, first, A) in zip(got, geo))
    err = [abs(g["bpm"] - bpm) for g, (_, bpm) in zip(got, made)]
    res = dict(metric="sound_tempo", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, reps=a.reps,
               request=dict(hop=q.hop_frames, bpm_min=q.bpm_min, bpm_max=q.bpm_max), hops=a.clips * -(-n // q.hop_frames),
               lags=int(sum(len(A) for _, _, A in geo)), source_bytes=src_bytes, energy_ms=em, acf_ms=am, rest_ms=rm, call_ms=float(np.median(wall)),
               energy_ms_all=energy, acf_ms_all=acf, rest_ms_all=rest, call_ms_all=wall, energy_GBs=src_bytes / (em * 1e-3) / 1e9,
               acf_products=products, acf_Gmacs=products / (am * 1e-3) / 1e9, acf_over_energy=am / em, host_bytes=72 * a.clips,
               worst_bpm_error=float(max(err)), min_confidence=float(min(g["confidence"] for g in got)))

    # one request of 65536 hops
    cid = syn.register_clip(rng.uniform(-0.5, 0.5, big).astype(np.float32) * (0.05 + (np.arange(big) % 32000 < 3000)).astype(np.float32), None, a.sr)
    one = []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        g = syn.clip_tempo(cid, 0, big, 64)
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            one.append((dt,) + syn.tempo_timings())
    W, first, A = syn.tempo_acf(0)
    p1 = macs(65536, first, len(A))
    med = [float(np.median([o[k] for o in one])) for k in range(4)]
    res["one_request_of_65536_hops"] = dict(hop=64, lags=len(A), products=p1, call_ms=med[0], energy_ms=med[1], acf_ms=med[2], rest_ms=med[3],
                                            acf_Gmacs=p1 / (med[2] * 1e-3) / 1e9, bpm=g["bpm"])
    syn.unregister_clip(cid)

    # the route without the call: every clip over PCIe (zlhip_sound_read), then the same header on the host
    h = C.CDLL(build.build_tempo_harness())
    h.zltp_run_planar.restype = C.c_int32
    h.zltp_run_planar.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_float, C.c_float, C.c_int32, C.POINTER(_abi.Tempo)]
    L = np.empty(n, np.float32); R = np.empty(n, np.float32); ln = C.c_int32(0)
    out = _abi.Tempo()

    def host():
        t0 = time.perf_counter(); t_read = 0.0
        for i, cid in enumerate(ids):
            t1 = time.perf_counter()
            assert lib.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data, n, C.byref(ln)) == 2
            t_read += time.perf_counter() - t1
            assert h.zltp_run_planar(L.ctypes.data, R.ctypes.data, 0, n, a.sr, 0, 0.0, 0.0, a.threads, C.byref(out)) == 0
            assert all(getattr(out, k) == got[i][k] for k in got[i]), i      # the figures are of two routes that compute the same thing
        return (time.perf_counter() - t0) * 1e3, t_read * 1e3
    host()
    runs = [host() for _ in range(3)]
    total = float(np.median([r[0] for r in runs]))
    res["host"] = dict(route="zlhip_sound_read + zl_tempo.h on the host", host_threads=a.threads, total_ms=total,
                       read_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs], ratio_to_call=total / res["call_ms"])
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
