"""Waveform overviews (zlhip_sound_overview_batch): device time (HIP events on the engine's stream, zlhip_set_profiling) and host wall
time of the call, median of 5 after a warm-up call, for
    batch    one call of 1024 x 256 columns over the benchmark's own sources -- 1024 distinct stereo clips of 2 s at 48 kHz, 786 MB
    single   one 15 s stereo clip at 512 and at 4096 columns
against (a) the only other route to the same columns, zlhip_sound_read of every clip plus a min / max scan on the host (numpy, one
thread), timed here, and (b) the box's device-to-device copy rate, measured here the way bench.py --full measures `roofline.
device_copy_GBs` (1 GiB, read + write bytes over time): the kernel reads every source byte once and writes almost nothing, so that rate
is its ceiling.  Prints one JSON line.

    python scripts/overview_bench.py [--clips 1024] [--seconds 2] [--columns 256] [--reps 5] [--no-parent] [--no-copy]
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


def host_columns(L, R, columns):
    """the host's scan of a clip read back with zlhip_sound_read: (min, max) per column and channel"""
    n = L.shape[0]
    lo = (np.arange(columns, dtype=np.int64) * n) // columns
    return np.stack([np.minimum.reduceat(L, lo), np.maximum.reduceat(L, lo), np.minimum.reduceat(R, lo), np.maximum.reduceat(R, lo)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--single-seconds", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--no-copy", action="store_true")
    a = ap.parse_args()

    from libzl_amd import SamplerSynth, _abi
    n = int(a.seconds * a.sr)
    n1 = int(a.single_seconds * a.sr)
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=a.clips + 8, sound_arena_bytes=(n + 16) * 8 * a.clips + (n1 + 16) * 8 + (1 << 20))
    lib, e = syn._lib, syn._e
    rng = np.random.default_rng(a.seed)                            # bench.py's sources: uniform in [-1, 1), every clip distinct
    ids, keep = [], {}
    for v in range(a.clips):
        L = rng.random(n, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
        R = rng.random(n, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
        ids.append(syn.register_clip(L, R, a.sr))
        if v in (0, a.clips - 1):
            keep[v] = (L, R)
    L1 = rng.random(n1, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
    R1 = rng.random(n1, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
    long_id = syn.register_clip(L1, R1, a.sr)
    syn.set_profiling(True)

    def timed(reqs):
        arr = (_abi.OverviewRequest * len(reqs))(*[_abi.OverviewRequest(*r) for r in reqs])
        total = sum(r[3] for r in reqs)
        out = np.empty((total, 4), np.float32)
        dev, wall = [], []
        for r in range(a.reps + 1):                                # the first call is the warm-up (code objects, the call's buffers)
            t0 = time.perf_counter()
            rc = lib.zlhip_sound_overview_batch(e, arr, len(reqs), out.ctypes.data, out.size)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rc
            if r:
                wall.append(dt); dev.append(syn.overview_timings())
        return out, float(np.median(dev)), float(np.median(wall)), dev, wall

    res = dict(metric="sound_overview", device=syn.device_name(), clips=a.clips, seconds=a.seconds, sr=a.sr, columns=a.columns, reps=a.reps)
    out, dev, wall, devs, walls = timed([(cid, 0, n, a.columns) for cid in ids])
    src_bytes = a.clips * n * 8
    for v, (L, R) in keep.items():                                 # the figures are of a call that computes the right thing
        assert np.array_equal(out[v * a.columns:(v + 1) * a.columns], host_columns(L, R, a.columns)), v
    res["batch"] = dict(requests=a.clips, columns_total=a.clips * a.columns, source_bytes=src_bytes, device_ms=dev, call_ms=wall,
                        device_ms_all=devs, call_ms_all=walls, source_GBs=src_bytes / (dev * 1e-3) / 1e9)
    res["single"] = []
    for cols in (512, 4096):
        out1, dev1, wall1, devs1, walls1 = timed([(long_id, 0, n1, cols)])
        assert np.array_equal(out1, host_columns(L1, R1, cols))
        res["single"].append(dict(seconds=a.single_seconds, columns=cols, source_bytes=n1 * 8, device_ms=dev1, call_ms=wall1,
                                  device_ms_all=devs1, call_ms_all=walls1, source_GBs=n1 * 8 / (dev1 * 1e-3) / 1e9))

    if not a.no_parent:
        # the route without zlhip_sound_overview: every clip over PCIe (zlhip_sound_read), then the scan on the host -- numpy, one thread
        def parent(clips, length, cols):
            L = np.empty(length, np.float32); R = np.empty(length, np.float32)
            ln = C.c_int32(0)
            t0 = time.perf_counter(); t_read = 0.0
            for cid in clips:
                t1 = time.perf_counter()
                assert lib.zlhip_sound_read(e, cid, L.ctypes.data, R.ctypes.data, length, C.byref(ln)) == 2
                t_read += time.perf_counter() - t1
                host_columns(L, R, cols)
            return (time.perf_counter() - t0) * 1e3, t_read * 1e3
        parent(ids[:8], n, a.columns)
        runs = [parent(ids, n, a.columns) for _ in range(3)]
        total_ms = float(np.median([r[0] for r in runs]))
        res["parent_batch"] = dict(route="zlhip_sound_read + numpy min/max scan", host_threads=1, total_ms=total_ms,
                                   read_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs],
                                   ratio_to_overview_call=total_ms / res["batch"]["call_ms"])
        res["parent_single"] = []
        for s in res["single"]:
            runs = [parent([long_id], n1, s["columns"]) for _ in range(a.reps)]
            total_ms = float(np.median([r[0] for r in runs]))
            res["parent_single"].append(dict(columns=s["columns"], host_threads=1, total_ms=total_ms, ratio_to_overview_call=total_ms / s["call_ms"]))
    syn.close()

    if not a.no_copy:
        import torch
        x = torch.empty(1 << 28, device="cuda", dtype=torch.float32); y = torch.empty_like(x)      # 1 GiB each, as bench.py --full
        y.copy_(x); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            y.copy_(x)
        e1.record(); torch.cuda.synchronize()
        copy_gbs = 5 * 2 * x.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        res["device_copy_GBs"] = copy_gbs
        res["batch"]["frac_of_device_copy"] = res["batch"]["source_GBs"] / copy_gbs
        for s in res["single"]:
            s["frac_of_device_copy"] = s["source_GBs"] / copy_gbs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
