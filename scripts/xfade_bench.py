"""Loop crossfade on the device (zlhip_sound_loop_crossfade_batch), measured in one process:

  The bank -- 1024 stereo clips of 2 s at 48 kHz, nominal loop the middle half, X = 960, curve AUTO -- crossfaded in ONE call: device
  time of the measuring launch and of the render and publishing launches (HIP events, zlhip_debug_xfade_timings), wall time of the call,
  median of --reps calls after a warm-up call; the render kernel's bytes per second (every extent byte read once and written once).
  The first call's result is held against the numpy restatement on two clips.

  The bar (section 14's): the whole call takes no longer than the route it replaces, in the same run -- zlhip_sound_read of each clip,
  the same header (tests/cpu_harness/xfade_host.cpp, the host build of zl_xfade.h) on 16 host threads, and a re-upload
  (zlhip_sound_upload_pcm_batch of the crossfaded floats; the old clips are released).

  Beside the bar, without a bar: the ratio of the render kernel to a device-to-device copy of the same bytes, timed with HIP events in
  the same run.  The kernel moves the same traffic plus about 1 % of fade groups: a ratio well above 1 names where the next change would go.

Writes one JSON line to profiles/xfade_bench.txt (--out) and prints it.  On a shared machine run it as ONE step under its own time
limit, so that a fault or a hang ends it and nothing else is started on the device behind it:

    timeout -k 10 600 python scripts/xfade_bench.py [--clips 1024] [--seconds 2] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))                    # xfade_ref: the restatement the first call is held against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--fade", type=int, default=960)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xfade_bench.txt"))
    a = ap.parse_args()

    import torch
    import xfade_ref as xr
    from libzl_amd import SamplerSynth, _abi, build
    K, sr, X = a.clips, float(a.rate), a.fade
    n = int(a.seconds * a.rate)
    s0, e0 = n // 4, 3 * n // 4
    floats = ((n + 8) * 2 + 3) & ~3
    arena = 3 * floats * 4 * K + (16 << 20)                        # the bank, the call's new extents, the host route's re-upload
    syn = SamplerSynth(2, 8, max_frames=256, max_batch_blocks=8, max_sounds=2 * K + 8, playback_sample_rate=sr, sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    syn.set_profiling(True)
    rng = np.random.default_rng(a.seed)
    raw = rng.integers(-32768, 32768, (K, n, 2), dtype=np.int16)   # every clip distinct, full range
    clip_bytes = n * 4
    srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(raw.ctypes.data + i * clip_bytes, n, 2, _abi.PCM_S16, 0, sr) for i in range(K)])
    ids = (C.c_int32 * K)()
    assert lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids) == 0, lib.zlhip_last_error(e)
    res = dict(metric="sound_loop_crossfade_batch", device=syn.device_name(), clips=K, seconds=a.seconds, rate=a.rate, channels=2, frames=n,
               start_frame=s0, stop_frame=e0, fade_frames=X, curve="auto", reps=a.reps, extent_bytes=K * floats * 4)

    # ---- the call ----------------------------------------------------------------------------------------------------------------
    reqs = (_abi.XfadeRequest * K)(*[_abi.XfadeRequest(ids[i], s0, e0, X, _abi.XFADE_AUTO) for i in range(K)])
    out = (_abi.Xfade * K)()
    measure_ms, render_ms, wall_ms = [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the records)
        before = [np.stack(syn.read_clip(ids[i])) for i in (0, K - 1)] if r == 0 else None
        t0 = time.perf_counter()
        rc = lib.zlhip_sound_loop_crossfade_batch(e, reqs, K, out)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, lib.zlhip_last_error(e))
        if r == 0:                                                 # the figures are of a call that fades the right thing
            for x, i in zip(before, (0, K - 1)):
                want, y = xr.crossfade(x, sr, s0, e0, X, xr.AUTO)
                assert (out[i].sab, out[i].saa, out[i].sbb, out[i].rho) == (want["sab"], want["saa"], want["sbb"], want["rho"]), i
                assert np.array_equal(syn.clip_extent(ids[i]).view(np.uint32), xr.extent(y).view(np.uint32)), i
        else:
            m, k = syn.xfade_timings()
            measure_ms.append(m); render_ms.append(k); wall_ms.append(dt)
    mm, rm, wm = (float(np.median(v)) for v in (measure_ms, render_ms, wall_ms))
    traffic = 2.0 * K * floats * 4
    res["call"] = dict(measure_ms=mm, render_ms=rm, call_ms=wm, measure_ms_all=measure_ms, render_ms_all=render_ms, call_ms_all=wall_ms,
                       render_bytes_per_s=traffic / (rm * 1e-3), render_TB_per_s=traffic / (rm * 1e-3) / 1e12)

    # ---- a device-to-device copy of the same bytes, HIP events, the same run ----------------------------------------------------------
    src = torch.empty(K * floats, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy_ms = []
    for r in range(a.reps + 1):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(); dst.copy_(src); ev1.record()
        torch.cuda.synchronize()
        if r > 0:
            copy_ms.append(float(ev0.elapsed_time(ev1)))
    del src, dst
    cm = float(np.median(copy_ms))
    res["device_copy"] = dict(ms=cm, ms_all=copy_ms, bytes_per_s=traffic / (cm * 1e-3), render_to_copy=rm / cm)

    # ---- the route it replaces: read, the same header on 16 host threads, re-upload -------------------------------------------------
    h = C.CDLL(build.build_xfade_harness())
    h.zlxf_call.restype = C.c_int32
    h.zlxf_call.argtypes = [C.c_int32] + [C.c_void_p] * 12

    def fade_on_host(args):
        i, L, R = args
        x = np.ascontiguousarray(np.stack([L, R], axis=1).reshape(-1))
        dst, writes, ab = np.empty(floats, np.float32), np.zeros(floats, np.int32), np.empty(2 * X, np.float32)
        q = _abi.XfadeRequest(0, s0, e0, X, _abi.XFADE_AUTO)
        o = _abi.Xfade()
        one = lambda arr: (C.c_void_p * 1)(arr.ctypes.data)
        pS, pD, pW, pA = one(x), one(dst), one(writes), one(ab)
        nsrc, length, ch, rate, verdict, walk = (C.c_int64 * 1)(x.size), (C.c_int32 * 1)(n), (C.c_int32 * 1)(2), (C.c_double * 1)(sr), (C.c_uint32 * 1)(0), (C.c_int64 * 4)()
        rc = h.zlxf_call(1, C.addressof(q), C.addressof(pS), C.addressof(nsrc), C.addressof(length), C.addressof(ch), C.addressof(rate), C.addressof(pD), C.addressof(pW),
                         C.addressof(o), C.addressof(pA), C.addressof(verdict), C.addressof(walk))
        assert rc == 1 and walk[3] == 0
        return dst[:n * 2]

    host_ms = []
    cur = [ids[i] for i in range(K)]
    with ThreadPoolExecutor(a.threads) as pool:
        for r in range(2):                                         # (the second round is the figure: the first one warms the pool and the pages)
            t0 = time.perf_counter()
            planes = [(i,) + tuple(syn.read_clip(cur[i])) for i in range(K)]
            faded = list(pool.map(fade_on_host, planes))
            new = syn.register_clips_pcm([(f, _abi.PCM_F32, 2, sr) for f in faded])
            for cid in cur:
                syn.unregister_clip(cid)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            cur = new
    res["host_route"] = dict(ms=host_ms[-1], ms_all=host_ms, threads=a.threads, what="zlhip_sound_read per clip, zl_xfade.h on host threads, zlhip_sound_upload_pcm_batch (F32), release")
    res["bar"] = dict(rule="call_ms <= host_route.ms", met=bool(wm <= host_ms[-1]), ratio=host_ms[-1] / wm)
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_xfade_kernel_resources.txt")
    if os.path.exists(path):
        res["kernel_resources"] = [line.strip() for line in open(path)]
    syn.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
