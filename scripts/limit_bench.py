"""The look-ahead limiter on the device (zlhip_sound_limit_batch), measured in one process:

  The bank -- 1024 stereo clips of 2 s at 48 kHz -- limited in ONE call, in two variants, each with and without ZLHIP_LIMIT_TRUE_PEAK,
  each call on a freshly loaded bank:
    bank   1 clip in 8 has a few overs, the realistic case: nearly all tiles are cold (a device copy);
    hot    every clip has an over in every tile: every tile recomputes the detector, the sliding maximum and the window.
  Per variant: device time of the detecting launch and of the render and publishing launches (HIP events, zlhip_debug_limit_timings),
  wall time of the call, median of --reps calls after a warm-up call.  The warm-up call's result is held against the numpy restatement
  on two clips.

  The bar (section 14's): the whole call takes no longer than the route it replaces, in the same run -- zlhip_sound_read of each clip,
  the same header (tests/cpu_harness/limit_host.cpp, the host build of zl_limit.h) on 16 host threads, and a re-upload
  (zlhip_sound_upload_pcm_batch of the limited floats; the old clips are released).

  Beside the bar, without a bar: the ratio of the render kernel to a device-to-device copy of the same bytes, timed with HIP events in
  the same run, and detect and render per byte.

Writes one JSON line to profiles/limit_bench.txt (--out) and prints it.  On a shared machine run it as ONE step under its own time
limit, so that a fault or a hang ends it and nothing else is started on the device behind it:

    timeout -k 10 900 python scripts/limit_bench.py [--clips 1024] [--seconds 2] [--reps 5] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                    # limit_ref: the restatement the first call is held against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limit_bench.txt"))
    a = ap.parse_args()

    import torch
    import limit_ref as lr
    from libzl_amd import SamplerSynth, _abi, build
    K, sr = a.clips, float(a.rate)
    n = int(a.seconds * a.rate)
    floats_of = lambda frames: ((frames + 8) * 2 + 3) & ~3
    arena = 3 * floats_of(n) * 4 * K + (16 << 20)                  # the bank, the call's new extents, the host route's re-upload
    syn = SamplerSynth(2, 8, max_frames=256, max_batch_blocks=8, max_sounds=2 * K + 8, playback_sample_rate=sr, sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    syn.set_profiling(True)
    rng = np.random.default_rng(a.seed)
    quiet = rng.integers(-9830, 9831, (K, n, 2), dtype=np.int16)   # every clip distinct, within +-0.3
    quiet[quiet == 0] = 1
    bank = quiet.copy()
    for f in (n // 7, n // 2, n // 2 + 40):                        # 1 clip in 8: three overs
        bank[::8, f, 0] = 32767
    hot = quiet.copy()
    hot[:, 300::512, 1] = -32768                                   # an over in every tile
    tables = {}
    for F in (4, 2):
        t = np.zeros(F * 64, np.float32)
        assert lib.zlhip_resample_design(sr, sr * F, None, None, None, None, t.ctypes.data, t.size) == 0
        tables[F] = t.reshape(F, 64)
    variants = [("bank", bank, 0), ("bank, true peak", bank, 1), ("hot", hot, 0), ("hot, true peak", hot, 1)]
    clip_bytes = n * 4

    def load(pcm):
        srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(pcm.ctypes.data + i * clip_bytes, n, 2, _abi.PCM_S16, 0, sr) for i in range(K)])
        ids = (C.c_int32 * K)()
        assert lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids) == 0, lib.zlhip_last_error(e)
        return [ids[i] for i in range(K)]

    def release(ids):
        for cid in ids:
            syn.unregister_clip(cid)

    def requests(ids, flags):
        return (_abi.LimitRequest * len(ids))(*[_abi.LimitRequest(cid, flags, 0, 0, 0.0, 0.0) for cid in ids])

    res = dict(metric="sound_limit_batch", device=syn.device_name(), clips=K, seconds=a.seconds, rate=a.rate, channels=2, frames=n, reps=a.reps,
               lookahead_frames=240, hold_frames=0, sliding_maximum="log-step doubling in LDS", variants={})
    h = C.CDLL(build.build_limit_harness())
    h.zllm_call.restype = C.c_int32
    h.zllm_call.argtypes = [C.c_int32] + [C.c_void_p] * 11
    bank_bytes = K * floats_of(n) * 4
    first_host = True

    for name, pcm, flags in variants:
        # ---- the call ------------------------------------------------------------------------------------------------------------
        out = (_abi.Limit * K)()
        detect_ms, render_ms, wall_ms = [], [], []
        for r in range(a.reps + 1):                                # the first call is the warm-up (code objects, the records)
            ids = load(pcm)
            check = (0, K - 1) if pcm is hot else (0, 8)
            before = [np.stack(syn.read_clip(ids[i])) for i in check] if r == 0 else None
            reqs = requests(ids, flags)
            t0 = time.perf_counter()
            rc = lib.zlhip_sound_limit_batch(e, reqs, K, out)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.zlhip_last_error(e))
            applied = sum(out[i].applied for i in range(K))
            if r == 0:                                             # the figures are of a call that limits the right thing
                for x, i in zip(before, check):
                    want, ext, _, _ = lr.limit(x, sr, dict(flags=flags), tables)
                    assert all(np.float32(getattr(out[i], k)).view(np.uint32) == np.float32(want[k]).view(np.uint32) for k in lr.RESULT_FIELDS), (name, i)
                    assert want["applied"] == 1 and np.array_equal(syn.clip_extent(ids[i]).view(np.uint32), ext.view(np.uint32)), (name, i)
            else:
                d, k = syn.limit_timings()
                detect_ms.append(d); render_ms.append(k); wall_ms.append(dt)
            release(ids)
        dm, rm, wm = (float(np.median(v)) for v in (detect_ms, render_ms, wall_ms))
        rendered = applied * floats_of(n) * 4                      # bytes of the new extents: read once, written once
        v = dict(flags=flags, applied=applied, detect_ms=dm, render_ms=rm, call_ms=wm, detect_ms_all=detect_ms, render_ms_all=render_ms, call_ms_all=wall_ms,
                 detect_TB_per_s=bank_bytes / (dm * 1e-3) / 1e12, render_TB_per_s=2.0 * rendered / (rm * 1e-3) / 1e12,
                 detect_ns_per_frame=dm * 1e6 / (K * n), render_ns_per_frame=rm * 1e6 / (applied * n))

        # ---- a device-to-device copy of the rendered bytes, HIP events, the same run ---------------------------------------------------
        src = torch.empty(rendered // 4, dtype=torch.float32, device="cuda").normal_()
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
        v["device_copy"] = dict(ms=cm, ms_all=copy_ms, TB_per_s=2.0 * rendered / (cm * 1e-3) / 1e12, render_to_copy=rm / cm)

        # ---- the route it replaces: read, the same header on 16 host threads, re-upload ---------------------------------------------
        def limit_on_host(args):
            L, R = args
            fl = floats_of(n)
            x = np.zeros(fl, np.float32)
            x[:2 * n] = np.stack([L, R], axis=1).reshape(-1)
            dst, writes = np.empty(fl, np.float32), np.zeros(fl, np.int32)
            qq = requests([0], flags)
            o = _abi.Limit()
            one = lambda arr: (C.c_void_p * 1)(arr.ctypes.data)
            pS, pD, pW = one(x), one(dst), one(writes)
            nsrc, length, ch, rate, verdict, walk = (C.c_int64 * 1)(x.size), (C.c_int32 * 1)(n), (C.c_int32 * 1)(2), (C.c_double * 1)(sr), (C.c_uint32 * 1)(0), (C.c_int64 * 8)()
            rc = h.zllm_call(1, C.addressof(qq), C.addressof(pS), C.addressof(nsrc), C.addressof(length), C.addressof(ch), C.addressof(rate), C.addressof(pD), C.addressof(pW),
                             C.addressof(o), C.addressof(verdict), C.addressof(walk))
            assert rc >= 0 and walk[3] == 0
            return dst[:2 * n] if o.applied else None

        host_ms = []
        with ThreadPoolExecutor(a.threads) as pool:
            for r in range(2 if first_host else 1):                # (the last round is the figure: the first one of the run warms the pool and the pages)
                cur = load(pcm)
                t0 = time.perf_counter()
                planes = [tuple(syn.read_clip(cid)) for cid in cur]
                limited = list(pool.map(limit_on_host, planes))
                todo = [(cid, f) for cid, f in zip(cur, limited) if f is not None]
                new = syn.register_clips_pcm([(f, _abi.PCM_F32, 2, sr) for _, f in todo])
                release([cid for cid, _ in todo])
                host_ms.append((time.perf_counter() - t0) * 1e3)
                release(new)
                release([cid for cid, f in zip(cur, limited) if f is None])
        first_host = False
        v["host_route"] = dict(ms=host_ms[-1], ms_all=host_ms, threads=a.threads, what="zlhip_sound_read per clip, zl_limit.h on host threads, zlhip_sound_upload_pcm_batch (F32) of the clips that changed, release")
        v["bar"] = dict(rule="call_ms <= host_route.ms", met=bool(wm <= host_ms[-1]), ratio=host_ms[-1] / wm)
        res["variants"][name] = v

    res["bar_met"] = all(v["bar"]["met"] for v in res["variants"].values())
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_limit_kernel_resources.txt")
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
