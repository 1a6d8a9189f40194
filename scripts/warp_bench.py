"""Warp on the device (zlhip_sound_warp_batch), measured in one process on one MI355X:

  1. The call -- 64 stereo clips of 10 s at 48 kHz, a hit every 125 ms (80 regions per clip), every hit moved by up to 3 % of the
     distance between two hits and the whole fitted to 1 / 0.96 of its length -- warped in ONE call: device time of the seek launch and
     of the synthesis and publishing launches (HIP events, zlhip_debug_warp_timings), wall time of the call; median of --reps calls
     after a warm-up call, each on a freshly uploaded bank (a warp replaces the clip's original).  The first call's result is held
     against the numpy restatement (tests/warp_ref.py) on one clip.
  2. The bar (section 14's): the whole call takes no longer than the route it replaces, in the same run -- zlhip_sound_read of each
     clip, the same header (tests/cpu_harness/warp_host.cpp, the host build of zl_warp.h) on 16 host threads, and a re-upload
     (zlhip_sound_upload_pcm_batch of the warped floats; the old clips are released).
  3. Beside the bar, without a bar: zlhip_sound_rerender_batch of the same clips at the uniform speed 0.96, which gives the same total
     output length -- one seek chain of about 150 segments per clip on one workgroup, against 80 chains of 2 segments per clip on 80
     workgroups.  The ratio of the two seek launches is reported whichever way it falls.

Writes one JSON line to profiles/warp_bench.txt (--out) and prints it.  On a shared machine run it as ONE step under its own time
limit, so that a fault or a hang ends it and nothing else is started on the device behind it:

    timeout -k 10 600 python scripts/warp_bench.py [--clips 64] [--seconds 10] [--reps 5] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                    # warp_ref: the restatement the first call is held against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--hit-ms", type=float, default=125.0)
    ap.add_argument("--speed", type=float, default=0.96)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.txt"))
    a = ap.parse_args()

    import warp_ref as wr
    from libzl_amd import SamplerSynth, _abi, build
    K, sr = a.clips, float(a.rate)
    n = int(a.seconds * a.rate)
    speed = float(np.float32(a.speed))
    N = max(1, int(np.floor(n / speed)))                           # the re-render's output length at that speed
    gap = int(round(a.hit_ms * a.rate / 1000.0))
    rng = np.random.default_rng(a.seed)
    # every clip its own anchors: a hit every `gap` frames, its image the uniform one moved by up to 3 % of the gap
    anchors = []
    for i in range(K):
        src = np.arange(0, n, gap, dtype=np.int64)[1:]
        src = src[src < n - gap // 2]
        dst = np.rint(src * (N / n)).astype(np.int64) + rng.integers(-int(0.03 * gap), int(0.03 * gap) + 1, src.size)
        an = np.concatenate([[[0, 0]], np.stack([src, dst], axis=1), [[n, N]]]).astype(np.int32)
        assert wr.resolve(sr, n, an) is not None
        anchors.append(np.ascontiguousarray(an))
    floats_in, floats_out = ((n + 8) * 2 + 3) & ~3, ((N + 8) * 2 + 3) & ~3
    arena = 4 * (floats_in + floats_out) * 4 * K + (64 << 20)
    syn = SamplerSynth(2, 8, max_frames=256, max_batch_blocks=8, max_sounds=4 * K + 8, playback_sample_rate=sr, sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    syn.set_profiling(True)
    raw = (rng.integers(-6000, 6000, (K, n, 2)) + (12000 * np.sin(2 * np.pi * np.arange(n) / 109.0))[None, :, None]).astype(np.int16)   # noise over a tone: every clip distinct
    clip_bytes = n * 4

    def upload_bank():
        srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(raw.ctypes.data + i * clip_bytes, n, 2, _abi.PCM_S16, 0, sr) for i in range(K)])
        ids = (C.c_int32 * K)()
        assert lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids) == 0, lib.zlhip_last_error(e)
        return [ids[i] for i in range(K)]

    summary = wr.resolve(sr, n, anchors[0])[0]
    res = dict(metric="sound_warp_batch", device=syn.device_name(), clips=K, seconds=a.seconds, rate=a.rate, channels=2, frames=n, out_frames=N,
               regions_per_clip=summary["regions"], segments_per_clip=summary["segments"], overlap=summary["overlap"], speed=speed, reps=a.reps)

    # ---- 1. the call -----------------------------------------------------------------------------------------------------------------
    PA = C.POINTER(_abi.WarpAnchor)
    seek_ms, synth_ms, wall_ms = [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the records)
        ids = upload_bank()
        before = np.stack(syn.read_clip(ids[K - 1])) if r == 0 else None
        reqs = (_abi.WarpRequest * K)(*[_abi.WarpRequest(ids[i], anchors[i].shape[0], C.cast(anchors[i].ctypes.data, PA)) for i in range(K)])
        out = (_abi.Warp * K)()
        t0 = time.perf_counter()
        rc = lib.zlhip_sound_warp_batch(e, reqs, K, out)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, lib.zlhip_last_error(e))
        if r == 0:                                                 # the figures are of a call that warps the right thing
            want, y, offs, _ = wr.warp(before, sr, anchors[K - 1])
            assert {k: getattr(out[K - 1], k) for k in wr.RESULT_FIELDS} == want
            assert np.array_equal(syn.warp_offsets(ids[K - 1]), offs)
            assert np.array_equal(syn.clip_extent(ids[K - 1]).view(np.uint32), wr.extent(y).view(np.uint32))
        else:
            s_, y_ = syn.warp_timings()
            seek_ms.append(s_); synth_ms.append(y_); wall_ms.append(dt)
        for cid in ids:
            syn.unregister_clip(cid)
    sm, ym, wm = (float(np.median(v)) for v in (seek_ms, synth_ms, wall_ms))
    res["call"] = dict(seek_ms=sm, synth_ms=ym, call_ms=wm, seek_ms_all=seek_ms, synth_ms_all=synth_ms, call_ms_all=wall_ms,
                       seek_workgroups=K * sum(1 for q in wr.resolve(sr, n, anchors[0])[1] if q["nseg"] > 1),
                       synth_bytes_per_s=(K * (floats_in + floats_out) * 4) / (ym * 1e-3))

    # ---- 3. the uniform stretch of the same clips to the same length (zlhip_sound_rerender_batch) -----------------------------------------
    ids = upload_bank()
    rr_seek, rr_synth, rr_wall = [], [], []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        syn.rerender_clips(ids, 0.0, 0.0, speed)
        dt = (time.perf_counter() - t0) * 1e3
        if r > 0:
            s_, y_ = syn.rerender_timings()
            rr_seek.append(s_); rr_synth.append(y_); rr_wall.append(dt)
    assert syn.clip_info(ids[0])["length"] == N
    nseg = int(syn.rerender_offsets(ids[0]).size)
    rsm, rym, rwm = (float(np.median(v)) for v in (rr_seek, rr_synth, rr_wall))
    res["rerender"] = dict(seek_ms=rsm, synth_ms=rym, call_ms=rwm, seek_ms_all=rr_seek, synth_ms_all=rr_synth, call_ms_all=rr_wall, segments_per_clip=nseg,
                           seek_workgroups=K, seek_ratio_rerender_to_warp=rsm / sm, call_ratio_rerender_to_warp=rwm / wm)
    syn.rerender_clips(ids, 0.0, 0.0, 1.0)                         # the originals play again

    # ---- 2. the route the call replaces: read, the same header on 16 host threads, re-upload ---------------------------------------------
    h = C.CDLL(build.build_warp_harness())
    h.zlwp_call.restype = C.c_int32
    h.zlwp_call.argtypes = [C.c_int32] + [C.c_void_p] * 13

    def warp_on_host(args):
        i, L, R = args
        x = np.ascontiguousarray(np.stack([L, R], axis=1).reshape(-1))
        dst, writes = np.empty(floats_out, np.float32), np.zeros(floats_out, np.int32)
        an = anchors[i]
        o = _abi.Warp()
        one = lambda arr: (C.c_void_p * 1)(arr.ctypes.data)
        pA, pS, pD, pW, pO = one(an), one(x), one(dst), one(writes), (C.c_void_p * 1)(None)
        counts, nsrc, length, ch, rate = (C.c_int32 * 1)(an.shape[0]), (C.c_int64 * 1)(x.size), (C.c_int32 * 1)(n), (C.c_int32 * 1)(2), (C.c_double * 1)(sr)
        verdict, walk = (C.c_uint32 * 1)(0), (C.c_int64 * 4)()
        rc = h.zlwp_call(1, C.addressof(counts), C.addressof(pA), C.addressof(pS), C.addressof(nsrc), C.addressof(length), C.addressof(ch), C.addressof(rate),
                         C.addressof(pD), C.addressof(pW), C.addressof(o), C.addressof(pO), C.addressof(verdict), C.addressof(walk))
        assert rc == 1 and walk[3] == 0
        return dst[:N * 2]

    host_ms = []
    cur = ids
    with ThreadPoolExecutor(a.threads) as pool:
        for r in range(2):                                         # (the second round is the figure: the first one warms the pool and the pages)
            if r == 1:
                for cid in cur:
                    syn.unregister_clip(cid)
                cur = upload_bank()
            t0 = time.perf_counter()
            planes = [(i,) + tuple(syn.read_clip(cur[i])) for i in range(K)]
            warped = list(pool.map(warp_on_host, planes))
            new = syn.register_clips_pcm([(f, _abi.PCM_F32, 2, sr) for f in warped])
            for cid in cur:
                syn.unregister_clip(cid)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            cur = new
    res["host_route"] = dict(ms=host_ms[-1], ms_all=host_ms, threads=a.threads, what="zlhip_sound_read per clip, zl_warp.h on host threads, zlhip_sound_upload_pcm_batch (F32), release")
    res["bar"] = dict(rule="call_ms <= host_route.ms", met=bool(wm <= host_ms[-1]), ratio=host_ms[-1] / wm)
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_warp_kernel_resources.txt")
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
