"""Clip edit on the device (zlhip_sound_edit_batch), measured in one process:

  The bank -- 1024 stereo clips of 2 s at 48 kHz -- edited in ONE call, in three variants, each on a freshly loaded bank:
    trim     ZLHIP_EDIT_TRIM over clips with 100 ms of silence on each side (the scan reads every clip whole);
    crop     the middle half from an ODD start frame, so that the source of every 16-byte group is misaligned by 8 bytes;
    reverse  the whole clip turned round.
  Per variant: device time of the scanning launch and of the render and publishing launches (HIP events, zlhip_debug_edit_timings),
  wall time of the call, median of --reps calls after a warm-up call; the render kernel's bytes per second (every byte of the new
  extents written once, every kept sample read once).  The warm-up call's result is held against the numpy restatement on two clips.

  The bar (section 14's): the whole call takes no longer than the route it replaces, in the same run -- zlhip_sound_read of each clip,
  the same header (tests/cpu_harness/edit_host.cpp, the host build of zl_edit.h) on 16 host threads, and a re-upload
  (zlhip_sound_upload_pcm_batch of the edited floats; the old clips are released).

  Beside the bar, without a bar: the ratio of the render kernel to a device-to-device copy of the rendered bytes, timed with HIP events
  in the same run, and the loop crossfade's render kernel (an aligned copy) over the same bank in the same run.

Writes one JSON line to profiles/edit_bench.txt (--out) and prints it.  On a shared machine run it as ONE step under its own time
limit, so that a fault or a hang ends it and nothing else is started on the device behind it:

    timeout -k 10 600 python scripts/edit_bench.py [--clips 1024] [--seconds 2] [--reps 5] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                    # edit_ref: the restatement the first call is held against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.txt"))
    a = ap.parse_args()

    import torch
    import edit_ref as er
    from libzl_amd import SamplerSynth, _abi, build
    K, sr = a.clips, float(a.rate)
    n = int(a.seconds * a.rate)
    gap = int(0.1 * a.rate)
    floats_of = lambda frames: ((frames + 8) * 2 + 3) & ~3
    arena = 3 * floats_of(n) * 4 * K + (16 << 20)                  # the bank, the call's new extents, the host route's re-upload
    syn = SamplerSynth(2, 8, max_frames=256, max_batch_blocks=8, max_sounds=2 * K + 8, playback_sample_rate=sr, sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    syn.set_profiling(True)
    rng = np.random.default_rng(a.seed)
    raw = rng.integers(-32768, 32768, (K, n, 2), dtype=np.int16)   # every clip distinct, full range
    raw[raw == 0] = 1
    quiet = raw.copy()
    quiet[:, :gap] = 0; quiet[:, n - gap:] = 0                     # 100 ms of silence on each side
    quiet[:, gap] = 20000; quiet[:, n - gap - 1] = -20000
    odd = (n // 4) | 1
    variants = [("trim", quiet, dict(flags=er.TRIM)), ("crop", raw, dict(first_frame=odd, num_frames=n // 2)), ("reverse", raw, dict(flags=er.REVERSE))]
    clip_bytes = n * 4

    def load(pcm):
        srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(pcm.ctypes.data + i * clip_bytes, n, 2, _abi.PCM_S16, 0, sr) for i in range(K)])
        ids = (C.c_int32 * K)()
        assert lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids) == 0, lib.zlhip_last_error(e)
        return [ids[i] for i in range(K)]

    def release(ids):
        for cid in ids:
            syn.unregister_clip(cid)

    def requests(ids, q):
        q = er.request(**q)
        return (_abi.EditRequest * len(ids))(*[_abi.EditRequest(cid, *(int(q[k]) for k in er.REQUEST_KEYS[:-1]), float(q["threshold"])) for cid in ids])

    res = dict(metric="sound_edit_batch", device=syn.device_name(), clips=K, seconds=a.seconds, rate=a.rate, channels=2, frames=n, reps=a.reps,
               load_shape="one dword-aligned 16-byte load per full destination group, scalar loads for the one group the data's end cuts", variants={})
    h = C.CDLL(build.build_edit_harness())
    h.zled_call.restype = C.c_int32
    h.zled_call.argtypes = [C.c_int32] + [C.c_void_p] * 12

    for name, pcm, q in variants:
        # ---- the call ------------------------------------------------------------------------------------------------------------
        out = (_abi.Edit * K)()
        scan_ms, render_ms, wall_ms = [], [], []
        for r in range(a.reps + 1):                                # the first call is the warm-up (code objects, the records)
            ids = load(pcm)
            before = [np.stack(syn.read_clip(ids[i])) for i in (0, K - 1)] if r == 0 else None
            reqs = requests(ids, q)
            t0 = time.perf_counter()
            rc = lib.zlhip_sound_edit_batch(e, reqs, K, out)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.zlhip_last_error(e))
            assert all(out[i].applied == 1 for i in range(K))
            if r == 0:                                             # the figures are of a call that edits the right thing
                for x, i in zip(before, (0, K - 1)):
                    want, y = er.edit(x, er.request(**q))
                    assert all(getattr(out[i], k) == want[k] for k in er.RESULT_FIELDS), (name, i)
                    assert np.array_equal(syn.clip_extent(ids[i]).view(np.uint32), er.extent(y).view(np.uint32)), (name, i)
            else:
                s, k = syn.edit_timings()
                scan_ms.append(s); render_ms.append(k); wall_ms.append(dt)
            new_len = out[0].length
            release(ids)
        sm, rm, wm = (float(np.median(v)) for v in (scan_ms, render_ms, wall_ms))
        written = K * floats_of(new_len) * 4
        traffic = float(written + K * new_len * 2 * 4)
        v = dict(request=q, new_frames=new_len, scan_ms=sm, render_ms=rm, call_ms=wm, scan_ms_all=scan_ms, render_ms_all=render_ms, call_ms_all=wall_ms,
                 render_bytes=traffic, render_TB_per_s=traffic / (rm * 1e-3) / 1e12)
        if sm > 0.0:
            v["scan_TB_per_s"] = K * n * 2 * 4 / (sm * 1e-3) / 1e12

        # ---- a device-to-device copy of the rendered bytes, HIP events, the same run ---------------------------------------------------
        src = torch.empty(written // 4, dtype=torch.float32, device="cuda").normal_()
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
        v["device_copy"] = dict(ms=cm, ms_all=copy_ms, TB_per_s=2.0 * written / (cm * 1e-3) / 1e12, render_to_copy=rm / cm)

        # ---- the route it replaces: read, the same header on 16 host threads, re-upload ---------------------------------------------
        def edit_on_host(args):
            L, R = args
            x = np.ascontiguousarray(np.stack([L, R], axis=1).reshape(-1))
            fl = floats_of(n)
            dst, writes, w = np.empty(fl, np.float32), np.zeros(fl, np.int32), np.empty(n // 2 + 1, np.float32)
            qq = requests([0], q)
            o = _abi.Edit()
            one = lambda arr: (C.c_void_p * 1)(arr.ctypes.data)
            pS, pD, pW, pI, pO = one(x), one(dst), one(writes), one(w), one(w)
            nsrc, length, ch, verdict, walk = (C.c_int64 * 1)(x.size), (C.c_int32 * 1)(n), (C.c_int32 * 1)(2), (C.c_uint32 * 1)(0), (C.c_int64 * 6)()
            rc = h.zled_call(1, C.addressof(qq), C.addressof(pS), C.addressof(nsrc), C.addressof(length), C.addressof(ch), C.addressof(pD), C.addressof(pW),
                             C.addressof(o), C.addressof(pI), C.addressof(pO), C.addressof(verdict), C.addressof(walk))
            assert rc == 1 and walk[3] == 0
            return dst[:o.length * 2]

        host_ms = []
        with ThreadPoolExecutor(a.threads) as pool:
            for r in range(2):                                     # (the second round is the figure: the first one warms the pool and the pages)
                cur = load(pcm)
                t0 = time.perf_counter()
                planes = [tuple(syn.read_clip(cid)) for cid in cur]
                edited = list(pool.map(edit_on_host, planes))
                new = syn.register_clips_pcm([(f, _abi.PCM_F32, 2, sr) for f in edited])
                release(cur)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                release(new)
        v["host_route"] = dict(ms=host_ms[-1], ms_all=host_ms, threads=a.threads, what="zlhip_sound_read per clip, zl_edit.h on host threads, zlhip_sound_upload_pcm_batch (F32), release")
        v["bar"] = dict(rule="call_ms <= host_route.ms", met=bool(wm <= host_ms[-1]), ratio=host_ms[-1] / wm)
        res["variants"][name] = v

    # ---- the loop crossfade's render kernel (an aligned copy of whole extents) over the same bank, the same run ----------------------------
    ids = load(raw)
    xreqs = (_abi.XfadeRequest * K)(*[_abi.XfadeRequest(cid, n // 4, 3 * n // 4, 960, _abi.XFADE_AUTO) for cid in ids])
    xout = (_abi.Xfade * K)()
    xr_ms = []
    for r in range(a.reps + 1):
        assert lib.zlhip_sound_loop_crossfade_batch(e, xreqs, K, xout) == 0, lib.zlhip_last_error(e)
        if r > 0:
            xr_ms.append(syn.xfade_timings()[1])
    release(ids)
    xm = float(np.median(xr_ms))
    res["xfade_render"] = dict(ms=xm, ms_all=xr_ms, TB_per_s=2.0 * K * floats_of(n) * 4 / (xm * 1e-3) / 1e12)
    res["bar_met"] = all(v["bar"]["met"] for v in res["variants"].values())
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_edit_kernel_resources.txt")
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
