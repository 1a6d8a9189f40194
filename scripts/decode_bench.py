"""Clips from raw PCM (zlhip_sound_upload_pcm_batch): the benchmark's source set as files would hold it -- 1024 stereo clips of 2 s at
48 kHz, as S16 (393 MB) and as S24 (590 MB) -- loaded in ONE call from pageable and from page-locked memory, median of 5 calls after a
warm-up call.  Reported per case: the call's wall time, the device time of its copies and of its decode launches (HIP events,
zlhip_debug_upload_pcm_timings), the raw PCM rate of the call against the box's own host-to-device copy of the same bytes from the same
kind of memory (taken here) and against the 63 GB/s the link is specified at, and the decode launches' output rate against the box's
device-to-device copy rate (taken here as bench.py --full takes it).
Against the parent's route, in the same process: the same data as WAV files through libzl_wav_read (the host decode loop) plus
zlhip_sound_upload, clip by clip -- and, so that both sides read the files, the new route through libzl_hotpath_clips_new.
Writes one JSON line to profiles/decode_bench.txt (--out) and prints it.

    python scripts/decode_bench.py [--clips 1024] [--seconds 2] [--reps 5] [--no-parent] [--no-copy] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LINK_GBS = 63.0                                                    # PCIe 5.0 x16, one direction, as specified


def wav_header(nbytes, channels, rate, bits):
    import struct
    block = channels * bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * block, block, bits)
            + b"data" + struct.pack("<I", nbytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.txt"))
    a = ap.parse_args()

    from libzl_amd import SamplerSynth, _abi, libzl
    from libzl_amd.engine import pinned_array
    n, K = int(a.seconds * a.sr), a.clips
    arena = (n + 16) * 8 * K + (1 << 20)
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=K + 8, sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    zl = libzl.load()
    syn.set_profiling(True)
    rng = np.random.default_rng(a.seed)
    res = dict(metric="sound_upload_pcm_batch", device=syn.device_name(), clips=K, seconds=a.seconds, sr=a.sr, channels=2, reps=a.reps,
               link_GBs=LINK_GBS, fp32_bytes=K * n * 8, cases={})
    ids = (C.c_int32 * K)()

    def release():
        for i in range(K):
            assert lib.zlhip_sound_release(e, ids[i]) == 0

    def reference(raw_clip, fmt):
        """numpy's decode of one clip -> planar [2][n]"""
        b = raw_clip.reshape(-1, _abi.PCM_BYTES[fmt]).astype(np.int64)
        v = (b[:, 0] << 16 | b[:, 1] << 24) if fmt == _abi.PCM_S16 else (b[:, 0] << 8 | b[:, 1] << 16 | b[:, 2] << 24)
        v = np.where(v >= 2 ** 31, v - 2 ** 32, v)
        return (v.astype(np.float64) * 2.0 ** -31).astype(np.float32).reshape(-1, 2).T

    raws = {}
    for name, fmt in (("s16", _abi.PCM_S16), ("s24", _abi.PCM_S24)):
        clip_bytes = n * 2 * _abi.PCM_BYTES[fmt]
        raws[name] = rng.integers(0, 256, K * clip_bytes, dtype=np.uint8)             # every clip distinct, full range
        for mem in ("pageable", "page_locked"):
            if mem == "pageable":
                buf = raws[name]
            else:
                buf = pinned_array(lib, (K * clip_bytes,), np.uint8)
                buf[:] = raws[name]
            srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(buf.ctypes.data + i * clip_bytes, n, 2, fmt, 0, float(a.sr)) for i in range(K)])
            wall, copy, dec = [], [], []
            for r in range(a.reps + 1):                            # the first call is the warm-up (code objects, the staging buffer)
                t0 = time.perf_counter()
                rc = lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids)
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0, (rc, lib.zlhip_last_error(e))
                if r == 0:                                         # the figures are of a call that loads the right thing
                    for i in (0, K - 1):
                        L, R = syn.read_clip(ids[i])
                        assert np.array_equal(np.stack([L, R]).view(np.uint32), reference(raws[name][i * clip_bytes:(i + 1) * clip_bytes], fmt).view(np.uint32)), i
                else:
                    wall.append(dt)
                    c, d = syn.upload_pcm_timings()
                    copy.append(c); dec.append(d)
                release()
            w, c, d = float(np.median(wall)), float(np.median(copy)), float(np.median(dec))
            raw_bytes = K * clip_bytes
            res["cases"][f"{name}_{mem}"] = dict(raw_bytes=raw_bytes, call_ms=w, copy_ms=c, decode_ms=d, call_ms_all=wall, copy_ms_all=copy, decode_ms_all=dec,
                                                raw_GBs=raw_bytes / (w * 1e-3) / 1e9, frac_of_link=raw_bytes / (w * 1e-3) / 1e9 / LINK_GBS,
                                                decode_out_GBs=K * (n + 8) * 8 / (d * 1e-3) / 1e9)
            del srcs, buf

    if not a.no_copy:
        import torch
        for name in ("s16", "s24"):
            nbytes = raws[name].size
            dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            for mem in ("pageable", "page_locked"):
                host = torch.from_numpy(raws[name]) if mem == "pageable" else torch.from_numpy(raws[name]).pin_memory()
                ts = []
                for r in range(a.reps + 1):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    dev.copy_(host); torch.cuda.synchronize()
                    if r:
                        ts.append((time.perf_counter() - t0) * 1e3)
                ms = float(np.median(ts))
                cs = res["cases"][f"{name}_{mem}"]
                cs["memcpy_ms"] = ms; cs["memcpy_GBs"] = nbytes / (ms * 1e-3) / 1e9
                cs["frac_of_memcpy"] = cs["raw_GBs"] / cs["memcpy_GBs"]
                del host
            del dev
        x = torch.empty(1 << 28, device="cuda", dtype=torch.float32); y = torch.empty_like(x)      # 1 GiB each, as bench.py --full
        y.copy_(x); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            y.copy_(x)
        e1.record(); torch.cuda.synchronize()
        res["device_copy_GBs"] = 5 * 2 * x.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        for cs in res["cases"].values():
            # the decode reads the raw bytes and writes fp32: both directions over the device-to-device copy's read + write rate
            cs["decode_frac_of_device_copy"] = ((cs["raw_bytes"] + K * (n + 8) * 8) / (cs["decode_ms"] * 1e-3) / 1e9) / res["device_copy_GBs"]
        del x, y

    if not a.no_parent:
        tmp = tempfile.mkdtemp(prefix="zl_decode_bench_")
        try:
            for name, fmt in (("s16", _abi.PCM_S16), ("s24", _abi.PCM_S24)):
                clip_bytes = n * 2 * _abi.PCM_BYTES[fmt]
                paths = []
                for i in range(K):
                    p = os.path.join(tmp, f"{name}_{i:04d}.wav")
                    with open(p, "wb") as f:
                        f.write(wav_header(clip_bytes, 2, a.sr, 8 * _abi.PCM_BYTES[fmt]))
                        f.write(raws[name][i * clip_bytes:(i + 1) * clip_bytes].tobytes())
                    paths.append(p.encode())

                def parent():
                    """the parent's route: libzl_wav_read (file + the host decode loop), zlhip_sound_upload, clip by clip"""
                    L, R = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
                    ln, sr = C.c_int(0), C.c_double(0.0)
                    out = C.c_int32(-1)
                    t0 = time.perf_counter(); t_dec = 0.0
                    for i, p in enumerate(paths):
                        t1 = time.perf_counter()
                        assert zl.libzl_wav_read(p, C.byref(L), C.byref(R), C.byref(ln), C.byref(sr)) == 0
                        t_dec += time.perf_counter() - t1
                        assert lib.zlhip_sound_upload(e, L, R, ln.value, sr.value, C.byref(out)) == 0
                        ids[i] = out.value
                        zl.libzl_wav_free(L); zl.libzl_wav_free(R)
                    return (time.perf_counter() - t0) * 1e3, t_dec * 1e3
                runs = []
                for r in range(4):                                 # (the first run warms the page cache)
                    ms = parent()
                    if r:
                        runs.append(ms)
                    release()
                total = float(np.median([r[0] for r in runs]))
                cs = res["cases"][f"{name}_pageable"]
                res[f"parent_{name}"] = dict(route="libzl_wav_read + zlhip_sound_upload, clip by clip", host_threads=1, total_ms=total,
                                             read_and_decode_ms=float(np.median([r[1] for r in runs])), total_ms_all=[r[0] for r in runs],
                                             ratio_to_batch_call=total / cs["call_ms"])
                if name == "s16":
                    # both sides from the files: the libzl-named layer, a fresh engine per run (its clips are released lazily by cycles)
                    cfg = _abi.Config()
                    lib.zlhip_config_default(C.byref(cfg))
                    cfg.num_buses, cfg.voices_per_bus, cfg.max_sounds, cfg.sound_arena_bytes = 1, 1, K + 8, arena
                    arr = (C.c_char_p * K)(*paths)
                    outp = (C.c_void_p * K)()
                    layer = {}
                    for route in ("clips_new", "ClipAudioSource_new, ZL_PCM_DECODE=0"):
                        ts = []
                        for r in range(3):
                            zl.libzl_hotpath_configure(C.byref(cfg))
                            zl.initJuce()
                            assert zl.libzl_hotpath_status() == 0
                            if route == "clips_new":
                                os.environ.pop("ZL_PCM_DECODE", None)
                                t0 = time.perf_counter()
                                assert zl.libzl_hotpath_clips_new(arr, K, outp) == K
                            else:
                                os.environ["ZL_PCM_DECODE"] = "0"
                                t0 = time.perf_counter()
                                for p in paths:
                                    assert zl.ClipAudioSource_new(p, False)
                            dt = (time.perf_counter() - t0) * 1e3
                            os.environ.pop("ZL_PCM_DECODE", None)
                            zl.shutdownJuce()
                            if r:
                                ts.append(dt)
                        layer[route] = dict(ms=float(np.median(ts)), ms_all=ts)
                    res["libzl_layer_s16"] = dict(layer, ratio=layer["ClipAudioSource_new, ZL_PCM_DECODE=0"]["ms"] / layer["clips_new"]["ms"])
                for p in paths:
                    os.remove(p)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    syn.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
