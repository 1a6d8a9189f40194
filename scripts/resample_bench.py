"""Sample-rate conversion on the device (zlhip_sound_convert_rate_batch), two measurements in one process:

  1. The benchmark's bank as files would hold it -- 1024 stereo clips of 2 s at 44.1 kHz, S16 -- loaded with
     zlhip_sound_upload_pcm_batch and converted to 48 kHz in ONE call: device time of the conversion (HIP events around its two
     launches), wall time of the call, and the device time of the load's copies beside it (zlhip_debug_upload_pcm_timings), median of
     --reps calls after a warm-up call.  The bar: the conversion costs no more device time than the copy of the same clips in the
     same run (converting at load then at most doubles a load).  The first call's result is held against the numpy restatement.
  2. The payoff: 1024 looping voices (8 buses x 128), 256-frame blocks, zlhip_render_batch; K2 time from zlhip_last_timings with the
     unconverted bank (the voices step at 0.91875: the pitched path) and with the converted one (unit step: the on-grid path), in
     --rounds alternating rounds.

Writes one JSON line to profiles/resample_bench.txt (--out) and prints it.  On a shared machine run it as ONE step under its own time
limit, so that a fault or a hang ends it and nothing else is started on the device behind it:

    timeout -k 10 900 python scripts/resample_bench.py [--clips 1024] [--seconds 2] [--reps 5] [--rounds 3] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                    # resample_ref: the restatement the first call is held against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=1024, help="clips of the bank; also the voices of the payoff run (a multiple of 8)")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--source-rate", type=int, default=44100)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2048, help="256-frame blocks per zlhip_render_batch call")
    ap.add_argument("--steps", type=int, default=5, help="timed render calls per bank and round (after two warm-up calls)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.txt"))
    a = ap.parse_args()

    import resample_ref as rr
    from libzl_amd import SamplerSynth, _abi, clip_command
    from libzl_amd.engine import synthetic_clocks
    K, fs, ft = a.clips, a.source_rate, a.rate
    assert K % 8 == 0
    n = int(a.seconds * fs)
    N = rr.out_frames(fs, ft, n)
    B, vpb, NF, KB = 8, K // 8, 256, a.blocks
    # the unconverted bank stays; a second one is loaded and converted per repetition (both of its extents exist during the call)
    arena = (2 * (n + 16) + (N + 16)) * 8 * K + (4 << 20)
    syn = SamplerSynth(B, vpb, max_frames=NF, max_batch_blocks=KB, max_sounds=2 * K + 8, playback_sample_rate=float(ft), sound_arena_bytes=arena)
    lib, e = syn._lib, syn._e
    syn.set_profiling(True)
    rng = np.random.default_rng(a.seed)
    raw = rng.integers(-32768, 32768, (K, n, 2), dtype=np.int16)   # every clip distinct, full range
    clip_bytes = n * 4
    res = dict(metric="sound_convert_rate_batch", device=syn.device_name(), clips=K, seconds=a.seconds, source_rate=fs, rate=ft, channels=2,
               reps=a.reps, source_frames=n, converted_frames=N, raw_bytes=K * clip_bytes, output_frames=K * N)
    L_, M_, T_, row_ = (C.c_int32(0) for _ in range(4))
    assert lib.zlhip_resample_design(float(fs), float(ft), C.byref(L_), C.byref(M_), C.byref(T_), C.byref(row_), None, 0) == 0
    table = np.zeros((L_.value, row_.value), np.float32)
    assert lib.zlhip_resample_design(float(fs), float(ft), None, None, None, None, table.ctypes.data, table.size) == 0
    res.update(L=L_.value, M=M_.value, taps=T_.value)

    def load():
        srcs = (_abi.PcmSource * K)(*[_abi.PcmSource(raw.ctypes.data + i * clip_bytes, n, 2, _abi.PCM_S16, 0, float(fs)) for i in range(K)])
        ids = (C.c_int32 * K)()
        rc = lib.zlhip_sound_upload_pcm_batch(e, srcs, K, ids)
        assert rc == 0, (rc, lib.zlhip_last_error(e))
        return ids

    plain = load()                                                 # the unconverted bank of the payoff run
    conv_ms, wall_ms, copy_ms, decode_ms = [], [], [], []
    for r in range(a.reps + 1):                                    # the first call is the warm-up (code objects, the table, the records)
        ids = load()
        c, d = syn.upload_pcm_timings()
        t0 = time.perf_counter()
        rc = lib.zlhip_sound_convert_rate_batch(e, ids, K, float(ft))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, lib.zlhip_last_error(e))
        if r == 0:                                                 # the figures are of a call that converts the right thing
            for i in (0, K - 1):
                Lc, Rc = syn.read_clip(ids[i])
                ref = rr.convert(table, fs, ft, (raw[i].astype(np.float64) * 2.0 ** -15).astype(np.float32))
                assert np.array_equal(np.stack([Lc, Rc], axis=1).view(np.uint32), ref.view(np.uint32)), i
                assert syn.clip_info(ids[i]) == {"length": N, "channels": 2, "sample_rate": float(ft), "finite": True, "rendered": False}
        else:
            conv_ms.append(syn.convert_timings()); wall_ms.append(dt); copy_ms.append(c); decode_ms.append(d)
        if r < a.reps:
            for i in range(K):
                assert lib.zlhip_sound_release(e, ids[i]) == 0
    converted = ids
    cm, wm, pm, dm = (float(np.median(v)) for v in (conv_ms, wall_ms, copy_ms, decode_ms))
    res["convert"] = dict(device_ms=cm, call_ms=wm, load_copy_ms=pm, load_decode_ms=dm, device_ms_all=conv_ms, call_ms_all=wall_ms,
                          load_copy_ms_all=copy_ms, ratio_to_copy=cm / pm, bar="device_ms <= load_copy_ms", bar_met=bool(cm <= pm),
                          output_Mframes_per_s=K * N / (cm * 1e-3) / 1e6,
                          tap_pairs_per_s=K * N * T_.value / (cm * 1e-3))

    # ---- the payoff: the same voices on the unconverted and on the converted bank ----------------------------------------------
    def start(bank):
        for v in range(K):
            bus, slot = divmod(v, vpb)
            syn.stop_voice(bus, slot, False)
        for v in range(K):
            p = syn.default_clip_params(n / float(fs))
            p.length_in_beats = 3.5                                # a fractional beat length: a sample-space loop (bench.py's scene)
            p.length_seconds = float(np.float32((n - 64 - (v % 17)) / float(fs)))
            p.volume_absolute = float(np.float32(0.25 + 0.75 * ((v * 37) % 101) / 100.0))
            p.pan = float(np.float32(-1.0 + 2.0 * ((v * 53) % 97) / 96.0))
            syn.set_clip_params(bank[v], p)
        for v in range(K):
            bus, slot = divmod(v, vpb)
            cmd = clip_command(clip=bank[v], midi_note=60, midi_channel=bus - 2, start_playback=1, looping=1, change_volume=1, volume=0.5)
            assert syn.start_voice(bus, slot, cmd, 0) == 1

    def run(bank, first_block):
        start(bank)
        ms, vs = [], 0
        for i in range(2 + a.steps):
            syn.render_batch(KB, NF, synthetic_clocks(KB, NF, float(ft), start_block=first_block + i * KB))
            syn.synchronize()
            t = syn.last_timings()
            if i >= 2:
                ms.append(float(t.render_ms)); vs = int(t.active_voice_frames)
        return ms, vs

    rounds, block = [], 0
    for r in range(a.rounds):
        row = {}
        for name, bank in (("unconverted", plain), ("converted", converted)):
            ms, vs = run(bank, block)
            block += (2 + a.steps) * KB
            row[name] = dict(k2_ms=float(np.median(ms)), k2_ms_all=ms, voice_samples_per_call=vs,
                             voice_samples_per_s=vs / (float(np.median(ms)) * 1e-3) if ms and np.median(ms) > 0 else None)
        row["ratio"] = row["unconverted"]["k2_ms"] / row["converted"]["k2_ms"]
        rounds.append(row)
    res["payoff"] = dict(voices=K, buses=B, frames=NF, blocks_per_call=KB, step_unconverted=fs / ft, rounds=rounds,
                         k2_ms_unconverted=float(np.median([x["unconverted"]["k2_ms"] for x in rounds])),
                         k2_ms_converted=float(np.median([x["converted"]["k2_ms"] for x in rounds])),
                         ratio=float(np.median([x["ratio"] for x in rounds])))
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_resample_kernel_resources.txt")
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
