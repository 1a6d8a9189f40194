"""Engine group (zlhip_group_*) on one box: span and bus-aligned groups of two members on device 0 against one engine of the same shape.

    python scripts/group_bench.py [--calls 6] [--warmup 2] [--blocks 2048] [--devices 0,0]

Shape: 8 buses x 128 voices, 256-frame blocks, 2048 blocks per call, every voice its own looping 2 s stereo clip at the playback rate.  Per
leg: milliseconds per call, queued back to back (wall clock over the timed calls, one synchronize at the end), and the members' K2
time (zlhip_last_timings of each member, profiling on).  The span group's output is checked bit for bit against one engine with
voices_per_task = 64, the bus-aligned group's against one engine with the whole config.  The spanning-bus sum's own kernel time comes
from a `rocprofv3 --kernel-trace --stats` run of this script (zl_k_group_reduce_scan).  One JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libzl_amd import SamplerSynth, SamplerSynthGroup, clip_command, synthetic_clocks  # noqa: E402
from libzl_amd import _abi  # noqa: E402

B, VPB, N = 8, 128, 256


def setup(syn, sources):
    for i, (L, R) in enumerate(sources):
        clip = syn.register_clip(L, R, 48000.0)
        p = syn.default_clip_params(L.shape[0] / 48000.0)
        # bench.py's scene: a fractional beat length (a sample-space loop, not a beat-locked one) a little shorter than the source
        p.length_in_beats = 3.5
        p.length_seconds = float(np.float32((L.shape[0] - 64 - (i % 17)) / 48000.0))
        syn.set_clip_params(clip, p)
    for b in range(B):
        for s in range(VPB):
            cmd = clip_command(clip=(b * VPB + s) % len(sources), midi_note=60, midi_channel=b - 2, start_playback=1, looping=1,
                               change_volume=1, volume=0.01)
            syn.start_voice(b, s, cmd, 0)


def member_render_ms(lib, engines):
    out = []
    for e in engines:
        t = _abi.Timings()
        lib.zlhip_last_timings(e, C.byref(t))
        out.append(round(t.render_ms, 4))
    return out


def run_leg(name, make, engines_of, K, calls, warmup):
    syn = make()
    lib = syn._lib
    setup(syn, SOURCES)
    engines = engines_of(syn)
    for e in engines:
        lib.zlhip_set_profiling(e, 1)
    clocks = [synthetic_clocks(K, N, 48000.0, start_block=i * K) for i in range(calls + warmup)]
    for i in range(warmup):
        syn.render_batch(K, N, clocks[i])
    syn.synchronize()
    t0 = time.perf_counter()
    for i in range(warmup, warmup + calls):
        syn.render_batch(K, N, clocks[i])
    syn.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / calls
    bus = syn.read_bus()
    row = dict(leg=name, buses=B, voices_per_bus=VPB, nframes=N, blocks_per_call=K, calls=calls, ms_per_call=round(ms, 4),
               member_k2_ms_last_call=member_render_ms(lib, engines),
               partial_bus_mb=round(B * 2 * K * N * 4 / 1e6, 2))
    syn.close()
    return row, bus


def main():
    global SOURCES
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--devices", default="0,0")
    a = ap.parse_args()
    devs = [int(x) for x in a.devices.split(",")]
    K = a.blocks
    rng = np.random.default_rng(7)
    # a distinct 2 s stereo source per voice (786 MB per engine), as bench.py's headline
    base = rng.uniform(-1, 1, (2, 96000 + 97 * B * VPB)).astype(np.float32)
    SOURCES = [(base[0, 97 * i:97 * i + 96000], base[1, 97 * i:97 * i + 96000]) for i in range(B * VPB)]
    kw = dict(max_frames=N, max_batch_blocks=K, max_sounds=B * VPB, sound_arena_bytes=900 << 20)

    span, span_bus = run_leg("span", lambda: SamplerSynthGroup(devs, B, VPB, partition="span", **kw),
                             lambda g: [g.member(r) for r in range(g.n)], K, a.calls, a.warmup)
    one_vpt, one_vpt_bus = run_leg("one_engine_vpt", lambda: SamplerSynth(B, VPB, voices_per_task=VPB // len(devs), device=devs[0], **kw),
                                   lambda s: [s.handle], K, a.calls, a.warmup)
    span["bit_exact_vs_one_engine"] = bool(np.array_equal(span_bus.view(np.int32), one_vpt_bus.view(np.int32)))
    span["one_engine_vpt_ms_per_call"] = one_vpt["ms_per_call"]
    print(json.dumps(span), flush=True)
    print(json.dumps(one_vpt), flush=True)

    bus, bus_bus = run_leg("bus_aligned", lambda: SamplerSynthGroup(devs, B, VPB, partition="bus", **kw),
                           lambda g: [g.member(r) for r in range(g.n)], K, a.calls, a.warmup)
    one, one_bus = run_leg("one_engine", lambda: SamplerSynth(B, VPB, device=devs[0], **kw), lambda s: [s.handle], K, a.calls, a.warmup)
    bus["bit_exact_vs_one_engine"] = bool(np.array_equal(bus_bus.view(np.int32), one_bus.view(np.int32)))
    bus["one_engine_ms_per_call"] = one["ms_per_call"]
    print(json.dumps(bus), flush=True)
    print(json.dumps(one), flush=True)


if __name__ == "__main__":
    main()
