"""Key detection (zlhip_sound_key_batch): one 30 s stereo clip at 48 kHz with the defaults in a call of its own, and a bank of 256 such
clips in ONE call; for each the median of `reps` calls after a warm-up call, profiling on -- the device time of the three launches
(zlhip_debug_key_timings: gate, correlate, fold), the host wall time of the call and the integer multiply-adds per second of the
correlate kernel (two per term: v c and v s; the window's m w is not counted).  A call is the same three launches for one request and
for 256: the call scaffold queues each launcher once, and the three stage times are all there is to report for either.
In the same session and on the same clip:
    ref        the same single-clip call in tests/key_ref.py (numpy and Python integers, one thread), fed with the library's table; its
               result must equal the device's
Prints one JSON line.

    python scripts/key_bench.py [--bank 256] [--seconds 30] [--reps 5] [--distinct 8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clip(rng, n, sr):
    """a chord loop in a key of its own: I-IV-V-I or i-iv-v-i repeated over the clip, triads with four harmonics and a bass, the channels'
    phases differ, over a quiet noise floor"""
    tonic, minor = int(rng.integers(0, 12)), int(rng.integers(0, 2))
    t = np.arange(n) / sr
    x = rng.uniform(-0.002, 0.002, (2, n))
    seg = int(0.75 * sr)
    for k in range(0, n, seg):
        root = 48 + tonic + (0, 5, 7, 0)[(k // seg) % 4]
        tt = t[k:k + seg]
        for note in (root - 12, root, root + (3 if minor else 4), root + 7):
            f = 440.0 * 2.0 ** ((note - 69.0) / 12.0)
            for c in range(2):
                for h in range(1, 5):
                    x[c, k:k + seg] += (0.08 / h) * np.sin(2.0 * np.pi * h * f * tt + 0.7 * c)
    return x.astype(np.float32), (tonic, minor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bank", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=float, default=48000.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()

    import key_ref as kr
    from libzl_amd import SamplerSynth, _abi
    n = int(a.seconds * a.sr)
    syn = SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=a.bank + 8, sound_arena_bytes=(n + 16) * 8 * a.bank + (1 << 20))
    rng = np.random.default_rng(a.seed)
    made = [clip(rng, n, a.sr) for _ in range(min(a.distinct, a.bank))]
    ids = [syn.register_clip(made[i % len(made)][0][0], made[i % len(made)][0][1], a.sr) for i in range(a.bank)]
    syn.set_profiling(True)
    bins, T = kr.library_table(_abi.load(), a.sr)
    per_frame = sum(b[1] for b in bins)

    def measure(reqs):
        gate, corr, fold, wall = [], [], [], []
        for r in range(a.reps + 1):                                # the first call is the warm-up (code objects, the call's buffers)
            t0 = time.perf_counter()
            got = syn.clip_key_batch(reqs)
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                wall.append(dt)
                t = syn.key_timings()
                gate.append(t[0]); corr.append(t[1]); fold.append(t[2])
        frames = sum(g["sounding"] for g in got)
        terms = frames * per_frame
        cm = float(np.median(corr))
        return got, dict(requests=len(reqs), launches=3, frames=sum(g["frames"] for g in got), work_items=sum(g["frames"] for g in got) * -(-len(bins) // 8), terms=terms,
                         gate_ms=float(np.median(gate)), correlate_ms=cm, fold_ms=float(np.median(fold)), call_ms=float(np.median(wall)),
                         correlate_ms_all=corr, call_ms_all=wall, correlate_Gmacs=2 * terms / (cm * 1e-3) / 1e9, host_bytes=136 * len(reqs))

    one, r1 = measure([(ids[0],)])
    bank, rb = measure([(cid,) for cid in ids])
    right = sum((g["tonic"], g["mode"]) == made[i % len(made)][1] for i, g in enumerate(bank))
    res = dict(metric="sound_key", device=syn.device_name(), seconds=a.seconds, sr=a.sr, reps=a.reps, bins=len(bins), span=bins[0][1], terms_per_frame=per_frame,
               one=r1, bank=rb, bank_right_keys=int(right), bank_min_confidence=float(min(g["confidence"] for g in bank)))
    t0 = time.perf_counter()
    want = kr.key(made[0][0], a.sr, bins, T)[0]
    res["ref"] = dict(route="tests/key_ref.py on one host thread, one clip", ms=(time.perf_counter() - t0) * 1e3)
    res["ref"]["ratio_to_call"] = res["ref"]["ms"] / r1["call_ms"]
    res["ref"]["bank_ms_extrapolated"] = res["ref"]["ms"] * a.bank
    assert all(one[0][k] == want[k] for k in want), (one[0], want)                # the figures are of two routes that compute the same thing
    assert bank[0] == one[0]
    syn.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
