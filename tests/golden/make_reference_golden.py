#!/usr/bin/env python3
"""Records tests/golden/ref_*.npz from the reference's OWN voice: the scenes of tests/reference_scenes.FIXTURES played through
oracle/_ref/libzl_refvoice.so (the reference's SamplerSynthVoice.cpp compiled unmodified: libzl_amd/build.py build_reference).
Each file holds the inputs in the layout of the g*.npz goldens (sources, clip fields, commands, clocks: tests/golden_util.py) and what
the reference voice gave: both buffers of every channel, the frame it stores to [nframes], every block's reports, isPlaying after
every block.  Arrays and settings only.  Needs the reference tree; run from the repository root:
    python tests/golden/make_reference_golden.py
tests/test_reference_golden_cpu.py re-records every fixture in memory where the library is available and holds the file to it."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden_util import _MAP  # noqa: E402

_KEY = {v: k for k, v in _MAP.items()}          # the oracle's ClipCommand field -> the goldens' event key


def _fields(f):
    return {_KEY[k]: v for k, v in f.items()}


def _event(ev):
    if ev[0] == "cmd":
        return dict(_fields(ev[1]), tick=int(ev[2]))
    if ev[0] == "start":
        return dict(_fields(ev[3]), kind="start", bus=ev[1], slot=ev[2], tick=int(ev[4]))
    if ev[0] == "update":
        return dict(_fields(ev[3]), kind="update", bus=ev[1], slot=ev[2])
    if ev[0] == "stopv":
        return dict(kind="stopv", bus=ev[1], slot=ev[2], tail=bool(ev[3]))
    if ev[0] == "enable":
        return dict(kind="enable", bus=ev[1], on=bool(ev[2]))
    raise ValueError(f"a {ev[0]!r} event cannot be stored")


def record(name, sc, lib_path=None):
    """-> the arrays of one fixture (what np.savez_compressed writes)"""
    import ctypes as C
    import ref_voice as rv
    from oracle import zl_oracle as zo
    out = rv.run_reference(sc, lib_path)["ref"]
    osyn = zo.OracleSynth(1, 1, sc.fs, 0, max_sounds=max(8, len(sc.sounds)))          # only its clip structs, for the stored clip fields
    clips = []
    for i, (L, R, sr) in enumerate(sc.sounds):
        osyn.register_clip(L, R, sr)
        if i in sc.clip_setup:
            sc.clip_setup[i](osyn.lib, osyn.clips[i])
        c = osyn.clips[i]
        clips.append(dict(start_sec=c.startPositionInSeconds, length_sec=c.lengthInSeconds, length_beats=c.lengthInBeats, volume_abs=c.volumeAbsolute,
                          pan=c.pan, duration=c.duration, root_note=c.rootNote, slice_pos=[c.slicePositions[j] for j in range(c.nSlicePositions)],
                          adsr=[c.adsr.p.attack, c.adsr.p.decay, c.adsr.p.sustain, c.adsr.p.release]))
    ck = sc.make_clocks(0, sc.nblocks)
    clocks = np.array([[c.current_usecs, c.next_usecs, c.jack_playhead, c.jack_playhead_usecs, c.jack_subbeat_length_usecs] for c in ck], dtype=np.uint64)
    meta = dict(name=name, B=sc.num_buses, VPB=sc.voices_per_bus, fs=sc.fs, mode=0, nframes=sc.nframes, nblocks=sc.nblocks, bpm=sc.bpm,
                events={str(k): [_event(ev) for ev in evs] for k, evs in sorted(sc.events.items())}, clips=clips,
                sample_rates=[s[2] for s in sc.sounds], stereo=[s[1] is not None for s in sc.sounds],
                source="reference lib/SamplerSynthVoice.cpp compiled unmodified, x86-64, -O2 -ffp-contract=off")
    arrays = dict(meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), busL=out["bus"][:, 0, :].copy(), busR=out["bus"][:, 1, :].copy(),
                  tail=out["tail"], reports=out["reports"], playing=out["playing"], clocks=clocks)
    for i, (L, R, sr) in enumerate(sc.sounds):
        arrays[f"snd{i}_L"] = np.asarray(L, dtype=np.float32)
        if R is not None:
            arrays[f"snd{i}_R"] = np.asarray(R, dtype=np.float32)
    return arrays


def main():
    import reference_scenes as rs
    for name, make in rs.FIXTURES.items():
        arrays = record(name, make())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        peak = np.nanmax(np.abs(np.stack([arrays["busL"], arrays["busR"]])))
        print(f"{name}: peak |x| = {peak:.4g} -> {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
