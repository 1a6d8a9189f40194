"""The scenes of tests/test_k2_pair_wrap.py (GPU) and tests/test_k2_pair_wrap_cpu.py (which counts, with the host planner, the voice-blocks
of each scene that the pair kernels take on the one-tap path): loops at the playback rate whose restarts fall inside 256-frame blocks.

A voice is a dict: loop = frames of the loop, start = its first frame in the source, tail = source frames behind the loop's last (0: the
loop ends at the source's last frame), stereo, note, beats (an integer lengthInBeats: restarts by the clock), src(L, R, start, stop) edits
the source in place.  Every scene is ONE bus of 8 or 16 voices (one or two chunks of 8): with two buses of 8 the launch packs two buses into a
workgroup (zl_k2_narrow_buses), which the pair kernels do not take (zl_pair_shape; tests/test_k2_pair_wrap_cpu.py holds every scene's shape
to the launch table).  A voice started at frame 0 of the scene restarts at scene frames loop, 2 loop, ...: in block j loop // 256 at
n1 = j loop % 256.  Start and length are given a quarter of a frame over the integer, so the float seconds truncate to it."""
import ctypes as C

import numpy as np

from scenario import Scene, play_cmd, rand_source
from test_k2_ongrid import ADVERSARIAL

FS = 48000.0
N = 256
STEADY = dict(loop=20000)                                            # never restarts inside a scene: on-grid, one segment, in every block


def build(seed, voices, *, num_buses, vpb, nblocks, bpm=120):
    rng = np.random.default_rng(seed)
    sc = Scene(num_buses=num_buses, voices_per_bus=vpb, fs=FS, mode=0, mix_group=0, nframes=N, nblocks=nblocks, bpm=bpm)
    assert len(voices) == num_buses * vpb
    for i, vo in enumerate(voices):
        loop, start, tail = vo["loop"], vo.get("start", 0), vo.get("tail", 300)
        L, R = rand_source(rng, start + loop + tail, stereo=vo.get("stereo", True))
        if "src" in vo:
            vo["src"](L, R, start, start + loop)
        sc.sounds.append((L, R, FS))
        st = float(np.float32((start + 0.25) / FS)) if start else 0.0
        length = float(np.float32(loop / FS)) if start else float(np.float32((loop + 0.25) / FS))
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))

        def setup(lib, clip, st=st, length=length, vol=vol, pan=pan, beats=vo.get("beats")):
            lib.zlo_clip_set_start_position(clip, C.c_float(st))
            clip.lengthInBeats = float(beats) if beats else 0.3      # fractional: a sample-space loop
            clip.lengthInSeconds = length
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // vpb - 2, loop=True, note=vo.get("note", 60), volume=float(np.float32(rng.uniform(0.2, 1.0)))), 0)
                    for i, vo in enumerate(voices)]
    return sc


def _adversarial(L, R, start, stop):
    """the adversarial finite values on both sides of the restart: the loop's last frames, the frames behind them, and its first"""
    for x in (L, R):
        if x is None:
            continue
        for a, b in ((stop - 6, stop + 3), (start, start + 6)):
            x[a:b] = ADVERSARIAL[(np.arange(a, b) * 7 + (3 if x is R else 0)) % len(ADVERSARIAL)]


def _non_finite_behind_the_loop(L, R, start, stop):
    L[stop + 40] = np.inf; R[stop + 41] = np.nan                     # never played, never a tap: the source is still not "finite"


# n1 of the first restart = loop % 256 (loops of 4 blocks and a bit: all of them restart in block 4, then apart)
RESIDUES = (1, 2, 127, 128, 129, 254, 255)

SCENES = {
    # every listed n1, odd and even; loop start 0 of the clip registered first, odd and even starts; seven voices restart in block 4
    "n1_values": dict(num_buses=1, vpb=8, nblocks=32, voices=[dict(loop=1024 + r, start=(0, 3, 4, 77, 78, 5, 6)[j]) for j, r in enumerate(RESIDUES)] + [STEADY]),
    # a mono chunk, all eight restarting in block 4; loop start 0 first in the arena, odd starts (4-byte aligned pair loads)
    "mono_all_eight": dict(num_buses=1, vpb=8, nblocks=24, voices=[dict(loop=1024 + r, start=(0, 1, 2, 3, 9, 10, 11, 12)[j], stereo=False)
                                                                   for j, r in enumerate((1, 3, 127, 129, 255, 100, 2, 254))]),
    # chunk 0: seven stereo voices and a mono one (a mixed-layout chunk: general); chunk 1: a pitched voice among restarting ones (general)
    "mixed_and_pitched": dict(num_buses=1, vpb=16, nblocks=24,
                              voices=[dict(loop=1100 + 37 * j, start=j, stereo=j != 5) for j in range(8)]
                              + [dict(loop=1300 + 41 * j, start=2 * j, note=67 if j == 2 else 60) for j in range(8)]),
    # chunk 0: a loop shorter than a block (more than two segments in every block); chunk 1: a loop that ends at the source's last frame
    "short_and_edge": dict(num_buses=1, vpb=16, nblocks=24,
                           voices=[dict(loop=100 if j == 3 else 900 + 53 * j, start=j) for j in range(8)]
                           + [dict(loop=1500 + 29 * j, start=j, tail=0 if j == 6 else 300) for j in range(8)]),
    # chunk 0: a source with a non-finite sample (its flag is off); chunk 1: loops of one beat that restart by the clock (600 bpm: 4800 frames)
    "non_finite_and_beat": dict(num_buses=1, vpb=16, nblocks=40, bpm=600,
                                voices=[dict(loop=1200 + 31 * j, start=j, src=_non_finite_behind_the_loop if j == 1 else None) for j in range(8)]
                                + [dict(loop=5280, start=j, beats=1) if j < 3 else dict(loop=2000 + 17 * j, start=j) for j in range(8)]),
    # restarts in the last block of each call (blocks 15 and 31 of two calls of 16): the report path; 16 voices, two chunks
    "last_block": dict(num_buses=1, vpb=16, nblocks=32,
                       voices=[dict(loop=15 * 256 + 77, start=3), dict(loop=31 * 256 + 5, start=0), dict(loop=15 * 256 + 200, start=8), dict(loop=14 * 256 + 9, start=1)]
                       + [STEADY] * 4 + [dict(loop=31 * 256 + 130, start=2)] + [STEADY] * 7),
    # the adversarial finite values around the restart, stereo and (chunk 1) mono
    "adversarial": dict(num_buses=1, vpb=16, nblocks=24,
                        voices=[dict(loop=1024 + r, start=j, src=_adversarial) for j, r in enumerate((1, 2, 127, 128, 129, 254, 255, 64))]
                        + [dict(loop=1024 + r, start=j, stereo=False, src=_adversarial) for j, r in enumerate((255, 254, 129, 128, 127, 2, 1, 33))]),
}


def scene(name):
    cfg = dict(SCENES[name])
    voices = [dict(v) for v in cfg.pop("voices")]
    for v in voices:
        if v.get("src") is None:
            v.pop("src", None)
    return build(0x3B00 + sorted(SCENES).index(name), voices, **cfg)


def calls(sc):
    """two calls"""
    return sc.nblocks // 2
