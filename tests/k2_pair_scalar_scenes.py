"""The scenes of tests/test_k2_pair_scalar.py (GPU) and tests/test_k2_pair_scalar_cpu.py (which makes, with the host planner, the scalar records
K1c leaves for each scene and counts the workgroups of zl_k2_pair_phase_render that skip staging): loops at the playback rate in buses of
8 to 128 voices, blocks of 256 frames, calls of at most 96 blocks.

A voice is a dict: loop = frames of the loop, start = its first frame in the source, tail = source frames behind the loop's last, stereo,
note, src(L, R, start, stop) edits the source in place, idle = the clip is never played, oneshot = the source is played once (loop = its
frames), decay = a decay of one second.  A fast workgroup needs every voice of its bus on one segment in the block, so the wide buses are
made of loops whose length is a whole number of blocks (they restart on block boundaries: one segment in every block) and a few that are not.
One bus of 8 or 16 voices per scene, or buses wider than 64: two narrow buses would be packed into one workgroup, which the pair kernels do
not take (tests/test_k2_pair_scalar_cpu.py holds every scene's shape to the launch table).  Start and length are given a quarter of a frame
over the integer, so the float seconds truncate to it."""
import ctypes as C

import numpy as np

from scenario import Scene, play_cmd, rand_source

FS = 48000.0
N = 256


def build(seed, voices, *, num_buses, vpb, calls, call, events=None, bpm=120, src_frames=0):
    rng = np.random.default_rng(seed)
    sc = Scene(num_buses=num_buses, voices_per_bus=vpb, fs=FS, mode=0, mix_group=0, nframes=N, nblocks=calls * call, bpm=bpm)
    assert len(voices) == num_buses * vpb
    for i, vo in enumerate(voices):
        loop, start, tail = vo["loop"], vo.get("start", 0), vo.get("tail", 300)
        L, R = rand_source(rng, max(start + loop + tail, src_frames), stereo=vo.get("stereo", True))
        if "src" in vo:
            vo["src"](L, R, start, start + loop)
        sc.sounds.append((L, R, FS))
        st = float(np.float32((start + 0.25) / FS)) if start else 0.0
        length = float(np.float32(loop / FS)) if start else float(np.float32((loop + 0.25) / FS))
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))

        def setup(lib, clip, st=st, length=length, vol=vol, pan=pan, loops="oneshot" not in vo, slow=vo.get("decay", False)):
            if loops:
                lib.zlo_clip_set_start_position(clip, C.c_float(st))
                clip.lengthInBeats = 0.3                              # fractional: a sample-space loop
                clip.lengthInSeconds = length
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
            if slow:
                clip.adsr.p.attack, clip.adsr.p.decay, clip.adsr.p.sustain, clip.adsr.p.release = 0.0, 1.0, 0.5, 0.0
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // vpb - 2, loop="oneshot" not in vo, note=vo.get("note", 60),
                                     volume=float(np.float32(rng.uniform(0.2, 1.0)))), 0)
                    for i, vo in enumerate(voices) if not vo.get("idle")]
    for k, evs in (events or {}).items():
        sc.events.setdefault(k, []).extend(evs)
    sc.call = call
    return sc


def _inf_behind_the_loop(L, R, start, stop):
    L[stop + 40] = np.inf                                            # never played, never a tap: the source is still not "finite"


def whole(j):
    """a loop of a whole number of blocks (3 to 6): it restarts on a block boundary, every block of it is one segment"""
    return dict(loop=N * (3 + j % 4), start=(0, 3, 4, 77, 78, 5, 6, 9)[j % 8])


def ragged(j):
    """a loop of 600 to 1500 frames that is no multiple of the block: it restarts inside a block every few blocks"""
    return dict(loop=600 + (j * 131) % 900 + (1 if (600 + (j * 131) % 900) % N == 0 else 0), start=(0, 3, 4, 77, 78, 5, 6, 9)[j % 8])


def _set_pan(value):
    def fn(lib, clip):
        lib.zlo_clip_set_pan(clip, C.c_float(value))
    return fn


def _set_volume(value):
    def fn(lib, clip):
        lib.zlo_clip_set_volume_absolute(clip, C.c_float(value))
    return fn


CALL = 48                                                            # blocks per call: more passes of every loop than a run list holds


def _negative(offender):
    """chunk 0 holds the offending voice (slot 3) among whole-block loops, chunk 1 is fast in every block: the workgroup must stage"""
    return dict(num_buses=1, vpb=16, calls=2, call=CALL, voices=[dict(whole(j), **offender) if j == 3 else whole(j) for j in range(16)])


SCENES = {
    # one bus of 8 / of 16 ragged loops over three calls: the first call has inline runs (k < run_end), from the second on there are none
    "bus_8": dict(num_buses=1, vpb=8, calls=3, call=CALL, voices=[ragged(j) for j in range(8)]),
    "bus_16": dict(num_buses=1, vpb=16, calls=3, call=CALL, voices=[whole(j) if j % 2 else ragged(j) for j in range(16)]),
    # 128 voices: two K1c waves feed one workgroup; 72: the bus ends inside a K1c wave; two buses of 72: bus 1 begins inside one, at a chunk boundary
    "bus_128": dict(num_buses=1, vpb=128, calls=2, call=CALL, voices=[ragged(j) if j in (5, 70, 127) else whole(j) for j in range(128)]),
    "bus_72": dict(num_buses=1, vpb=72, calls=2, call=CALL, voices=[ragged(j) if j in (9, 71) else whole(j) for j in range(72)]),
    "two_buses_72": dict(num_buses=2, vpb=72, calls=2, call=CALL, voices=[ragged(j) if j in (9, 71, 72, 143) else whole(j) for j in range(144)]),
    # a restart inside the block: voice 0 restarts in about every second block (loop 500), voice 1's loop ends on a block's last frame (1024),
    # voice 2 restarts one frame into a block and voice 3 one frame before its end (every fifth block); the blocks before and after a restart are fast
    "restarts": dict(num_buses=1, vpb=8, calls=2, call=CALL,
                     voices=[dict(loop=500, start=2), dict(loop=1024, start=0), dict(loop=1281, start=5), dict(loop=1279, start=8)] + [whole(j) for j in range(4, 8)]),
    # one voice of a chunk not fast, the other chunk of the bus fast
    "neg_pitched": _negative(dict(note=67)),
    "neg_mono_among_stereo": _negative(dict(stereo=False)),
    "neg_not_finite": _negative(dict(src=_inf_behind_the_loop)),
    "neg_decay": _negative(dict(decay=True)),
    "neg_idle": _negative(dict(idle=True)),
    "neg_oneshot": _negative(dict(oneshot=True, loop=20 * N + 77)),           # ends in block 20 of the first call: dead_from inside the window
    # an all-mono bus: the fast path with 8-byte loads
    "all_mono": dict(num_buses=1, vpb=8, calls=2, call=CALL, voices=[dict(whole(j) if j % 3 else ragged(j), stereo=False) for j in range(8)]),
    # sources of 50000 frames in an arena of 1 MiB: the later ones land in grown segments, wherever the allocator put them
    "grown_arena": dict(num_buses=1, vpb=8, calls=2, call=CALL, src_frames=50000, voices=[dict(whole(j), start=40000 + j) for j in range(8)]),
}
# the commands between calls: the record sets alternate across calls, nothing of an earlier call's records may be read
SCENES["edits"] = dict(num_buses=1, vpb=8, calls=5, call=CALL, voices=[whole(j) for j in range(8)], events={
    # a hard stop and the same clip again on the same slot (an idle slot would keep the bus off the fast path for good), a pan knob
    CALL: [("stopv", 0, 2, False), ("start", 0, 2, play_cmd(2, midi_channel=-2, loop=True, note=60, volume=0.5), 0), ("clip", 5, _set_pan(-0.65))],
    2 * CALL: [("update", 0, 3, dict(clip=3, midiChannel=-2, midiNote=60, changeVolume=1, volume=0.37)), ("clip", 1, _set_volume(0.55))],
    3 * CALL: [("enable", 0, False)],
    4 * CALL: [("enable", 0, True)],
})
POSITIVE = ("bus_8", "bus_16", "bus_128", "bus_72", "two_buses_72", "restarts", "all_mono", "grown_arena", "edits")
NEGATIVE = tuple(n for n in SCENES if n.startswith("neg_"))
ARENA_BYTES = {"grown_arena": 1 << 20}
# the chunk of the negative scene's bus that holds the offender: slot 3, chunk 0 -- but commands fill a bus's slots in order, so the slot
# that stays idle is the bus's last one, in chunk 1
OFFENDING_CHUNK = {"neg_idle": 1}


def scene(name):
    cfg = dict(SCENES[name])
    voices = [dict(v) for v in cfg.pop("voices")]
    return build(0x3D00 + sorted(SCENES).index(name), voices, **cfg)
