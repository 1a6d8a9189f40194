"""The scenes of tests/test_k2_pair_laps.py (GPU) and tests/test_k2_pair_laps_cpu.py (which counts, from the host planner's records and the host
order, the workgroups of zl_k2_pair_phase_render that take the two-slot walk): built with tests/k2_pair_scalar_scenes.py's builder -- loops at the
playback rate, blocks of 256 frames -- in calls of at most 48 blocks.

A workgroup takes the walk when both of its blocks are fast (every voice of the bus on one segment, on-grid, one layout; behind run_end; not the
call's last block), so the positive scenes are made of loops of a whole number of blocks with a few that are not: those restart inside a block
every few blocks, which gives workgroups of one fast block and one with a restart.  The first call of a scene has inline runs: run_end lies
inside it, one block of a workgroup in front of it and one behind."""
import k2_pair_scalar_scenes as base
from k2_pair_scalar_scenes import N, ragged, whole

CALL = 48


def long_ragged(j):
    """a loop of 1300 to 1500 frames that is no multiple of the block: a restart inside a block about every sixth block"""
    return dict(loop=1301 + 37 * (j % 6), start=(0, 3, 4, 77)[j % 4])


def far(j):
    """loops of 1, 3, 5 and 7 blocks: the lengths differ by two blocks and more, so after one lap phase neighbours share no line of these voices
    (longer loops stay inline runs for whole calls of 48 blocks: run_end is then the call's end and nobody is fast)"""
    return dict(loop=N * (1 + 2 * (j % 4)), start=(0, 3, 4, 77, 78, 5, 6, 9)[j % 8])


def short(j):
    """loops shorter than a block (90 to 230 frames): a restart in every block"""
    return dict(loop=90 + 20 * j, start=(0, 3, 4, 77, 78, 5, 6, 9)[j % 8])


SCENES = {
    # the bus widths: 8 (the pair kernels' smallest launch), 16, 128, two buses of 72 (bus 1 begins inside a K1c wave)
    "bus_8": dict(num_buses=1, vpb=8, calls=3, call=CALL, voices=[long_ragged(j) if j == 5 else whole(j) for j in range(8)]),
    "bus_16": dict(num_buses=1, vpb=16, calls=3, call=CALL, voices=[long_ragged(j) if j in (2, 11) else whole(j) for j in range(16)]),
    "bus_128": dict(num_buses=1, vpb=128, calls=2, call=CALL, voices=[long_ragged(j) if j in (5, 70, 127) else whole(j) for j in range(128)]),
    "two_buses_72": dict(num_buses=2, vpb=72, calls=2, call=CALL, voices=[long_ragged(j) if j in (9, 71, 72, 143) else whole(j) for j in range(144)]),
    # 47 blocks: the bus's last workgroup holds one block
    "blocks_47": dict(num_buses=1, vpb=16, calls=3, call=47, voices=[long_ragged(j) if j == 7 else whole(j) for j in range(16)]),
    # the restarts of k2_pair_scalar_scenes: restarts one frame into a block, one frame before its end, on a block's last frame
    "restarts": dict(base.SCENES["restarts"]),
    # an all-mono bus: the mono walk
    "all_mono": dict(num_buses=1, vpb=8, calls=2, call=CALL, voices=[dict(long_ragged(j) if j == 3 else whole(j), stereo=False) for j in range(8)]),
    # neighbours that share no line after the first lap
    "far_apart": dict(num_buses=1, vpb=8, calls=2, call=CALL, voices=[far(j) for j in range(8)]),
    # stop and restart, update, disable / enable and clip edits between five calls
    "edits": dict(base.SCENES["edits"]),
    # ---- no workgroup takes the walk
    # two blocks: one workgroup, and it holds the call's last block; one block: the pair kernels do not take the launch at all
    "blocks_2": dict(num_buses=1, vpb=8, calls=4, call=2, voices=[whole(j) for j in range(8)]),
    "blocks_1": dict(num_buses=1, vpb=8, calls=6, call=1, voices=[whole(j) for j in range(8)]),
    # chunk 0 stereo, chunk 1 mono: every chunk fast, two layouts -- the workgroups stage
    "mono_and_stereo_chunks": dict(num_buses=1, vpb=16, calls=2, call=CALL, voices=[dict(whole(j), stereo=j < 8) for j in range(16)]),
    "short_loops": dict(num_buses=1, vpb=8, calls=2, call=CALL, voices=[short(j) for j in range(8)]),
    "not_finite": dict(num_buses=1, vpb=8, calls=2, call=CALL, voices=[dict(whole(j), src=base._inf_behind_the_loop) if j == 3 else whole(j) for j in range(8)]),
}
POSITIVE = ("bus_8", "bus_16", "bus_128", "two_buses_72", "blocks_47", "restarts", "all_mono", "far_apart", "edits")
NEGATIVE = tuple(n for n in SCENES if n not in POSITIVE)


def scene(name):
    cfg = dict(SCENES[name])
    voices = [dict(v) for v in cfg.pop("voices")]
    return base.build(0x4C00 + sorted(SCENES).index(name), voices, **cfg)
