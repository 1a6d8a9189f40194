"""The case table of the mode tests (no GPU, no HIP): every value of the engine's `mode` -- ZLHIP_MODE_FIX_GAIN (1), ZLHIP_MODE_FIX_DELAY (2),
ZLHIP_MODE_HERMITE (4) and their sums -- on every non-staged K2 launch shape.  tests/test_modes_cpu.py holds the table to the launch
decision (zl_k2_launch, zl_launch.h: which kernel each row reaches), tests/test_modes_gpu.py runs the rows on the device against the oracle.

A case is (name, mode, scene kwargs for scenario.random_scene, run kwargs for scenario.run_backend, environment).  The scenes are the
smallest that still reach each path: 2-5 buses of at most 16 voices (the `wide` rows: 32-40 voices, the widths of tests/test_rt_fanout.py),
8-16 blocks, the default clip lengths, commands and clip edits between the blocks -- which also cut a run into calls of different lengths.

Environment: ZL_K2_PHASE_ORDER is 2 in the `phase` rows and 0 elsewhere (the default, 1, picks the order from the playing voices, which the
launch decision of a row must not depend on); ZL_K2_PAIR is 0 in the mode-0 rows (the pair kernels exist for mode 0 only and have tests of
their own: tests/test_k2_pair.py); the LDS-staged variants (ZL_K2_STAGED) are withdrawn and never switched on here."""
from __future__ import annotations

from typing import Dict, NamedTuple

from scenario import _segments, random_scene

MODES = tuple(range(8))
FIX_DELAY = 2                                # ZLHIP_MODE_FIX_DELAY
RENDER, PHASE_RENDER = 0, 1                  # ZlK2Kernel (zl_launch.h)
RT_SPLIT_MIN_VOICES = 32                     # ZL_RT_SPLIT_MIN_VOICES (zl_engine.cpp): a single block of a bus this wide is split by voice


class ModeCase(NamedTuple):
    name: str
    mode: int
    scene: Dict
    run: Dict
    env: Dict

    @property
    def id(self):
        return f"{self.name}-mode{self.mode}"

    def make_scene(self):
        return random_scene(**self.scene)


class Shape(NamedTuple):
    scene: Dict                              # random_scene's kwargs but for seed and mode
    run: Dict
    env: Dict
    kernel: int                              # what the name promises: ZlK2Kernel, blocks per workgroup ...
    bpw: int
    scans_levels: bool                       # ... and whether K2 scans the levels itself (else zl_k3_scan / zl_k3_finalize)


NO_ORDER = {"ZL_K2_PHASE_ORDER": "0"}

# name -> shape; what each row reaches is in its comment
SHAPES = {
    # zl_k2_render<m, 4, false>; the last workgroup of the last call holds fewer than four blocks
    "bpw4": Shape(dict(num_buses=3, voices_per_bus=8, nframes=64, nblocks=16), {}, NO_ORDER, RENDER, 4, True),
    # zl_k2_render<m, 2, false>
    "bpw2": Shape(dict(num_buses=4, voices_per_bus=8, nframes=128, nblocks=12), {}, NO_ORDER, RENDER, 2, True),
    # zl_k2_render<m, 1, false>, three buses per workgroup (zl_k2_narrow_buses > 1)
    "bpw1_narrow": Shape(dict(num_buses=3, voices_per_bus=8, nframes=256, nblocks=10), {}, NO_ORDER, RENDER, 1, True),
    # the same kernel, one bus per workgroup, a voice chunk that is not full
    "bpw1_single_bus": Shape(dict(num_buses=2, voices_per_bus=5, nframes=256, nblocks=10), {}, NO_ORDER, RENDER, 1, True),
    # 128 lanes for 100 frames: lanes behind the block's end
    "partial_wave": Shape(dict(num_buses=3, voices_per_bus=8, nframes=100, nblocks=12), {}, NO_ORDER, RENDER, 1, True),
    # two workgroups per block (gx = 2), the levels from zl_k3_scan
    "two_tiles": Shape(dict(num_buses=2, voices_per_bus=8, nframes=512, nblocks=8), {}, NO_ORDER, RENDER, 1, False),
    # ragged tiles: 441 = 256 + 185
    "ragged": Shape(dict(num_buses=3, voices_per_bus=8, nframes=441, nblocks=8), {}, NO_ORDER, RENDER, 1, False),
    # two mix groups per bus: partial rows and zl_k3_finalize
    "mix_groups": Shape(dict(num_buses=2, voices_per_bus=8, nframes=256, nblocks=10, mix_group=4), {}, NO_ORDER, RENDER, 1, False),
    # zl_k2_phase_render<m>
    "phase": Shape(dict(num_buses=2, voices_per_bus=16, nframes=256, nblocks=12, nclips=14), {}, {"ZL_K2_PHASE_ORDER": "2"}, PHASE_RENDER, 1, True),
    # the K = 1 launch of a batch call
    "single_blocks": Shape(dict(num_buses=3, voices_per_bus=8, nframes=128, nblocks=8), dict(batch=1), NO_ORDER, RENDER, 1, True),
    # ... of a wide bus: one voice per workgroup, summed by zl_k3_finalize
    "wide_single_blocks": Shape(dict(num_buses=2, voices_per_bus=40, nframes=128, nblocks=8, nclips=30), dict(batch=1), NO_ORDER, RENDER, 1, False),
}


LAST_CALL_MIN = 3                            # blocks of a row's last call: the level checks see a first, a middle and a last block


def _last_call_fits(sh, kw):
    """The level checks of the GPU tier read the LAST call of a row (block_peaks, levels_tick), and a call of one block is always
    zl_k2_render<m, 1, false> with one bus per workgroup and no order.  So a row that renders several blocks per call takes the first seed
    whose commands leave a last call of LAST_CALL_MIN blocks or more -- the kernel the name says, checked for its levels too -- and, with
    several blocks per workgroup, one whose last workgroup is not full."""
    if sh.run.get("batch") == 1:
        return True
    K = _segments(random_scene(**kw), 1 << 30)[-1][1]
    return K >= LAST_CALL_MIN and (sh.bpw == 1 or K % sh.bpw != 0)


def _case(name, mode, i):
    sh = SHAPES[name]
    env = dict(sh.env)
    if mode == 0:
        env["ZL_K2_PAIR"] = "0"
    kw = dict(sh.scene, seed=0x3D00 + 8 * i + mode, mode=mode)
    while not _last_call_fits(sh, kw):
        kw["seed"] += 0x1000
    return ModeCase(name, mode, kw, dict(sh.run), env)


BATCH_CASES = [_case(name, mode, i) for i, name in enumerate(SHAPES) for mode in MODES]


def case_id(c):
    return c.id


def calls(case):
    """(first block, blocks) of every render call of the case, as scenario.run_backend cuts it"""
    return _segments(case.make_scene(), case.run.get("batch", 1 << 30))


def mix_groups(scene_kw, K):
    """mix groups per bus of a call of K blocks (pick_group, zl_engine.cpp): the scene's voices_per_task, else one voice per group for a
    single block of a wide bus, else the whole bus"""
    vpb, g = scene_kw["voices_per_bus"], scene_kw.get("mix_group", 0)
    G = min(g, vpb) if g > 0 else 1 if (K == 1 and vpb >= RT_SPLIT_MIN_VOICES) else vpb
    return (vpb + G - 1) // G


# ---- bounce (zlhip_bounce): the modes with ZLHIP_MODE_FIX_DELAY, and 5 and 0 as controls -------------------------------------------------
BOUNCE_MODES = (2, 3, 6, 7, 5, 0)
# frames per block -> (blocks per sub-batch of the bounce, how the copy-engine delivery is asked for): ragged sub-batches, both ways
BOUNCE_SHAPES = {64: (5, "env"), 128: (3, "pageable"), 256: (4, "env"), 100: (7, "pageable"), 441: (3, "env")}


def bounce_scene(mode, nframes):
    return random_scene(0x3E00 + 8 * sorted(BOUNCE_SHAPES).index(nframes) + mode, num_buses=3, voices_per_bus=8, nframes=nframes, nblocks=13, mode=mode)


# ---- the resident real-time kernel (ZL_RT_PERSISTENT=1): scene kwargs and period, 24 cycles each -------------------------------------------
RT_CYCLES = 24
RT_NARROW = (dict(num_buses=4, voices_per_bus=8, nclips=14), 128)
RT_NARROW_100 = (dict(num_buses=4, voices_per_bus=8, nclips=14), 100)
RT_WIDE = (dict(num_buses=2, voices_per_bus=40, nclips=50), 128)          # tests/test_rt_fanout.py, wide_resident
RT_CASES = [("narrow", m) + RT_NARROW for m in MODES] + [("narrow_100", m) + RT_NARROW_100 for m in (6, 7)] + [("wide", m) + RT_WIDE for m in MODES]


def rt_scene(what, mode, kw, period):
    return random_scene(0x3F00 + 8 * ("narrow", "narrow_100", "wide").index(what) + mode, nframes=period, nblocks=RT_CYCLES, mode=mode, **kw)


# ---- the fused fan-out with ZLHIP_MODE_FIX_DELAY ------------------------------------------------------------------------------------------------
FANOUT_BATCH = [(name, mode) for name in ("bpw2", "bpw1_narrow", "mix_groups") for mode in (3, 6, 7)]
FANOUT_RT = [(what, mode) for what in ("narrow", "wide") for mode in (6, 7)]
