"""Warp, GPU tier: the kernels of libzl_amd/csrc/zl_warp.hip against the numpy / Python-integer restatement (tests/warp_ref.py), bit for
bit and with no tolerance: the whole grid of tests/warp_cases.py in ONE call -- the data from read_clip, the whole extent including the
zero frames and the pad in an arena that held noise, the seek offsets, the result records --, periodic clips whose candidates tie,
ZL_SOUND_FINITE from both sides, a loud neighbour, and playback against the oracle over the restatement's data.  The engine around the
call is tests/test_warp_edges_gpu.py's."""
import ctypes as C
import os

import numpy as np
import pytest

import warp_cases as wc
import warp_ref as wr
from warp_cases import check_call, dirty, mismatch, upload

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SR = 48000.0


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=64, sound_arena_bytes=8 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def test_the_grid_in_one_call(built):
    grid = wc.grid()
    with make() as s:
        dirty(s, 400000)
        ids = [upload(s, c["x"], c["rate"]) for c in grid]
        before = s.memory_bytes()[1]
        bad, outs = check_call(s, grid, ids)
        assert not bad, bad
        assert [o["applied"] for o in outs].count(0) == 4
        for cid, c in zip(ids, grid):
            summary, y, offs, _ = wc.want(c)
            L, R = s.read_clip(cid)
            got = np.stack([L, R]) if R is not None else L[None, :]
            assert wc.same_bits(got, y), c["tag"]
            info = s.clip_info(cid)
            assert (info["length"], info["channels"], info["sample_rate"], info["finite"], info["rendered"]) == (summary["length"], c["x"].shape[0], c["rate"], True, False), c["tag"]
            if "expect_off2" in c:
                assert int(s.warp_offsets(cid)[2]) == c["expect_off2"]
        assert s.memory_bytes()[1] == before                       # the arena did not grow: the old extents went back


def test_periodic_clips_whose_candidates_tie(built):
    """rerender_cases.tie_source in two stretched regions: the candidates o, o + P, ... score the same to the bit; P = 37: in different
    lanes of one wave, P = 64: the same lane of neighbouring waves, P = 512: one lane on successive passes.  So that the case cannot
    pass emptily: on the restatement's own offsets, at least 4 segments whose window lies inside the clip take an offset below the period"""
    from rerender_cases import tie_cases
    cases = [wc.tie_case(sr, ch, P) for sr, ch, P in tie_cases()]
    with make(sound_arena_bytes=32 << 20) as s:
        ids = [upload(s, c["x"], c["rate"]) for c in cases]
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
    for c in cases:
        summary, regs = wr.resolve(c["rate"], c["x"].shape[1], c["anchors"])
        offs = wc.want(c)[2]
        inside = []
        for r, base in zip(regs, np.cumsum([0] + [q["nseg"] for q in regs[:-1]])):
            for k in range(1, r["nseg"]):
                nominal = r["a"] + min(int(np.floor(k * r["step"])), r["room"])
                if nominal + r["W"] + summary["overlap"] <= c["x"].shape[1] and r["W"] > c["period"]:
                    inside.append(int(offs[base + k]))
        assert len(inside) >= 4 and all(v < c["period"] for v in inside), (c["tag"], inside)


def test_the_finite_flag(built):
    """cleared by an inf or a NaN the warp plays; it stays set on a finite clip (two samples near FLT_MAX among them: the fade's weights
    sum to 1), and a clip that lacked it -- an inf in frames the warp skips -- does not gain it"""
    from libzl_amd import _abi
    base = wc.clip(6, 2, 300)
    cases, expect = [], []
    for k in range(5):
        x = base.copy()
        if k == 1:
            x[1, 10] = np.inf
        if k == 2:
            x[0, 290] = np.nan
        if k == 3:
            x[0, 5] = x[1, 200] = 3e38
        cases.append(dict(tag="finite%d" % k, rate=1000.0, x=x, anchors=[(0, 0), (150, 200), (300, 330)]))
        expect.append(k in (0, 3, 4))
    # tau = 4 skips source frames: the inf at frame 60 is read by nothing (L = 24, O = 16, W = 15; the segments start at 0, 96 + off and 192 + off)
    x = wc.clip(8, 2, 240).copy()
    x[0, 60] = np.inf
    cases.append(dict(tag="finite-skipped", rate=1000.0, x=x, anchors=[(0, 0), (240, 60)]))
    y = wr.warp(x, 1000.0, cases[-1]["anchors"])[1]
    assert wr.all_finite(y)
    expect.append(False)
    with make() as s:
        dirty(s, 100000)
        ids = [s.register_clip_pcm(np.ascontiguousarray(c["x"].T), _abi.PCM_F32, 2, c["rate"]) for c in cases]
        assert [s.clip_info(i)["finite"] for i in ids] == [True, False, False, True, True, False]
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
        assert [s.clip_info(i)["finite"] for i in ids] == expect
    for c, ok in zip(cases[:5], expect[:5]):
        assert wr.all_finite(wc.want(c)[1]) == ok


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_loud_neighbour_is_unchanged_and_does_not_leak(built, ch):
    """a quiet clip between two loud ones in a small arena that held noise: the warp of the quiet one reads up to its last frame and
    behind it (zeros by the definition, a neighbour's frames in the arena); the neighbours' extents stay bit for bit"""
    with make(max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(35)
        dirty(s, 200000)
        for n, pairs in ((333, [(133, 150), (200, 180)]), (601, [(601, 700)]), (200, [(100, 100), (100, 130)])):
            loud = [rng.choice(np.array([-7.9, 7.9], f32), (ch, m)) for m in (301, 303)]
            quiet = (rng.uniform(-1.0, 1.0, (ch, n)) * 0.004).astype(f32)
            ids = [upload(s, x, 1000.0) for x in (loud[0], quiet, loud[1])]
            exts = [s.clip_extent(ids[0]), s.clip_extent(ids[2])]
            c = wc.case("quiet-%d-%d" % (n, ch), 1000, ch, pairs, x=quiet)
            bad, outs = check_call(s, [c], [ids[1]])
            assert not bad, bad
            assert np.abs(wc.want(c)[1]).max() < 0.01
            assert wc.same_bits(s.clip_extent(ids[0]), exts[0]) and wc.same_bits(s.clip_extent(ids[2]), exts[1])
            for cid in ids:
                s.unregister_clip(cid)


# ---- playback -------------------------------------------------------------------------------------------------------------------------
PLAY_ANCHORS = [(0, 0), (5000, 5500), (10000, 10000)]


def playback_scene(x, note, nblocks=24):
    """one looping voice over a free-running loop of some 2300 frames from frame 1440 of clip x (planar)"""
    from scenario import Scene, play_cmd
    sc = Scene(num_buses=1, voices_per_bus=2, fs=SR, mode=0, mix_group=0, nframes=256, nblocks=nblocks, bpm=120)
    sc.sounds.append((x[0].copy(), x[1].copy() if x.shape[0] == 2 else None, SR))

    def setup(lib, clip):
        lib.zlo_clip_set_start_position(clip, C.c_float(0.030005))
        lib.zlo_clip_set_length(clip, C.c_float(0.1), 120)           # no whole number of beats: the free-running loop branch
    sc.clip_setup[0] = setup
    sc.events[0] = [("cmd", play_cmd(0, midi_channel=-2, loop=True, note=note, volume=0.8), 0)]
    return sc


def play_warped(x, note, resident=False):
    """(the engine's audio of the scene over clip x warped on the device, the oracle's audio over the restatement's data)"""
    from oracle import zl_oracle as zo
    from scenario import engine_cmd, run_oracle, snapshot_clip
    from libzl_amd.engine import synthetic_clocks
    sc = playback_scene(x, note)
    ref = zo.OracleSynth(1, 1, SR, 0, max_sounds=8)
    assert ref.register_clip(*sc.sounds[0]) == 0
    sc.clip_setup[0](ref.lib, ref.clips[0])
    p = snapshot_clip(ref.clips[0])
    c = dict(tag="play-%d-%d" % (note, resident), rate=SR, x=x, anchors=PLAY_ANCHORS)
    with make(num_buses=1, voices_per_bus=2, max_batch_blocks=sc.nblocks) as s:
        cid = upload(s, x, SR)
        s.set_clip_params(cid, p)
        got = s.clip_warp(cid, PLAY_ANCHORS)
        assert got["applied"] == 1 and got["stretched_regions"] == 2 and mismatch(s, cid, c, got) is None
        s.handle_clip_command(engine_cmd(**sc.events[0][0][1]), 0)
        if resident:
            out = np.zeros((1, 2, sc.nblocks * 256), f32)
            clocks = synthetic_clocks(sc.nblocks, 256, SR)
            for k in range(sc.nblocks):
                L, R = s.process(256, clocks[k])
                out[:, 0, k * 256:(k + 1) * 256] = L
                out[:, 1, k * 256:(k + 1) * 256] = R
            assert s.rt_stats()[1] == sc.nblocks
        else:
            s.render_batch(sc.nblocks, 256, synthetic_clocks(sc.nblocks, 256, SR))
            out = np.array(s.read_bus(), copy=True)
    y = wc.want(c)[1]
    sc.sounds[0] = (y[0].copy(), y[1].copy() if y.shape[0] == 2 else None, SR)
    ref_bus, _, _ = run_oracle(sc)
    return out, ref_bus


@pytest.mark.parametrize("note", [60, 67], ids=["on-grid", "pitched"])
def test_a_voice_across_the_warped_clip_equals_the_oracle_over_the_restatement(built, note):
    x = wc.clip(36 + note, 2, 10000)
    out, ref_bus = play_warped(x, note)
    assert out.shape == ref_bus.shape and len(np.unique(out[0, 0])) > 1000
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_a_voice_through_the_resident_kernel_equals_the_oracle(built, rt_env):
    x = wc.clip(37, 2, 10000)
    out, ref_bus = play_warped(x, 60, resident=True)
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
