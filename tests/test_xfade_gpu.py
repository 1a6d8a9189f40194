"""Loop crossfade, GPU tier: the kernels of libzl_amd/csrc/zl_xfade.hip against the numpy / Python-integer restatement
(tests/xfade_ref.py).  Every extent is read back whole (zlhip_debug_sound_extent) from a small arena that held noise and compared ==
with the restatement, which takes rho from the device's three integers (themselves == the restatement's) through the library's
zlhip_xfade_design; then the limits, the correlation's edges, the finite flag, a loud neighbour, and a looping voice rendered across
two laps of the crossfaded clip against the oracle's run over the restatement's data.  tests/test_xfade_edges_gpu.py holds the
engine's behaviour around the call."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_ref as lr
import xfade_cases as xc
import xfade_ref as xr
from xfade_cases import SR, check_call, dirty, mismatch, upload

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
def test_the_grid_in_one_call(built):
    """tests/xfade_cases.py::grid (tests/test_xfade_cpu.py asserts what it covers): every case in ONE call, requests with nothing to fade
    first, last and twice in a row; then every clip's info and that the clips with nothing to fade are untouched"""
    cases = xc.grid()
    with make(max_sounds=512, sound_arena_bytes=32 << 20) as s:
        dirty(s, 3 << 20)
        ids = [upload(s, c["x"]) for c in cases]
        before = {i: s.clip_extent(cid) for i, (cid, c) in enumerate(zip(ids, cases)) if c["start_frame"] == 0}
        bad, outs = check_call(s, cases, ids)
        assert not bad, (len(bad), bad[:3])
        assert [i for i, o in enumerate(outs) if not o["applied"]] == sorted(before) and len(before) == 4
        for i, ext in before.items():
            assert np.array_equal(s.clip_extent(ids[i]).view(u32), ext.view(u32))
        for cid, c in zip(ids, cases):
            assert s.clip_info(cid) == {"length": c["x"].shape[1], "channels": c["x"].shape[0], "sample_rate": SR, "finite": True, "rendered": False}
        # the extents' tails are the kernel's zeros, not the arena's noise
        for cid, c in zip(ids[1:40], cases[1:40]):
            ext = s.clip_extent(cid)
            assert ext.size > c["x"].size and not ext[c["x"].size:].any()


def test_the_single_call_and_a_second_fade_of_the_same_clip(built):
    with make() as s:
        dirty(s, 100000)
        rng = np.random.default_rng(31)
        c = dict(x=xc.clip(rng, 2, 5000), start_frame=1000, stop_frame=4000, fade_frames=0, curve=xr.AUTO)
        cid = upload(s, c["x"])
        got = s.clip_loop_crossfade(cid, 1000, 4000)
        assert got["applied"] == 1 and got["fade_frames"] == 960 and mismatch(s, cid, c, got) is None
        # again, on the crossfaded data, another loop and a fixed curve
        L, R = s.read_clip(cid)
        c2 = dict(x=np.stack([L, R]), start_frame=700, stop_frame=2001, fade_frames=333, curve=xr.EQUAL_POWER)
        got = s.clip_loop_crossfade(cid, 700, 2001, 333, xr.EQUAL_POWER)
        assert got["rho"] == 0.0 and got["curve"] == xr.EQUAL_POWER and mismatch(s, cid, c2, got) is None


# ---- the limits -----------------------------------------------------------------------------------------------------------------------
def test_the_longest_fade_with_the_largest_sums(built):
    """X = 65536 on a mono clip of 200000 frames at +-10: every q is +-32767, saa = sbb = 65536 * 32767^2, 64 chunks of the measuring
    workgroup"""
    rng = np.random.default_rng(32)
    x = rng.choice(np.array([-10.0, 10.0], f32), (1, 200000))
    c = dict(x=x, start_frame=70000, stop_frame=199999, fade_frames=65536, curve=xr.AUTO)
    with make(sound_arena_bytes=4 << 20) as s:
        dirty(s, 500000)
        cid = upload(s, x)
        got = s.clip_loop_crossfade(cid, 70000, 199999, 65536)
        assert got["saa"] == got["sbb"] == 65536 * 32767 ** 2 and abs(got["sab"]) < got["saa"]
        assert mismatch(s, cid, c, got) is None
        from libzl_amd import ZlHipError
        with pytest.raises(ZlHipError, match=r"\(-1\)"):
            s.clip_loop_crossfade(cid, 70000, 199999, 65537)


# ---- the correlation's edges ----------------------------------------------------------------------------------------------------------
def test_silence_identical_and_antiphase_regions(built):
    rng = np.random.default_rng(33)
    n, s0, e0, X = 3000, 700, 2500, 300
    base = xc.clip(rng, 2, n)
    silent = base.copy(); silent[:, e0 - X:e0] = 0.0                 # Saa = 0
    same = base.copy(); same[:, e0 - X:e0] = same[:, s0 - X:s0]
    anti = base.copy(); anti[:, e0 - X:e0] = -anti[:, s0 - X:s0]
    cases = [dict(x=x, start_frame=s0, stop_frame=e0, fade_frames=X, curve=xr.AUTO) for x in (silent, same, anti, np.zeros((1, n), f32))]
    with make() as s:
        dirty(s, 100000)
        ids = [upload(s, c["x"]) for c in cases]
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
        assert outs[0]["saa"] == 0 and outs[0]["sbb"] > 0 and outs[0]["correlation"] == 0.0 and outs[0]["rho"] == 0.0
        assert outs[1]["sab"] == outs[1]["saa"] == outs[1]["sbb"] > 0 and outs[1]["correlation"] == 1.0 and outs[1]["rho"] == 1.0
        assert outs[2]["sab"] == -outs[2]["saa"] == -outs[2]["sbb"] and outs[2]["correlation"] == -1.0 and outs[2]["rho"] == 0.0     # clamped
        assert (outs[3]["sab"], outs[3]["saa"], outs[3]["sbb"], outs[3]["rho"]) == (0, 0, 0, 0.0) and outs[3]["applied"] == 1


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def test_the_finite_flag(built):
    """cleared by an inf in A, a NaN in B, two 3e38 samples that overflow at mid-fade under the equal-power curve; it stays set on a
    finite clip (the same two samples under the linear curve among them), and a clip that lacked it does not gain it"""
    from libzl_amd import _abi
    rng = np.random.default_rng(34)
    base = rng.uniform(-1.0, 1.0, (2, 400)).astype(f32)
    cases, expect = [], []
    for k in range(6):
        x = base.copy()
        if k == 1:
            x[1, 290] = np.inf
        if k == 2:
            x[0, 90] = np.nan
        if k in (3, 4):
            x[0, 275] = x[0, 75] = 3e38
        if k == 5:
            x[1, 20] = np.inf                                      # outside both regions: the original lacks the flag
        cases.append(dict(x=x, start_frame=100, stop_frame=300, fade_frames=50, curve=xr.LINEAR if k == 4 else xr.EQUAL_POWER))
        expect.append(k in (0, 4))
    with make() as s:
        dirty(s, 100000)
        ids = [s.register_clip_pcm(np.ascontiguousarray(c["x"].T), _abi.PCM_F32, 2, SR) for c in cases]
        assert [s.clip_info(i)["finite"] for i in ids] == [True, False, False, True, True, False]
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
        assert [s.clip_info(i)["finite"] for i in ids] == expect
        for c, ok in zip(cases[:5], expect[:5]):
            _, y = xr.crossfade(c["x"], SR, 100, 300, 50, c["curve"])
            assert xr.all_finite(y, 100, 300, 50) == ok


# ---- a neighbour does not leak --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a clip at 0.004 between two at +-7.9 in a small arena that held noise; B begins at the quiet clip's frame 0 and A ends at its last
    frame, whose 16-byte group lies partly behind the data: a neighbour's frame in a head or tail group would change the integers (a
    loud frame is 2000 times a quiet one) or the extent"""
    with make(max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(35)
        dirty(s, 200000)
        for n, X in ((3333, 257), (6001, 960), (131, 65)):
            loud = [np.repeat(rng.choice(np.array([-7.9, 7.9], f32), (1, m)), ch, axis=0) for m in (3001, 3003)]      # (both channels alike: |m| = ch * 32358)
            quiet = (rng.uniform(-1.0, 1.0, (ch, n)) * 0.004).astype(f32)
            xs = (loud[0], quiet, loud[1])
            ids = [upload(s, x) for x in xs]
            cases = [dict(x=x, start_frame=X, stop_frame=x.shape[1], fade_frames=X, curve=xr.AUTO) for x in (quiet, loud[0], loud[1])]
            bad, outs = check_call(s, cases, [ids[1], ids[0], ids[2]])
            assert not bad, bad
            assert 0 < outs[0]["saa"] < X * (17 * ch) ** 2 and outs[1]["saa"] == X * (ch * 32358) ** 2
            for cid in ids:
                s.unregister_clip(cid)


# ---- playback -------------------------------------------------------------------------------------------------------------------------
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


def play_crossfaded(x, note, resident=False):
    """(the engine's audio of the scene over clip x crossfaded on the device, the oracle's audio over the restatement's data, the result)"""
    from oracle import zl_oracle as zo
    from scenario import engine_cmd, run_oracle, snapshot_clip
    from libzl_amd.engine import synthetic_clocks
    sc = playback_scene(x, note)
    ref = zo.OracleSynth(1, 1, SR, 0, max_sounds=8)
    assert ref.register_clip(*sc.sounds[0]) == 0
    sc.clip_setup[0](ref.lib, ref.clips[0])
    p = snapshot_clip(ref.clips[0])
    s0, e0 = lr.frame_of(p.start_position_seconds, SR), lr.stop_of(p.start_position_seconds, p.length_seconds, SR)
    assert s0 == 1440 and 2000 <= e0 - s0 <= 2500                  # the frames the voice derives from the clip's seconds
    with make(num_buses=1, voices_per_bus=2, max_batch_blocks=sc.nblocks) as s:
        cid = upload(s, x)
        s.set_clip_params(cid, p)
        got = s.clip_loop_crossfade(cid, s0, e0)
        c = dict(x=x, start_frame=s0, stop_frame=e0, fade_frames=0, curve=xr.AUTO)
        assert got["fade_frames"] == 960 and mismatch(s, cid, c, got) is None
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
    _, y = xr.crossfade(x, SR, s0, e0, 0, xr.AUTO, ints=(got["sab"], got["saa"], got["sbb"]))
    sc.sounds[0] = (y[0].copy(), y[1].copy() if y.shape[0] == 2 else None, SR)
    ref_bus, _, _ = run_oracle(sc)
    return out, ref_bus, got


@pytest.mark.parametrize("note", [60, 67], ids=["on-grid", "pitched"])
def test_a_looping_voice_over_two_laps_equals_the_oracle_over_the_restatement(built, note):
    x = xr.tone(218.4, 2, 6000, decay=3000.0) + xr.noise(36, 2, 6000, 0.01)
    out, ref_bus, _ = play_crossfaded(x.astype(f32), note)
    assert out.shape == ref_bus.shape and len(np.unique(out[0, 0])) > 1000       # it moves through the loop; 6144 frames: more than two laps
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


def test_a_looping_voice_through_the_resident_kernel_equals_the_oracle(built, rt_env):
    x = (xr.tone(133.7, 2, 6000, decay=3000.0) + xr.noise(37, 2, 6000, 0.01)).astype(f32)
    out, ref_bus, _ = play_crossfaded(x, 60, resident=True)
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
