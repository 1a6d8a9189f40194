"""Engine group (zlhip_group_*, SamplerSynthGroup) on the GPU, bit-exact: the bus-aligned partition against the oracle and one engine
with the whole config, the span partition (the spanning-bus sum zl_k_group_reduce_scan) against the oracle with mix_group = VPB / n and
one engine with voices_per_task = VPB / n, the routing of a spanning bus that overflows, consecutive calls queued without a
synchronisation, a group of one, and two devices when there are two."""

import numpy as np
import pytest

from group_cases import assert_same_bus, assert_same_levels, assert_same_reports, check_against, group
from libzl_amd import MODE_FAITHFUL, MODE_FIX_DELAY, MODE_HERMITE, SamplerSynth, SamplerSynthGroup
from scenario import Scene, compare_runs, engine_cmd, play_cmd, rand_source, random_scene, run_backend, run_oracle, snapshot_clip

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
@pytest.mark.parametrize("seed", [3, 11])
def test_bus_aligned_equals_one_engine_and_oracle(devices, seed):
    """the reference shape (12 buses x 8 voices), commands by midi channel and clip edits between blocks; the hold bus lives on a
    member other than the first"""
    sc = random_scene(seed, num_buses=12, voices_per_bus=8)
    hold = 7 if len(devices) == 2 else 5                           # (bus 7 of 2 members, bus 5 of 3: member 1)
    check_against(sc, group(devices, "bus"), hold=hold)
    syn = SamplerSynthGroup(devices, 12, 8, partition="bus")
    lay = syn.layout()
    assert [m["partition"] for m in lay] == ["bus"] * len(devices)
    assert lay[1]["first_bus"] <= hold < lay[1]["first_bus"] + lay[1]["num_buses"]
    syn.close()


@pytest.mark.parametrize("mode", [MODE_FAITHFUL, MODE_FIX_DELAY, MODE_HERMITE])
@pytest.mark.parametrize("n", [2, 4])
def test_span_commands_by_midi_channel(n, mode):
    """VPB = 8 spanning n members: the routing of commands by midi channel on the device path"""
    for seed in (5, 17):
        sc = random_scene(seed, num_buses=3, voices_per_bus=8, mode=mode, mix_group=8 // n)
        check_against(sc, group([0] * n, "span"))


def wide_scene(mode, n, nblocks=6, nframes=256):
    """8 buses x 128 voices, every slot started with start_voice (a clip each of 24 sources, looping, pitched by the note)"""
    rng = np.random.default_rng(1234 + mode)
    sc = Scene(num_buses=8, voices_per_bus=128, fs=48000.0, mode=mode, mix_group=128 // n, nframes=nframes, nblocks=nblocks)
    for i in range(24):
        L, R = rand_source(rng, 3000 + 211 * i, stereo=(i % 5 != 4))
        sc.sounds.append((L, R, 44100.0 if i % 3 == 0 else 48000.0))
    ev = []
    for b in range(8):
        for s in range(128):
            if (b * 128 + s) % 7 == 3:
                continue                                           # a few idle slots
            ev.append(("start", b, s, play_cmd((b * 128 + s) % 24, midi_channel=b - 2, loop=(s % 9 != 0), note=55 + (s % 11),
                                                volume=0.05 + 0.001 * s), 0))
    sc.events[0] = ev
    sc.events[3] = [("stopv", 2, 5, True), ("stopv", 6, 127, False)]
    return sc


@pytest.mark.parametrize("mode", [MODE_FAITHFUL, MODE_FIX_DELAY, MODE_HERMITE])
@pytest.mark.parametrize("n", [2, 4])
def test_span_wide_buses(n, mode):
    check_against(wide_scene(mode, n), group([0] * n, "span"))


def test_span_routing_overflow():
    """ten starts on one bus of 8 voices over 4 members (two voices each): every slot of the bus is taken in global slot order --
    member 0's slice first -- and the two starts beyond are dropped, as one engine drops them"""
    rng = np.random.default_rng(99)
    sc = Scene(num_buses=2, voices_per_bus=8, fs=48000.0, mix_group=2, nframes=128, nblocks=6)
    for i in range(10):
        L, R = rand_source(rng, 2500 + 50 * i)
        sc.sounds.append((L, R, 48000.0))
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=-2, note=50 + i, volume=0.3), 0) for i in range(10)]
    sc.events[2] = [("cmd", play_cmd(1, midi_channel=-1, note=60), 0), ("cmd", dict(clip=3, midiChannel=-2, midiNote=53, stopPlayback=1,
                                                                                   startPlayback=1, looping=1, volume=0.7), 0)]
    ref, orep, osyn = run_oracle(sc)
    grp, repg, syn, _ = run_backend(sc, group([0] * 4, "span"))
    compare_runs(ref, orep, osyn, grp, repg, 16)
    for v in range(8):                                             # slot v of bus 0 plays the v-th start, as in the oracle
        assert osyn.voices[v].isPlaying and repg[v].clip == osyn.voices[v].sound == v
    syn.close()
    # the taken / voices of one engine
    syn = SamplerSynthGroup([0] * 4, 2, 8, partition="span", max_sounds=16, sound_arena_bytes=1 << 22)
    one = SamplerSynth(2, 8, max_sounds=16, sound_arena_bytes=1 << 22)
    for s in (syn, one):
        for (L, R, sr) in sc.sounds:
            s.register_clip(L, R, sr)
    cmds = [engine_cmd(**play_cmd(i, midi_channel=-2, note=50 + i)) for i in range(10)]
    tg, vg = syn.handle_clip_commands(cmds, 0, want_voices=True)
    t1, v1 = one.handle_clip_commands(cmds, 0, want_voices=True)
    assert (tg, vg) == (t1, v1) == ([1] * 8 + [0, 0], list(range(8)) + [-1, -1])
    assert all(syn.voice_is_playing(0, s) for s in range(8)) and not syn.voice_is_playing(1, 0)
    syn.close()
    one.close()


def test_span_calls_queue_without_synchronising():
    """three span calls into three caller buffers on the root's device, queued back to back: the third call's render may not start
    before every member's share of the second call's sum has read the partial buses (ordering step 3)"""
    import torch
    rng = np.random.default_rng(5)
    K, N, calls = 48, 256, 3
    sc = Scene(num_buses=4, voices_per_bus=32, fs=48000.0, mix_group=16, nframes=N, nblocks=K * calls)
    for i in range(12):
        L, R = rand_source(rng, 4000 + 333 * i)
        sc.sounds.append((L, R, 44100.0 if i % 2 else 48000.0))
    sc.events[0] = [("start", b, s, play_cmd((b * 32 + s) % 12, midi_channel=b - 2, note=52 + (s % 13), volume=0.1), 0)
                    for b in range(4) for s in range(32) if (b + s) % 5]
    ref, _, _ = run_oracle(sc, batch=K)
    syn = SamplerSynthGroup([0, 0], 4, 32, partition="span", max_batch_blocks=K, max_frames=N, max_sounds=16, sound_arena_bytes=1 << 22)
    from scenario import zo
    oref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=16)
    for i, (L, R, sr) in enumerate(sc.sounds):
        oref.register_clip(L, R, sr)
        assert syn.register_clip(L, R, sr) == i
        syn.set_clip_params(i, snapshot_clip(oref.clips[i]))
    for ev in sc.events[0]:
        syn.start_voice(ev[1], ev[2], engine_cmd(**ev[3]), ev[4])
    outs = [torch.full((4, 2, K * N), 3.0, device="cuda:0", dtype=torch.float32) for _ in range(calls)]
    for c in range(calls):
        syn.render_batch(K, N, sc.make_clocks(c * K, K), bus_out_dev=outs[c].data_ptr())
    syn.synchronize()
    torch.cuda.synchronize()
    for c in range(calls):
        assert_same_bus(ref[:, :, c * K * N:(c + 1) * K * N], outs[c].cpu().numpy(), f"call {c}")
    syn.close()


@pytest.mark.parametrize("partition", ["span", "bus"])
def test_group_of_one_is_one_engine(partition):
    sc = random_scene(8, num_buses=3, voices_per_bus=8)
    check_against(sc, group([0], partition))


def test_two_devices_equal_one_device():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    sc = random_scene(21, num_buses=12, voices_per_bus=8)
    a, ra, sa, _ = run_backend(sc, group([0, 0], "bus"))
    b, rb, sb, _ = run_backend(sc, group([0, 1], "bus"))
    assert_same_bus(a, b, "bus-aligned [0, 1] vs [0, 0]")
    assert_same_reports(ra, rb, 96, "bus-aligned [0, 1] vs [0, 0]")
    sc = random_scene(22, num_buses=3, voices_per_bus=8, mix_group=4)
    a, ra, sa, _ = run_backend(sc, group([0, 0], "span"))
    b, rb, sb, _ = run_backend(sc, group([0, 1], "span"))
    assert_same_bus(a, b, "span [0, 1] vs [0, 0]")
    assert_same_reports(ra, rb, 24, "span [0, 1] vs [0, 0]")
    assert_same_levels(sa.levels_tick(), sb.levels_tick(), 3, "span [0, 1] vs [0, 0]")
