"""K2's phase order (K1o, zl_order.h): a window's blocks rendered in the loop-phase order of a key voice.  Parity against the oracle, bit for
bit, with the order forced on (ZL_K2_PHASE_ORDER=2) on scenes of short unit-ratio loops -- many passes per window -- for wide buses, narrow
buses with the split tail, fan-out, the offline bounce, calls cut into several windows and the last block's reports; and the same scenes
rendered with the order off and forced on, compared with each other."""
import ctypes as C

import numpy as np
import pytest

from scenario import Scene, compare_runs, play_cmd, rand_source, run_backend, run_oracle


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def loop_scene(seed, *, num_buses, voices_per_bus, nframes=256, nblocks=200, events=False, mode=0):
    """every voice a sample-space loop at the playback rate (unit ratio: the voices the order is built for), loops of 700..5000 frames"""
    rng = np.random.default_rng(seed)
    fs = 48000.0
    sc = Scene(num_buses=num_buses, voices_per_bus=voices_per_bus, fs=fs, mode=mode, mix_group=0, nframes=nframes, nblocks=nblocks, bpm=120)
    V = num_buses * voices_per_bus
    for i in range(V):
        n = int(rng.integers(6000, 12000))
        L, R = rand_source(rng, n, stereo=bool(rng.random() < 0.8))
        sc.sounds.append((L, R, fs))
        beats = float(rng.uniform(0.03, 0.2))                      # fractional beats: a sample-space loop of 0.015..0.1 s
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))

        def setup(lib, clip, beats=beats, vol=vol, pan=pan):
            lib.zlo_clip_set_length(clip, C.c_float(beats), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // voices_per_bus - 2, loop=True, note=60, volume=float(np.float32(rng.uniform(0.2, 1.0)))),
                     int(rng.integers(0, 50))) for i in range(V)]
    if events:
        for k in sorted(set(int(x) for x in rng.integers(1, nblocks, size=3))):
            i = int(rng.integers(0, V))
            sc.events.setdefault(k, []).append(("cmd", dict(clip=i, midiChannel=i // voices_per_bus - 2, midiNote=60, changeVolume=1,
                                                            volume=float(np.float32(rng.uniform(0.1, 1.0)))), 0))
    return sc


def _both(monkeypatch, sc, Engine, V, **kw):
    """oracle parity with the order forced on, then the same run with it off: the two renders agree bit for bit"""
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    out = {}
    for mode in ("2", "0"):
        monkeypatch.setenv("ZL_K2_PHASE_ORDER", mode)
        bus, rep, syn, _ = run_backend(sc, Engine, **kw)
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
        out[mode] = (bus.copy(), getattr(syn, "fan_result", None))
        syn.close()
    assert np.array_equal(out["2"][0].view(np.int32), out["0"][0].view(np.int32))
    if out["2"][1] is not None:
        assert np.array_equal(out["2"][1].view(np.int32), out["0"][1].view(np.int32))
    return ref_bus


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_phase_order_wide_buses(Engine, monkeypatch, mode):
    sc = loop_scene(0x0D01 + mode, num_buses=2, voices_per_bus=80, nblocks=300, mode=mode)
    _both(monkeypatch, sc, Engine, 160, batch=1 << 30)


@pytest.mark.gpu
@pytest.mark.parametrize("buses,tail_min", [(8, None), (12, None), (8, "2048")])
def test_phase_order_narrow_buses_split_tail(Engine, monkeypatch, buses, tail_min):
    """narrow buses: one z-slot holds every bus, and the split tail's slots index the same table; 250 blocks split at the test tier's
    threshold, 2100 blocks at the shipped one (2048) as well"""
    sc = loop_scene(0x0D10 + buses, num_buses=buses, voices_per_bus=8, nblocks=2100 if tail_min else 250)
    _both(monkeypatch, sc, Engine, buses * 8, batch=1 << 30)


@pytest.mark.gpu
def test_phase_order_fanout(Engine, monkeypatch):
    from libzl_amd import PassthroughParams
    from test_rt_fanout import _oracle_fanout
    sc = loop_scene(0x0D20, num_buses=4, voices_per_bus=16, nblocks=180)
    fan = [PassthroughParams(0.8, 1.0, -1.25, -0.3 + 0.1 * b, 0) for b in range(4)]
    ref_bus = _both(monkeypatch, sc, Engine, 64, batch=1 << 30, fanout=fan)
    monkeypatch.setenv("ZL_K2_PHASE_ORDER", "2")
    bus, rep, syn, _ = run_backend(sc, Engine, batch=1 << 30, fanout=fan)
    assert np.array_equal(syn.fan_result.view(np.int32), _oracle_fanout(ref_bus, fan).view(np.int32))
    syn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
@pytest.mark.parametrize("direct", ["2", "0"])
def test_phase_order_bounce(Engine, monkeypatch, fmt, direct):
    monkeypatch.setenv("ZL_BOUNCE_DIRECT", direct)
    sc = loop_scene(0x0D30, num_buses=3, voices_per_bus=8, nblocks=160, events=True)
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    outs = []
    for mode in ("2", "0"):
        monkeypatch.setenv("ZL_K2_PHASE_ORDER", mode)
        bus, rep, syn, _ = run_backend(sc, Engine, bounce=(fmt, 70))
        if fmt == "f32":
            compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, 24)
        outs.append(np.array(bus, copy=True))
        syn.close()
    assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("window", [40, 97])
def test_phase_order_several_windows_and_events(Engine, monkeypatch, window):
    """plan windows of 40 / 97 blocks (the record sets alternate; each window has its own table) and events that cut the calls"""
    sc = loop_scene(0x0D40 + window, num_buses=4, voices_per_bus=16, nblocks=400, events=True)
    _both(monkeypatch, sc, Engine, 64, batch=1 << 30, plan_window_blocks=window)


@pytest.mark.gpu
def test_phase_order_auto_headline_shape(Engine, monkeypatch):
    """auto mode (the default) on the shape it is built for: unit-ratio loops, 256-frame blocks, one bus of 128 voices, a window of many passes"""
    sc = loop_scene(0x0D50, num_buses=1, voices_per_bus=128, nblocks=500)
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    monkeypatch.setenv("ZL_K2_PHASE_ORDER", "1")
    bus, rep, syn, _ = run_backend(sc, Engine, batch=1 << 30)
    compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, 128)
    syn.close()
