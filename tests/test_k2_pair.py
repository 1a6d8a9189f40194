"""K2 with two frames per lane (zl_k2_pair_render / zl_k2_pair_phase_render, zl_pair.h): lane j of a 128-lane workgroup renders frames 2 j and
2 j + 1 of a 256-frame block, and an on-grid voice gives it both frames in one 16-byte load.  Parity against the oracle, bit for bit, with the
kernels taken wherever the launch shape allows (ZL_K2_PAIR=2) and never (0), in time order (ZL_K2_PHASE_ORDER=0) and in phase order (2); the
four renders are also compared with each other.  Checked against the oracle: the bus as int32, the reports of the call's last block, the integer
block peaks of every block of the last call and the RMS extension of several of its blocks per bus and channel (the fused level scan, whose
defined order the pair form keeps with a tree of its own, zl_wave_levels4_pair).

A GPU test cannot see which kernel ran; the CPU tier's table can (tests/test_k2_launch_cpu.py: the launch description zl_launch_render launches
from).  With the switch at 2 every batch launch of mode 0, 256 frames, wide buses and no mix groups takes the pair kernels
(tests/test_k2_pair_cpu.py holds the gate's truth table), and the scenes are built so that every chunk class passes through them --
on-grid interior blocks, the blocks at loop restarts, pitched voices, mono sources, envelopes, voices that start and stop.

NaN frames are compared as in tests/test_k2_ongrid.py: "NaN in the same frames"."""
import ctypes as C

import numpy as np
import pytest

from level_checks import INT_MAX, check_levels, peak_int      # (tests/test_k2_pair_*.py take check_levels from here)
from scenario import Scene, compare_runs, play_cmd, rand_source, run_backend, run_oracle, stop_cmd
from test_k2_ongrid import ADVERSARIAL, loop_scene, same_bits_nan_aware

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def _all(monkeypatch, sc, factory, V, *, orders=("0", "2"), nan_ok=False, levels=True, **kw):
    """oracle parity with the pair kernels on (2) and off (0), in time order and in phase order; all renders agree bit for bit"""
    ref_bus, ref_rep, ref_syn = run_oracle(sc, threads=8 if V >= 512 else 1)
    outs = []
    for order in orders:
        monkeypatch.setenv("ZL_K2_PHASE_ORDER", order)
        for pair in ("2", "0"):
            monkeypatch.setenv("ZL_K2_PAIR", pair)
            bus, rep, syn, _ = run_backend(sc, factory, **kw)
            try:
                if nan_ok:
                    assert same_bits_nan_aware(ref_bus, bus), (order, pair)
                    compare_runs(np.nan_to_num(ref_bus, nan=0.0), ref_rep, ref_syn, np.nan_to_num(bus, nan=0.0), rep, V, exact=False, tol=0.0)
                else:
                    compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
                if levels:
                    check_levels(syn, ref_bus, sc.nframes)
                fan = getattr(syn, "fan_result", None)
                outs.append((bus.copy(), None if fan is None else fan.copy()))
            finally:
                syn.close()
    for o, f in outs[1:]:
        assert np.array_equal(outs[0][0].view(np.int32), o.view(np.int32))
        if f is not None:
            assert np.array_equal(outs[0][1].view(np.int32), f.view(np.int32))
    return ref_bus


# (a) the headline shape and a small one: stereo loops at ratio 1
@pytest.mark.parametrize("buses,vpb,nblocks", [(8, 128, 60), (3, 16, 120)])
def test_ratio_one_stereo_loops(Engine, monkeypatch, buses, vpb, nblocks):
    sc = loop_scene(0x1F01 + buses, num_buses=buses, voices_per_bus=vpb, nblocks=nblocks)
    _all(monkeypatch, sc, Engine, buses * vpb, batch=1 << 30)


# (b) whole chunks of mono voices (the 8-byte pair load, any 4-byte alignment), and mono mixed with stereo (mixed chunks: the general path)
def test_mono_chunks_and_mono_with_stereo(Engine, monkeypatch):
    sc = loop_scene(0x1F10, num_buses=2, voices_per_bus=16, nblocks=90, stereo_p=0.0)
    _all(monkeypatch, sc, Engine, 32, batch=1 << 30)
    sc = loop_scene(0x1F11, num_buses=2, voices_per_bus=32, nblocks=90, stereo_p=0.5)
    _all(monkeypatch, sc, Engine, 64, batch=1 << 30)


# (c) pitched voices among root-note ones: the two-tap classes, once per frame of the lane
def test_pitched_voices_among_root_note_ones(Engine, monkeypatch):
    sc = loop_scene(0x1F20, num_buses=4, voices_per_bus=32, nblocks=90, stereo_p=0.7, notes=(60, 60, 60, 48, 67, 72))
    _all(monkeypatch, sc, Engine, 128, batch=1 << 30)


# (d) sources made of the adversarial finite values (signed zeros, denormals, +-FLT_MAX) ...
def test_adversarial_finite_sources(Engine, monkeypatch):
    def sources(rng, i, L, R):
        for x in (L, R):
            pick = rng.random(x.size) < (0.9 if i % 3 == 0 else 0.3)
            x[pick] = ADVERSARIAL[rng.integers(0, len(ADVERSARIAL) - (2 if i % 2 else 0), int(pick.sum()))]
        if i % 5 == 0:
            L[:] = np.where(rng.random(L.size) < 0.5, np.float32(0.0), np.float32(-0.0)); R[:] = -L
        return L, R
    sc = loop_scene(0x1F30, num_buses=3, voices_per_bus=16, nblocks=80, sources=sources)
    _all(monkeypatch, sc, Engine, 48, batch=1 << 30, nan_ok=True)


# ... and a source with NaN and infinities among clean ones: its chunk is not on-grid, the NaN frames are the oracle's
def test_a_non_finite_source(Engine, monkeypatch):
    def sources(rng, i, L, R):
        if i % 8 == 3:
            at = rng.integers(0, 3000, 40)
            L[at[:10]] = np.nan; R[at[10:20]] = np.inf; L[at[20:30]] = -np.inf; R[at[30:]] = np.nan
            L[:600:7] = np.inf
        return L, R
    sc = loop_scene(0x1F40, num_buses=2, voices_per_bus=16, nblocks=80, sources=sources)
    ref_bus = _all(monkeypatch, sc, Engine, 32, batch=1 << 30, nan_ok=True)
    assert np.isnan(ref_bus).any() and not np.isnan(ref_bus).all(axis=2).any()


# (e) start positions that are an integer number of samples, odd ones among them (a mono pair load that is only 4-byte aligned)
def test_integer_start_positions(Engine, monkeypatch):
    sc = loop_scene(0x1F50, num_buses=2, voices_per_bus=24, nblocks=90, start=True, stereo_p=0.6)
    _all(monkeypatch, sc, Engine, 48, batch=1 << 30)


def envelope_scene(seed, *, num_buses=2, voices_per_bus=16, nblocks=96):
    """loops and one-shots at ratio 1 with attack / decay / release envelopes; voices started and stopped at blocks inside the scene (the
    release tails, the per-frame-control chunks and the chunks with idle voices all run inside the pair kernels)"""
    rng = np.random.default_rng(seed)
    fs = 48000.0
    sc = Scene(num_buses=num_buses, voices_per_bus=voices_per_bus, fs=fs, nframes=256, nblocks=nblocks, bpm=120)
    V = num_buses * voices_per_bus
    loops = []
    for i in range(V):
        loop = bool(i % 3)
        loops.append(loop)
        n = int(rng.integers(6000, 12000)) if loop else int(rng.integers(3000, 20000))
        L, R = rand_source(rng, n, stereo=bool(rng.random() < 0.8))
        sc.sounds.append((L, R, fs))
        beats = float(rng.uniform(0.03, 0.2))
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))
        adsr = [(0.0, 0.1, 1.0, 0.0), (0.004, 0.003, 0.7, 0.02), (0.0, 0.002, 0.5, 0.05)][i % 3]

        def setup(lib, clip, loop=loop, beats=beats, vol=vol, pan=pan, adsr=adsr):
            if loop:
                lib.zlo_clip_set_length(clip, C.c_float(beats), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
            clip.adsr.p.attack, clip.adsr.p.decay, clip.adsr.p.sustain, clip.adsr.p.release = adsr
        sc.clip_setup[i] = setup

    def play(i):
        return ("cmd", play_cmd(i, midi_channel=i // voices_per_bus - 2, loop=loops[i], note=60, volume=float(np.float32(rng.uniform(0.2, 1.0)))),
                int(rng.integers(0, 50)))
    late = set(int(x) for x in rng.choice(V, V // 4, replace=False))
    sc.events[0] = [play(i) for i in range(V) if i not in late]
    for i in sorted(late):                                           # started inside the scene
        sc.events.setdefault(int(rng.integers(5, nblocks // 2)), []).append(play(i))
    for i in rng.choice(V, V // 3, replace=False):                   # stopped inside it: release tails
        sc.events.setdefault(int(rng.integers(nblocks // 2, nblocks - 8)), []).append(
            ("cmd", stop_cmd(int(i), midi_channel=int(i) // voices_per_bus - 2, note=60), 0))
    return sc


# (f) one-shots with release tails, voices started and stopped between the calls of a scene
def test_one_shots_release_tails_starts_and_stops(Engine, monkeypatch):
    sc = envelope_scene(0x1F60)
    _all(monkeypatch, sc, Engine, 32, batch=1 << 30)


# (g) a call cut into several plan windows (the record sets alternate), and three calls queued without a synchronise
@pytest.mark.parametrize("window", [40, 97])
def test_several_plan_windows(Engine, monkeypatch, window):
    sc = loop_scene(0x1F70 + window, num_buses=4, voices_per_bus=16, nblocks=400, stereo_p=0.8)
    _all(monkeypatch, sc, Engine, 64, batch=1 << 30, plan_window_blocks=window)


def test_three_calls_queued_without_a_synchronise(Engine, monkeypatch):
    sc = loop_scene(0x1F80, num_buses=4, voices_per_bus=32, nblocks=180, stereo_p=0.8)
    _all(monkeypatch, sc, Engine, 128, batch=60, pipelined=True, levels=False)


# (h) the scene's last block ends exactly at a loop restart: loops of 750, 1500 and 3000 frames (lengths that are exact in float seconds)
#     started at frame 0; 375 blocks of 256 frames are 64 passes of 1500
def test_last_block_ends_at_a_loop_restart(Engine, monkeypatch):
    fs = 48000.0
    rng = np.random.default_rng(0x1F90)
    sc = Scene(num_buses=2, voices_per_bus=16, fs=fs, nframes=256, nblocks=375, bpm=120)
    for i in range(32):
        L, R = rand_source(rng, 6000, stereo=bool(i % 4))
        sc.sounds.append((L, R, fs))
        length = (750.0, 1500.0, 3000.0)[i % 3] / fs
        pan = float(rng.uniform(-1, 1))

        def setup(lib, clip, length=length, pan=pan):
            clip.lengthInBeats = 0.3                                 # fractional: a sample-space loop
            clip.lengthInSeconds = length
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // 16 - 2, loop=True, note=60, volume=0.7), 0) for i in range(32)]
    _all(monkeypatch, sc, Engine, 32, batch=1 << 30)


# shapes the gate must refuse with the switch at 2: they keep the kernels they have and are still the oracle's bits
REFUSED = {
    "n64": dict(nframes=64), "n100": dict(nframes=100), "n128": dict(nframes=128), "n512": dict(nframes=512),
    "narrow": dict(num_buses=12, voices_per_bus=8), "mixgroup": dict(num_buses=2, voices_per_bus=64, mix_group=16),
    "mode1": dict(mode=1), "mode2": dict(mode=2), "mode4": dict(mode=4), "fanout": dict(fanout=True), "bounce": dict(bounce=True),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_shapes_the_gate_refuses(Engine, monkeypatch, what):
    cfg = dict(num_buses=2, voices_per_bus=16, nframes=256, mode=0, mix_group=0, fanout=False, bounce=False)
    cfg.update(REFUSED[what])
    V = cfg["num_buses"] * cfg["voices_per_bus"]
    sc = loop_scene(0x1FA0 + sorted(REFUSED).index(what), num_buses=cfg["num_buses"], voices_per_bus=cfg["voices_per_bus"], nframes=cfg["nframes"],
                    nblocks=max(40, 80 * 256 // cfg["nframes"]), mode=cfg["mode"], stereo_p=0.8)
    sc.mix_group = cfg["mix_group"]
    kw = dict(batch=1 << 30)
    fan = None
    if cfg["fanout"]:
        from libzl_amd import PassthroughParams
        fan = [PassthroughParams(0.8, 1.0, -1.25, -0.3 + 0.1 * b, 0) for b in range(cfg["num_buses"])]
        kw["fanout"] = fan
    if cfg["bounce"]:
        kw = dict(bounce=("f32", 30))
    ref_bus = _all(monkeypatch, sc, Engine, V, levels=False, **kw)
    if fan is not None:
        from test_rt_fanout import _oracle_fanout
        monkeypatch.setenv("ZL_K2_PAIR", "2")
        bus, rep, syn, _ = run_backend(sc, Engine, **kw)
        assert np.array_equal(syn.fan_result.view(np.int32), _oracle_fanout(ref_bus, fan).view(np.int32))
        syn.close()
