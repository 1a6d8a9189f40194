"""K2's on-grid chunks in packed f32 (zl_kernels.hip: zl_mix_acc_ongrid_pk in zl_k2_chunk_ongrid and zl_k2_chunk_ongrid_pair, the report path as
a template parameter, one staged address per voice): parity against the oracle, bit for bit, at the smallest shapes that reach the new code.
Every case is rendered with the pair kernels wherever the shape allows (ZL_K2_PAIR=2) and never (0), in time order (ZL_K2_PHASE_ORDER=0) and in
phase order (2); the four renders are compared with the oracle -- bus as int32, the reports of the call's last block, the integer block peaks and
the RMS extension (check_levels of tests/test_k2_pair.py) -- and with each other.

What the packed sequence can get wrong is the meaning of an operand modifier (which half feeds which lane, which half is negated): any such
mistake moves every frame of every on-grid voice, so one chunk suffices to see it; the shapes below are about where the packed and the scalar
text MEET -- the call's last block (the report path keeps the scalar text), chunks beside chunks of another class adding to the same
accumulator, mono beside stereo -- and about the staged address (start positions inside the source come with every loop restart; a source in a
grown arena segment lies below or above the first segment's base).

A GPU test cannot see which kernel ran: tests/test_k2_launch_cpu.py holds the launch table.  NaN frames compare as in tests/test_k2_ongrid.py."""
import ctypes as C

import numpy as np
import pytest

from scenario import Scene, play_cmd, rand_source
from test_k2_ongrid import ADVERSARIAL
from test_k2_pair import _all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def grid_scene(seed, *, num_buses, voices_per_bus, nblocks, loop_frames=(2600, 4800), stereo=lambda i: True, note=lambda i: 60, sources=None,
               source_frames=(6000, 12000)):
    """sample-space loops at the playback rate (note 60 of a source at the engine's rate: step 1 from integer positions) of loop_frames frames;
    the first three voices of every bus are panned hard left, centre and hard right, the others at random"""
    rng = np.random.default_rng(seed)
    fs = 48000.0
    sc = Scene(num_buses=num_buses, voices_per_bus=voices_per_bus, fs=fs, mode=0, mix_group=0, nframes=256, nblocks=nblocks, bpm=120)
    V = num_buses * voices_per_bus
    for i in range(V):
        L, R = rand_source(rng, int(rng.integers(*source_frames)), stereo=bool(stereo(i)))
        if sources is not None:
            L, R = sources(rng, i, L, R)
        sc.sounds.append((L, R, fs))
        beats = float(rng.integers(*loop_frames)) / 24000.0              # 120 bpm: a beat is 24000 frames
        vol = float(rng.uniform(0.2, 1.0))
        pan = (-1.0, 0.0, 1.0)[i % voices_per_bus] if i % voices_per_bus < 3 else float(rng.uniform(-1, 1))

        def setup(lib, clip, beats=beats, vol=vol, pan=pan):
            lib.zlo_clip_set_length(clip, C.c_float(beats), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // voices_per_bus - 2, loop=True, note=int(note(i)),
                                     volume=float(np.float32(rng.uniform(0.2, 1.0)))), int(rng.integers(0, 50))) for i in range(V)]
    return sc


# one on-grid chunk; the last of the three blocks takes the report path
def test_one_chunk_three_blocks(Engine, monkeypatch):
    sc = grid_scene(0x2801, num_buses=1, voices_per_bus=8, nblocks=3)
    _all(monkeypatch, sc, Engine, 8, batch=1 << 30)


# a partial chunk (9 voices), and a mixed chunk (one pitched voice in the second) beside a packed one
@pytest.mark.parametrize("vpb,pitched", [(9, None), (16, 11)])
def test_partial_and_mixed_chunks(Engine, monkeypatch, vpb, pitched):
    sc = grid_scene(0x2810 + vpb, num_buses=1, voices_per_bus=vpb, nblocks=3, note=lambda i: 67 if i == pitched else 60)
    _all(monkeypatch, sc, Engine, vpb, batch=1 << 30)


# loops of 300 to 700 frames: every voice restarts inside the call, packed and two-tap chunks alternate in one accumulator
def test_short_loops_restart_inside_the_call(Engine, monkeypatch):
    sc = grid_scene(0x2820, num_buses=2, voices_per_bus=128, nblocks=6, loop_frames=(300, 701), source_frames=(1500, 3000))
    _all(monkeypatch, sc, Engine, 256, batch=1 << 30)


# whole chunks of mono voices; and one bus with a mono chunk, a stereo chunk and a chunk of both
def test_mono_and_mono_with_stereo(Engine, monkeypatch):
    sc = grid_scene(0x2830, num_buses=1, voices_per_bus=16, nblocks=3, stereo=lambda i: False)
    _all(monkeypatch, sc, Engine, 16, batch=1 << 30)
    sc = grid_scene(0x2831, num_buses=1, voices_per_bus=24, nblocks=3, stereo=lambda i: i >= 8 and not (i >= 16 and i % 2))
    _all(monkeypatch, sc, Engine, 24, batch=1 << 30)


# sources of the adversarial finite values: +-FLT_MAX, denormals, signed zeros (stereo chunk and mono chunk)
def test_adversarial_finite_sources(Engine, monkeypatch):
    def sources(rng, i, L, R):
        for x in (L, R):
            if x is None:
                continue
            pick = rng.random(x.size) < (0.9 if i % 3 == 0 else 0.3)
            x[pick] = ADVERSARIAL[rng.integers(0, len(ADVERSARIAL) - (2 if i % 2 else 0), int(pick.sum()))]
        if i % 5 == 0 and R is not None:
            L[:] = np.where(rng.random(L.size) < 0.5, np.float32(0.0), np.float32(-0.0)); R[:] = -L
        return L, R
    sc = grid_scene(0x2840, num_buses=1, voices_per_bus=16, nblocks=4, stereo=lambda i: i < 8, sources=sources)
    ref = _all(monkeypatch, sc, Engine, 16, batch=1 << 30, nan_ok=True)
    assert np.isinf(ref).any() or np.isnan(ref).any()                   # FLT_MAX met FLT_MAX


# a call of two blocks: half of the workgroups are on the report path
def test_a_call_of_two_blocks(Engine, monkeypatch):
    sc = grid_scene(0x2850, num_buses=2, voices_per_bus=16, nblocks=2, stereo=lambda i: i % 16 < 8)
    _all(monkeypatch, sc, Engine, 32, batch=1 << 30)


# three calls of two blocks queued on one stream without a synchronise
def test_three_calls_queued_without_a_synchronise(Engine, monkeypatch):
    sc = grid_scene(0x2860, num_buses=2, voices_per_bus=16, nblocks=6, stereo=lambda i: i % 16 < 8)
    _all(monkeypatch, sc, Engine, 32, batch=2, pipelined=True, levels=False)
    _all(monkeypatch, sc, Engine, 32, batch=2)                          # ... and call by call, with the last call's levels


# an arena too small for the second source: every source but the first lands in a segment of its own, somewhere else in the address space
def test_sources_in_grown_arena_segments(Engine, monkeypatch):
    arena = 1 << 20
    grown = []

    def factory(**kw):
        kw["sound_arena_bytes"] = arena
        syn = Engine(**kw)
        close = syn.close

        def closing():
            grown.append(syn.memory_bytes()[1])
            close()
        syn.close = closing
        return syn
    sc = grid_scene(0x2870, num_buses=1, voices_per_bus=16, nblocks=4, stereo=lambda i: i < 8, source_frames=(100000, 110000))
    _all(monkeypatch, sc, factory, 16, batch=1 << 30)
    assert len(grown) == 4 and min(grown) >= 4 * arena
