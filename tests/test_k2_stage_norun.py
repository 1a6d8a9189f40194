"""The pair kernels' staging without the run lists (zl_k2_stage_load<false>, zl_kernels.hip): in phase order K1o leaves, behind the order
table, the first block no inline run of a bus's voices reaches (run_end) and a dense copy of every voice's dead_from; a workgroup of
zl_k2_pair_phase_render whose block lies at or behind run_end stages its voices without touching their run lists.  Nothing the kernel
computes from changes, so the bits must not: every scene is rendered with ZL_K2_STAGE_NORUN at 1 and at 0 (K1o then writes
run_end = INT_MAX and every block fetches the run lists, as before), each render is the oracle's bit for bit -- the bus, the reports, the block peaks
and the RMS extension of the last call -- and the two renders equal each other in the bus, the levels and the reports.

ZL_K2_PAIR=2 and ZL_K2_PHASE_ORDER=2 give every launch of these shapes to zl_k2_pair_phase_render (tests/test_k2_launch_cpu.py holds the
table).  Shapes: 2 buses x 16 voices, blocks of 256 frames, calls of 96 blocks, loops of 600..1500 frames at ratio 1 -- a window holds far
more passes than a run list has runs, so from its second call on a steady loop has no inline run at all (ZlPlanner::replay_cached_pass)."""
import ctypes as C

import numpy as np
import pytest

from scenario import Scene, compare_runs, play_cmd, rand_source, run_backend, run_oracle, stop_cmd
from test_k2_pair import check_levels

pytestmark = pytest.mark.gpu

FS = 48000.0
CALL = 96


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def scene(seed, *, nblocks, num_buses=2, vpb=16, long_loops=(), mono=(), pitched=(), idle=(), oneshots=None, decay=(), events=None):
    """stereo sample-space loops of 600..1500 frames at the playback rate (note 60, source at the engine's rate).  long_loops: voices whose
    loop is about 40 blocks; mono / pitched (note 67): voices of those kinds; idle: clips never played (their voice slots stay idle);
    oneshots: {voice: source frames} played once; decay: voices with a decay of one second (no block of theirs is in sustain: no inline run);
    events: {block: [event, ...]} added to the scene"""
    rng = np.random.default_rng(seed)
    sc = Scene(num_buses=num_buses, voices_per_bus=vpb, fs=FS, mode=0, mix_group=0, nframes=256, nblocks=nblocks, bpm=120)
    oneshots = oneshots or {}
    V = num_buses * vpb
    for i in range(V):
        frames = int(rng.integers(600, 1501))
        if i in long_loops:
            frames = 40 * 256 + int(rng.integers(0, 200))
        n = oneshots.get(i, frames + 2000)
        L, R = rand_source(rng, n, stereo=i not in mono)
        sc.sounds.append((L, R, FS))
        beats = frames / 24000.0                                     # 120 bpm: a beat is 24000 frames
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))

        def setup(lib, clip, beats=beats, vol=vol, pan=pan, loop=i not in oneshots, slow=i in decay):
            if loop:
                lib.zlo_clip_set_length(clip, C.c_float(beats), 120)
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
            if slow:
                clip.adsr.p.attack, clip.adsr.p.decay, clip.adsr.p.sustain, clip.adsr.p.release = 0.0, 1.0, 0.5, 0.0
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // vpb - 2, loop=i not in oneshots, note=67 if i in pitched else 60,
                                     volume=float(np.float32(rng.uniform(0.2, 1.0)))), int(rng.integers(0, 50)))
                    for i in range(V) if i not in idle]
    for k, evs in (events or {}).items():
        sc.events.setdefault(k, []).extend(evs)
    return sc


def report_rows(rep, V):
    return [(bool(rep[v].playing), rep[v].source_sample_position, rep[v].valid, rep[v].gain, rep[v].progress) for v in range(V)]


def both(monkeypatch, sc, factory, *, levels=True, **kw):
    """oracle parity with the switch at 1 and at 0; the two renders agree bit for bit in the bus, the levels and the reports"""
    V = sc.num_buses * sc.voices_per_bus
    monkeypatch.setenv("ZL_K2_PAIR", "2")
    monkeypatch.setenv("ZL_K2_PHASE_ORDER", "2")
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    outs = []
    for sw in ("1", "0"):
        monkeypatch.setenv("ZL_K2_STAGE_NORUN", sw)
        bus, rep, syn, _ = run_backend(sc, factory, batch=CALL, **kw)
        try:
            compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
            peaks = lv = None
            if levels:
                check_levels(syn, ref_bus, sc.nframes)
                peaks = np.array(syn.block_peaks(), copy=True)
                K = syn._last[0]
                lv = []
                for k in range(0, K, 7):
                    tick = syn.levels_tick(block_index=k)
                    lv += [(tick[b].rms_a, tick[b].rms_b) for b in range(sc.num_buses)]
            outs.append((bus.copy(), peaks, lv, report_rows(rep, V)))
        finally:
            syn.close()
    a, b = outs
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
    if levels:
        assert np.array_equal(a[1], b[1])
        assert np.array_equal(np.array(a[2], np.float64).view(np.int64), np.array(b[2], np.float64).view(np.int64))
    assert a[3] == b[3]
    return ref_bus


# (a) all loops steady: the second call replays the cached passes -- no voice has an inline run, run_end is 0 and every workgroup stages
#     without the run lists; in the first call the passes before the periodic part are inline runs, so it has blocks on both sides
def test_all_loops_steady(Engine, monkeypatch):
    both(monkeypatch, scene(0x2A01, nblocks=2 * CALL), Engine)


# (b) one long loop per bus (about 40 blocks: a call's two or three passes fit the run list, n > 0): the same launch has blocks on both
#     sides of run_end, in every call
def test_one_long_loop_per_bus(Engine, monkeypatch):
    both(monkeypatch, scene(0x2A02, nblocks=2 * CALL, long_loops=(5, 16 + 11)), Engine)


# (c) idle voice slots, one-shots that end inside a window (0 < dead_from < K) -- one in sustain, which is an inline run up to its end,
#     one under a one-second decay, which has none -- a one-shot started with the second call, and a loop stopped by a command between
#     the calls: all in buses whose other voices have no inline run in the second call.  The dense dead_from decides who plays.
def test_idle_slots_and_early_ends(Engine, monkeypatch):
    vpb = 16
    oneshots = {2: 50 * 256 + 77, 7: 130 * 256 + 5, 16 + 3: 61 * 256 + 200, 16 + 9: 30 * 256 + 31}
    events = {CALL: [("cmd", stop_cmd(4, midi_channel=4 // vpb - 2, note=60), 0),
                     ("cmd", stop_cmd(16 + 12, midi_channel=(16 + 12) // vpb - 2, note=60), 0),
                     ("cmd", play_cmd(16 + 9, midi_channel=(16 + 9) // vpb - 2, loop=False, note=60, volume=0.8), 10)]}
    sc = scene(0x2A03, nblocks=2 * CALL, idle=(0, 13, 16 + 9, 16 + 15), oneshots=oneshots, decay=(7, 16 + 3), events=events)
    ref_bus = both(monkeypatch, sc, Engine)
    assert np.abs(ref_bus[:, :, CALL * 256:]).max() > 0.0


# (d) windows of 32 blocks (the record sets and their order buffers alternate, three windows per call) and three calls queued without a
#     synchronise: each window's tail is read by the launch it was written for
def test_short_windows_three_calls_queued(Engine, monkeypatch):
    sc = scene(0x2A04, nblocks=3 * CALL, long_loops=(3,), oneshots={16 + 6: 70 * 256 + 9})
    both(monkeypatch, sc, Engine, levels=False, pipelined=True, plan_window_blocks=32)
    both(monkeypatch, sc, Engine, plan_window_blocks=32)


# (e) a mono voice among stereo ones and one pitched voice: the chunk classes that are not on-grid, staged without the run lists
def test_mono_and_pitched_voices(Engine, monkeypatch):
    both(monkeypatch, scene(0x2A05, nblocks=2 * CALL, mono=(6, 16 + 1), pitched=(9, 16 + 14)), Engine)
