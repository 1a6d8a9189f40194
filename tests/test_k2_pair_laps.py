"""K2's two-slot workgroups (ZL_K2_PAIR_LAPS; zl_kernels.hip: a workgroup of zl_k2_pair_phase_render holds two neighbouring slots of its bus's
phase order, and where both blocks are fast zl_k2_pair_fast2 renders them in one pass over the voices, block B's load of a voice directly behind
block A's; every other workgroup renders its blocks one after the other).  Each block's voices are mixed in voice order into its own accumulators
by the operations of the one-block walk, so the bits must not move: every scene is rendered with the switch at 1 and at 2, each render is the
oracle's bit for bit -- the bus, the reports, the block peaks and the RMS extension of the last call -- and the two renders equal each other.
ZL_K2_PAIR=2 and ZL_K2_PHASE_ORDER=2 give every launch of two blocks and more to the phase-order pair kernel.  Which workgroups take the walk a
GPU test cannot see: tests/test_k2_pair_laps_cpu.py counts them for every scene with the host planner."""
import numpy as np
import pytest

import k2_pair_laps_scenes as scenes
from scenario import compare_runs, run_backend, run_oracle
from test_k2_pair import check_levels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def report_rows(rep, V):
    return [(bool(rep[v].playing), rep[v].source_sample_position, rep[v].valid, rep[v].gain, rep[v].progress) for v in range(V)]


@pytest.mark.parametrize("name", scenes.POSITIVE + scenes.NEGATIVE)
def test_scene(Engine, monkeypatch, name):
    sc = scenes.scene(name)
    V = sc.num_buses * sc.voices_per_bus
    monkeypatch.setenv("ZL_K2_PAIR", "2")
    monkeypatch.setenv("ZL_K2_PHASE_ORDER", "2")
    ref_bus, ref_rep, ref_syn = run_oracle(sc, batch=sc.call)
    outs = []
    for laps in ("1", "2"):
        monkeypatch.setenv("ZL_K2_PAIR_LAPS", laps)
        bus, rep, syn, _ = run_backend(sc, Engine, batch=sc.call)
        try:
            compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)      # the bus and the reports (gains and positions) of the last call
            check_levels(syn, ref_bus, sc.nframes)                   # block peaks and the RMS extension of the last call
            peaks = np.array(syn.block_peaks(), copy=True)
            lv = []
            for k in range(0, syn._last[0], 7):
                tick = syn.levels_tick(block_index=k)
                lv += [(tick[b].rms_a, tick[b].rms_b) for b in range(sc.num_buses)]
            outs.append((bus.copy(), peaks, np.array(lv, np.float64), report_rows(rep, V)))
        finally:
            syn.close()
    a, b = outs
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    assert a[3] == b[3]
    assert np.abs(ref_bus[:, :, -scenes.N * sc.call:]).max() > 0.0  # the last call is not silence


@pytest.mark.parametrize("name", ("bus_16", "two_buses_72", "edits"))
def test_queued_calls(Engine, monkeypatch, name):
    """the scene's calls queued on one stream, nothing read back or synchronised in between: the last block of one call, its report path and the
    first block of the next meet the two-slot workgroups while both calls are in flight"""
    sc = scenes.scene(name)
    V = sc.num_buses * sc.voices_per_bus
    monkeypatch.setenv("ZL_K2_PAIR", "2")
    monkeypatch.setenv("ZL_K2_PHASE_ORDER", "2")
    ref_bus, ref_rep, ref_syn = run_oracle(sc, batch=sc.call)
    outs = []
    for laps in ("1", "2"):
        monkeypatch.setenv("ZL_K2_PAIR_LAPS", laps)
        bus, rep, syn, _ = run_backend(sc, Engine, batch=sc.call, pipelined=True)
        try:
            compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
            outs.append((bus.copy(), report_rows(rep, V)))
        finally:
            syn.close()
    assert np.array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32)) and outs[0][1] == outs[1][1]
