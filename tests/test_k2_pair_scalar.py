"""The pair kernels' fast workgroups (ZL_K2_PAIR_SCALAR; zl_kernels.hip: zl_k1c_assemble leaves, per on-grid voice-block, the address of the
block's frame 0 and, per chunk of 8 voices, a bit; a workgroup of zl_k2_pair_phase_render whose bus is on-grid in every chunk of its block reads
addresses and pans with scalar loads and does not stage).  The loads, the order of the voices and the mix are the staged path's, so the bits must
not move: every scene is rendered with the switch at 1 and at 0 and in both orders (ZL_K2_PHASE_ORDER 2 and 0: in time order no workgroup is fast),
each render is the oracle's bit for bit -- the bus, the reports, the block peaks and the RMS extension of the last call -- and the renders equal
each other.  ZL_K2_PAIR=2 gives every launch to the pair kernels.  Which workgroups are fast a GPU test cannot see:
tests/test_k2_pair_scalar_cpu.py makes every scene's records with the host planner and holds the counts."""
import numpy as np
import pytest

import k2_pair_scalar_scenes as scenes
from scenario import compare_runs, run_backend, run_oracle
from test_k2_pair import check_levels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def report_rows(rep, V):
    return [(bool(rep[v].playing), rep[v].source_sample_position, rep[v].valid, rep[v].gain, rep[v].progress) for v in range(V)]


def render_all_ways(monkeypatch, name, Engine):
    sc = scenes.scene(name)
    V = sc.num_buses * sc.voices_per_bus
    factory = Engine
    if name in scenes.ARENA_BYTES:                                   # an arena too small for the scene's sources: the later ones land in grown segments
        def factory(**kw):
            kw["sound_arena_bytes"] = scenes.ARENA_BYTES[name]
            return Engine(**kw)
    monkeypatch.setenv("ZL_K2_PAIR", "2")
    ref_bus, ref_rep, ref_syn = run_oracle(sc, batch=sc.call)
    outs = []
    for order in ("2", "0"):
        for sw in ("1", "0"):
            monkeypatch.setenv("ZL_K2_PHASE_ORDER", order)
            monkeypatch.setenv("ZL_K2_PAIR_SCALAR", sw)
            bus, rep, syn, _ = run_backend(sc, factory, batch=sc.call)
            try:
                compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)          # the bus and the reports (gains and positions) of the last call
                check_levels(syn, ref_bus, sc.nframes)               # block peaks and the RMS extension of the last call
                peaks = np.array(syn.block_peaks(), copy=True)
                lv = []
                for k in range(0, syn._last[0], 7):
                    tick = syn.levels_tick(block_index=k)
                    lv += [(tick[b].rms_a, tick[b].rms_b) for b in range(sc.num_buses)]
                if name in scenes.ARENA_BYTES:
                    assert syn.memory_bytes()[1] > scenes.ARENA_BYTES[name]   # the arena did grow
                outs.append((bus.copy(), peaks, np.array(lv, np.float64), report_rows(rep, V)))
            finally:
                syn.close()
    a = outs[0]
    for b in outs[1:]:
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
        assert a[3] == b[3]
    return ref_bus


@pytest.mark.parametrize("name", scenes.POSITIVE + scenes.NEGATIVE)
def test_scene(Engine, monkeypatch, name):
    ref_bus = render_all_ways(monkeypatch, name, Engine)
    assert np.abs(ref_bus[:, :, -scenes.N * scenes.CALL:]).max() > 0.0          # the last call is not silence
