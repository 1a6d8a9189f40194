"""The pair kernels' one-tap path for voice-blocks that hold one loop restart (zl_k2_chunk_ongrid_pair_wrap, zl_kernels.hip; zl_voice_ongrid2,
zl_render.h): a chunk whose voices are all on-grid, one or more of them restarting inside the block, is mixed from the first tap of each
frame's own segment instead of going through the two-tap chunk functions frame by frame.  Nothing it computes from changes, so the bits must
not: every scene is rendered with ZL_K2_PAIR_WRAP at 1 and at 0 (the parent's classes), in time order (ZL_K2_PHASE_ORDER=0) and in phase
order (2), with ZL_K2_PAIR=2; each render is the oracle's bit for bit -- the bus, the reports of the last block, the block peaks and the RMS
extension of the last call -- and the renders equal each other in the bus, the levels and the reports.

Shapes: blocks of 256 frames, ONE bus of 8 or 16 voices (one or two chunks; two buses of 8 would be packed two to a workgroup, which the pair
kernels do not take), 24 to 40 blocks in two calls.  The scenes are tests/k2_pair_wrap_scenes.py's;
a GPU test cannot see which chunk function ran, so tests/test_k2_pair_wrap_cpu.py counts, with the host planner, the voice-blocks of each
scene that are eligible, holds every case listed there to occur, and holds every scene's shape to the launch table: the pair kernels in both orders."""
import numpy as np
import pytest

import k2_pair_wrap_scenes as scenes
from scenario import compare_runs, run_backend, run_oracle
from test_k2_ongrid import same_bits_nan_aware
from test_k2_pair import check_levels
from test_k2_stage_norun import report_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def every_way(monkeypatch, name, factory, *, nan_ok=False):
    sc = scenes.scene(name)
    V = sc.num_buses * sc.voices_per_bus
    monkeypatch.setenv("ZL_K2_PAIR", "2")
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    outs = []
    for order in ("0", "2"):
        monkeypatch.setenv("ZL_K2_PHASE_ORDER", order)
        for sw in ("1", "0"):
            monkeypatch.setenv("ZL_K2_PAIR_WRAP", sw)
            bus, rep, syn, _ = run_backend(sc, factory, batch=scenes.calls(sc))
            try:
                if nan_ok:
                    assert same_bits_nan_aware(ref_bus, bus), (order, sw)
                    compare_runs(np.nan_to_num(ref_bus, nan=0.0), ref_rep, ref_syn, np.nan_to_num(bus, nan=0.0), rep, V, exact=False, tol=0.0)
                else:
                    compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
                check_levels(syn, ref_bus, sc.nframes)
                peaks = np.array(syn.block_peaks(), copy=True)
                lv = []
                for k in range(0, syn._last[0], 5):
                    tick = syn.levels_tick(block_index=k)
                    lv += [(tick[b].rms_a, tick[b].rms_b) for b in range(sc.num_buses)]
                outs.append((bus.copy(), peaks, np.array(lv, np.float64), report_rows(rep, V)))
            finally:
                syn.close()
    for o in outs[1:]:
        assert np.array_equal(outs[0][0].view(np.int32), o[0].view(np.int32))
        assert np.array_equal(outs[0][1], o[1])
        assert np.array_equal(outs[0][2].view(np.int64), o[2].view(np.int64))
        assert outs[0][3] == o[3] or nan_ok and str(outs[0][3]) == str(o[3])
    return ref_bus


# every listed n1 (1, 2, 127, 128, 129, 254, 255), odd and even; loop start 0 with the clip first in the arena, odd and even starts; stereo;
# seven voices restarting in one block
def test_listed_n1_values_and_starts(Engine, monkeypatch):
    every_way(monkeypatch, "n1_values", Engine)


# a mono chunk, all eight voices restarting in one block
def test_mono_chunk_all_eight_restart_in_one_block(Engine, monkeypatch):
    every_way(monkeypatch, "mono_all_eight", Engine)


# a mixed-layout chunk and a chunk with one pitched voice: both stay general
def test_mixed_layout_and_pitched_chunks(Engine, monkeypatch):
    every_way(monkeypatch, "mixed_and_pitched", Engine)


# a loop shorter than a block (more than two segments) and a loop that ends at the source's last frame (not interior): not eligible
def test_short_loop_and_loop_ending_at_the_last_frame(Engine, monkeypatch):
    every_way(monkeypatch, "short_and_edge", Engine)


# a source with a non-finite sample (its flag is off) and beat-locked restarts (lengthInBeats an integer)
def test_non_finite_source_and_beat_locked_restarts(Engine, monkeypatch):
    every_way(monkeypatch, "non_finite_and_beat", Engine)


# restarts in the last block of each call: the report path
def test_restart_in_the_calls_last_block(Engine, monkeypatch):
    every_way(monkeypatch, "last_block", Engine)


# the adversarial finite values of test_k2_ongrid.ADVERSARIAL around the restart, stereo and mono
def test_adversarial_values_around_the_restart(Engine, monkeypatch):
    every_way(monkeypatch, "adversarial", Engine, nan_ok=True)
