"""CPU tier: tests/golden/ref_*.npz -- scenes recorded from the reference's OWN compiled voice (tests/golden/make_reference_golden.py) --
reproduced bit for bit by the C oracle, by the numpy restatement and by the engine's kernel code built for the host.  Needs neither the
reference tree nor its library: the fixtures carry the reference's results to every machine (tests/test_reference_golden_gpu.py holds
the HIP engine to the same files)."""
import dataclasses

import numpy as np
import pytest

import test_numpy_twin_random as twin
from golden_util import load_reference_fixture, reference_fixture_names
from oracle import zl_oracle as zo
from ref_voice import same_bits_nan_aware
from scenario import oracle_cmd, run_backend, run_oracle

NAMES = reference_fixture_names()


def test_the_fixtures_are_there():
    assert len(NAMES) == 12


def _oracle_blockwise(sc):
    """the C oracle through its own handleCommand, one block per call: bus, every block's reports, isPlaying after every block"""
    osyn = zo.OracleSynth(sc.num_buses, sc.voices_per_bus, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    for i, (L, R, sr) in enumerate(sc.sounds):
        assert osyn.register_clip(L, R, sr) == i
        if i in sc.clip_setup:
            sc.clip_setup[i](osyn.lib, osyn.clips[i])
    V, K, N = sc.num_buses * sc.voices_per_bus, sc.nblocks, sc.nframes
    bus = np.zeros((sc.num_buses, 2, K * N), dtype=np.float32)
    reports, playing = np.zeros((K, V, 3), dtype=np.float32), np.zeros((K, V), dtype=np.uint8)
    for k in range(K):
        for ev in sc.events.get(k, []):
            if ev[0] == "cmd":
                osyn.handle_clip_command(oracle_cmd(**ev[1]), ev[2])
            elif ev[0] == "start":
                osyn.start_voice(ev[1], ev[2], oracle_cmd(**ev[3]), ev[4])
            elif ev[0] == "update":
                osyn.update_voice(ev[1], ev[2], oracle_cmd(**ev[3]))
            elif ev[0] == "stopv":
                osyn.stop_voice(ev[1], ev[2], ev[3])
            else:
                raise AssertionError(ev[0])
        b, rep = osyn.render_batch(1, N, sc.make_clocks(k, 1))
        bus[:, :, k * N:(k + 1) * N] = b
        for v in range(V):
            reports[k, v] = (rep[v].valid, rep[v].gain, rep[v].progress)
            playing[k, v] = osyn.voices[v].isPlaying
    return bus, reports, playing


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_fixture(built, name):
    sc, ex = load_reference_fixture(name)
    bus, reports, playing = _oracle_blockwise(sc)
    assert np.nanmax(np.abs(ex["bus"])) > 0
    assert same_bits_nan_aware(bus, ex["bus"]), f"first difference at {np.argwhere(bus.view(np.int32) != ex['bus'].view(np.int32))[:2].tolist()}"
    assert np.array_equal(playing, ex["playing"])
    assert same_bits_nan_aware(reports, ex["reports"])
    # the frame the reference stores to [nframes]: what ZLO_MODE_FIX_DELAY (frame f to [f], same arithmetic) keeps as each block's last frame
    fix, _, _ = run_oracle(dataclasses.replace(sc, mode=zo.MODE_FIX_DELAY))
    N = sc.nframes
    assert same_bits_nan_aware(np.ascontiguousarray(fix[:, :, N - 1::N].transpose(2, 0, 1)), ex["tail"])
    assert same_bits_nan_aware(np.ascontiguousarray(fix.reshape(sc.num_buses, 2, sc.nblocks, N)[:, :, :, :N - 1]),
                               np.ascontiguousarray(ex["bus"].reshape(sc.num_buses, 2, sc.nblocks, N)[:, :, :, 1:]))


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_reproduces_the_reference_fixture(name):
    sc, ex = load_reference_fixture(name)
    with np.errstate(all="ignore"):                                    # (ref_11: FLT_MAX sources overflow on purpose)
        bus, rep, syn = twin.run_numpy(sc)
    assert same_bits_nan_aware(bus, ex["bus"]), f"first difference at {np.argwhere(bus.view(np.int32) != ex['bus'].view(np.int32))[:2].tolist()}"
    VPB = sc.voices_per_bus
    for b in range(sc.num_buses):
        for i, v in enumerate(syn.voices[b]):
            assert bool(v.is_playing) == bool(ex["playing"][-1, b * VPB + i]), (b, i)
            want = ex["reports"][-1, b * VPB + i]
            assert bool(want[0]) == ((b, i) in rep and bool(rep[(b, i)][0])), (b, i)
            if want[0]:
                assert np.float32(rep[(b, i)][1]) == want[1] and np.float32(rep[(b, i)][2]) == want[2], (b, i)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("batch", [1, 1 << 30])
def test_kernel_code_on_host_reproduces_the_reference_fixture(built, name, batch):
    from cpu_harness.sim import SimSynth
    sc, ex = load_reference_fixture(name)
    bus, rep, syn, _ = run_backend(sc, SimSynth, batch=batch)
    assert same_bits_nan_aware(bus, ex["bus"]), f"first difference at {np.argwhere(bus.view(np.int32) != ex['bus'].view(np.int32))[:2].tolist()}"
    for v in range(sc.num_buses * sc.voices_per_bus):
        want = ex["reports"][-1, v]
        assert bool(rep[v].playing) == bool(ex["playing"][-1, v]), v
        assert int(rep[v].valid) == int(want[0]), v
        if want[0]:
            assert np.float32(rep[v].gain) == want[1] and np.float32(rep[v].progress) == want[2], v
