"""GPU tier: the HIP engine through the C-ABI against tests/golden/ref_*.npz -- scenes recorded from the reference's OWN compiled voice
(tests/golden/make_reference_golden.py) -- bit for bit: one block per call, the whole scene in one batch, the resident real-time
kernel cycle by cycle, each with K2's on-grid form on and off (ZL_K2_ONGRID).  Reads tests/golden/ only.

NaN frames (ref_11: +FLT_MAX and -FLT_MAX meet in the bus) are compared as "NaN in the same frames", as tests/test_k2_ongrid.py does."""
import numpy as np
import pytest

import test_rt_persistent as rt
from golden_util import load_reference_fixture, reference_fixture_names
from ref_voice import same_bits_nan_aware
from scenario import run_backend

pytestmark = pytest.mark.gpu

NAMES = reference_fixture_names()


def _check(name, sc, ex, bus, rep):
    d = np.argwhere(bus.view(np.int32) != ex["bus"].view(np.int32))
    assert same_bits_nan_aware(bus, ex["bus"]), f"{name}: {len(d)} samples differ from the reference voice, first at [bus, channel, frame] {d[:2].tolist()}"
    for v in range(sc.num_buses * sc.voices_per_bus):
        want = ex["reports"][-1, v]
        assert bool(rep[v].playing) == bool(ex["playing"][-1, v]), (name, v)
        assert int(rep[v].valid) == int(want[0]), (name, v)
        if want[0]:
            assert np.float32(rep[v].gain) == want[1] and np.float32(rep[v].progress) == want[2], (name, v)


def test_the_fixtures_are_there():
    assert len(NAMES) == 12


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ongrid", ["1", "0"])
@pytest.mark.parametrize("batch", [1, 1 << 30])
def test_engine_batches_reproduce_the_reference_fixture(built, monkeypatch, name, ongrid, batch):
    from libzl_amd import SamplerSynth
    monkeypatch.setenv("ZL_K2_ONGRID", ongrid)
    sc, ex = load_reference_fixture(name)
    bus, rep, syn, _ = run_backend(sc, SamplerSynth, batch=batch)
    try:
        _check(name, sc, ex, bus, rep)
    finally:
        syn.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ongrid", ["1", "0"])
def test_resident_kernel_reproduces_the_reference_fixture(built, monkeypatch, name, ongrid):
    monkeypatch.setenv("ZL_K2_ONGRID", ongrid)
    monkeypatch.setenv("ZL_RT_PERSISTENT", "1")
    sc, ex = load_reference_fixture(name)
    bus, rep, syn = rt._play_blockwise(sc)
    try:
        _check(name, sc, ex, bus, rep)
    finally:
        syn.close()
