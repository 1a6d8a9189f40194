"""K2's on-grid form (zl_k2_chunk_ongrid, zl_render.h): unit-step voices at integer positions of sources known to be finite are mixed
from ONE tap.  Parity against the oracle, bit for bit (bus compared as int32, reports of the call's last block included), with the
form on (ZL_K2_ONGRID=1, the default) and off (0), the two renders compared with each other, and for the batch forms in time order
(ZL_K2_PHASE_ORDER=0) and phase order (2).  A test cannot see which variant ran: the scenes are built so that interior blocks of
ratio-1 loops -- the on-grid class -- are most of the work, next to the blocks at loop restarts, which take the older paths.

NaN frames (a source that holds NaN or an infinity) are compared as "NaN in the same frames": the payload and sign of a NaN that an
invalid operation creates (inf * 0, inf - inf) are the platform's choice -- x86 makes 0xffc00000, the GPU 0x7fc00000."""
import ctypes as C

import numpy as np
import pytest

from scenario import Scene, compare_runs, play_cmd, rand_source, run_backend, run_oracle

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
ADVERSARIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, 1.0, -1.0], dtype=np.float32)


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


def loop_scene(seed, *, num_buses, voices_per_bus, nframes=256, nblocks=120, mode=0, stereo_p=1.0, notes=(60,), start=False,
               sources=None):
    """sample-space loops at the playback rate (note 60 of a source at the engine's rate: step exactly 1, integer positions), loops of
    700..5000 frames: several restarts per voice over the call.  notes: drawn per voice (others than 60 are pitched: off the grid).
    start: a start position of an integer number of samples that is not 0."""
    rng = np.random.default_rng(seed)
    fs = 48000.0
    sc = Scene(num_buses=num_buses, voices_per_bus=voices_per_bus, fs=fs, mode=mode, mix_group=0, nframes=nframes, nblocks=nblocks, bpm=120)
    V = num_buses * voices_per_bus
    for i in range(V):
        n = int(rng.integers(6000, 12000))
        L, R = rand_source(rng, n, stereo=bool(rng.random() < stereo_p))
        if sources is not None:
            L, R = sources(rng, i, L, R)
        sc.sounds.append((L, R, fs))
        beats = float(rng.uniform(0.03, 0.2))
        vol, pan = float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1))
        st = float(int(rng.integers(1, 400)) / 48000.0 + 1e-7) if start else 0.0        # (a hair over k / fs: (int)(start * fs) = k)

        def setup(lib, clip, beats=beats, vol=vol, pan=pan, st=st):
            lib.zlo_clip_set_length(clip, C.c_float(beats), 120)
            lib.zlo_clip_set_start_position(clip, C.c_float(st))
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(vol))
            lib.zlo_clip_set_pan(clip, C.c_float(pan))
        sc.clip_setup[i] = setup
    sc.events[0] = [("cmd", play_cmd(i, midi_channel=i // voices_per_bus - 2, loop=True, note=int(rng.choice(notes)),
                                     volume=float(np.float32(rng.uniform(0.2, 1.0)))), int(rng.integers(0, 50))) for i in range(V)]
    return sc


def same_bits_nan_aware(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def _both(monkeypatch, sc, factory, V, *, orders=("0", "2"), nan_ok=False, **kw):
    """oracle parity with the on-grid form on and off, in time order and in phase order; all renders agree bit for bit"""
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    outs = []
    for order in orders:
        monkeypatch.setenv("ZL_K2_PHASE_ORDER", order)
        for og in ("1", "0"):
            monkeypatch.setenv("ZL_K2_ONGRID", og)
            bus, rep, syn, _ = run_backend(sc, factory, **kw)
            if nan_ok:
                assert same_bits_nan_aware(ref_bus, bus), (order, og)
                compare_runs(np.nan_to_num(ref_bus, nan=0.0), ref_rep, ref_syn, np.nan_to_num(bus, nan=0.0), rep, V, exact=False, tol=0.0)
            else:
                compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, V)
            outs.append(bus.copy())
            syn.close()
    for o in outs[1:]:
        assert np.array_equal(outs[0].view(np.int32), o.view(np.int32))
    return ref_bus


# (a) the headline shape and the reference's: wide and narrow buses of stereo loops at ratio 1
@pytest.mark.parametrize("buses,vpb,nblocks", [(8, 128, 60), (12, 8, 250)])
def test_ratio_one_stereo_loops(Engine, monkeypatch, buses, vpb, nblocks):
    sc = loop_scene(0x0E01 + buses, num_buses=buses, voices_per_bus=vpb, nblocks=nblocks)
    _both(monkeypatch, sc, Engine, buses * vpb, batch=1 << 30)


# (b) sources made of the adversarial finite values: signed zeros, denormals, +-FLT_MAX
def test_adversarial_finite_sources(Engine, monkeypatch):
    def sources(rng, i, L, R):
        for x in (L, R):
            pick = rng.random(x.size) < (0.9 if i % 3 == 0 else 0.3)
            x[pick] = ADVERSARIAL[rng.integers(0, len(ADVERSARIAL) - (2 if i % 2 else 0), int(pick.sum()))]
        if i % 5 == 0:
            L[:] = np.where(rng.random(L.size) < 0.5, np.float32(0.0), np.float32(-0.0)); R[:] = -L      # whole stretches of signed zeros
        return L, R
    sc = loop_scene(0x0E10, num_buses=3, voices_per_bus=16, nblocks=80, sources=sources)
    _both(monkeypatch, sc, Engine, 48, batch=1 << 30, nan_ok=True)       # (+FLT_MAX and -FLT_MAX of two voices meet: inf - inf in the bus)


# (c) one source with NaN and +-inf among seven clean ones in a chunk: the chunk falls back, the NaN frames are the oracle's
def test_a_non_finite_source_takes_its_chunk_back_to_two_taps(Engine, monkeypatch):
    def sources(rng, i, L, R):
        if i % 8 == 3:
            at = rng.integers(0, 3000, 40)                           # inside every loop (loops are 700 frames and longer: some hit)
            L[at[:10]] = np.nan; R[at[10:20]] = np.inf; L[at[20:30]] = -np.inf; R[at[30:]] = np.nan
            L[:600:7] = np.inf
        return L, R
    sc = loop_scene(0x0E20, num_buses=2, voices_per_bus=16, nblocks=80, sources=sources)
    ref_bus = _both(monkeypatch, sc, Engine, 32, batch=1 << 30, nan_ok=True)
    assert np.isnan(ref_bus).any() and not np.isnan(ref_bus).all(axis=2).any()


# (d) root-note and pitched voices on one bus, mono with stereo
def test_pitched_and_mono_voices_among_them(Engine, monkeypatch):
    sc = loop_scene(0x0E30, num_buses=4, voices_per_bus=32, nblocks=90, stereo_p=0.6, notes=(60, 60, 60, 48, 67, 72))
    _both(monkeypatch, sc, Engine, 128, batch=1 << 30)
    sc = loop_scene(0x0E31, num_buses=2, voices_per_bus=16, nblocks=90, stereo_p=0.0)        # whole chunks of mono voices: the mono twin
    _both(monkeypatch, sc, Engine, 32, batch=1 << 30)


# (e) start positions that are an integer number of samples, not 0
def test_integer_start_positions(Engine, monkeypatch):
    sc = loop_scene(0x0E40, num_buses=2, voices_per_bus=24, nblocks=90, start=True, stereo_p=0.8)
    _both(monkeypatch, sc, Engine, 48, batch=1 << 30)


# (f) a clip re-rendered with a gain and then played (the rendered extent has not been looked at: two taps), and back to identity
def test_rerendered_clip_and_back_to_identity(built, monkeypatch):
    import stretch_ref as sr_
    from libzl_amd.engine import synthetic_clocks
    from rerender_cases import source
    from test_rerender_gpu import _oracle_swap, _pair
    sr, N = 48000.0, 256
    src = source(sr, 2, 40000, seed=77)
    ref, _ = sr_.render(src, sr, -6.0, 0.0, 1.0)
    outs = {}
    for og in ("1", "0"):
        monkeypatch.setenv("ZL_K2_ONGRID", og)
        osyn, syn = _pair(0, src[0], src[1], sr, N)
        got = []
        try:
            for k0, n, swap in ((0, 6, None), (6, 8, ref), (14, 8, src)):
                if swap is ref:
                    syn.rerender_clip(0, gain_db=-6.0)
                    _oracle_swap(osyn, ref)
                elif swap is src:
                    syn.rerender_clip(0)
                    _oracle_swap(osyn, src)
                clk = synthetic_clocks(n, N, 48000.0, start_block=k0)
                bus, orep = osyn.render_batch(n, N, clk)
                syn.render_batch(n, N, clk)
                out = syn.read_bus()
                assert np.array_equal(out.view(np.int32), bus.view(np.int32)), (og, k0, np.abs(out - bus).max())
                rep = syn.voice_reports()
                for v in range(8):
                    assert (rep[v].valid, rep[v].gain, rep[v].progress) == (orep[v].valid, orep[v].gain, orep[v].progress), (og, k0, v)
                got.append(out.copy())
        finally:
            syn.close()
        outs[og] = np.concatenate(got, axis=2)
    assert np.array_equal(outs["1"].view(np.int32), outs["0"].view(np.int32))


# (g) the three ways in: host upload (every test above), device upload, device upload behind a producer stream
@pytest.mark.parametrize("how", ["device", "device_on"])
def test_device_uploads(Engine, monkeypatch, how):
    import torch
    keep = []

    def factory(**kw):
        syn = Engine(**kw)

        def register(L, R, sr):
            tl = torch.from_numpy(L).cuda(); tr = torch.from_numpy(R).cuda() if R is not None else None
            keep.append((tl, tr))
            if how == "device":
                torch.cuda.synchronize()
                return syn.register_clip_device(tl.data_ptr(), tr.data_ptr() if tr is not None else None, L.shape[0], sr)
            return syn.register_clip_device_on(tl.data_ptr(), tr.data_ptr() if tr is not None else None, L.shape[0], sr,
                                               torch.cuda.current_stream().cuda_stream)
        syn.register_clip = register
        return syn

    def sources(rng, i, L, R):
        if i == 5:
            L[100] = np.nan; R[2000] = -np.inf                       # the device scan has to find them: this voice's chunk keeps two taps
        return L, R
    sc = loop_scene(0x0E50, num_buses=2, voices_per_bus=16, nblocks=80, stereo_p=0.8, sources=sources)
    ref_bus = _both(monkeypatch, sc, factory, 32, orders=("0",), nan_ok=True, batch=1 << 30)
    assert np.isnan(ref_bus).any()


# (h) the resident real-time kernel, cycle by cycle, at 64 and 256 frames
@pytest.mark.parametrize("nframes", [64, 256])
def test_resident_kernel(built, monkeypatch, nframes):
    from test_rt_persistent import _play_blockwise
    monkeypatch.setenv("ZL_RT_PERSISTENT", "1")
    sc = loop_scene(0x0E60 + nframes, num_buses=12, voices_per_bus=8, nframes=nframes, nblocks=60, stereo_p=0.8)
    ref_bus, ref_rep, ref_syn = run_oracle(sc)
    outs = []
    for og in ("1", "0"):
        monkeypatch.setenv("ZL_K2_ONGRID", og)
        bus, rep, syn = _play_blockwise(sc)
        starts, cycles = syn.rt_stats()
        assert cycles == sc.nblocks and starts >= 1
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, 96)
        outs.append(bus.copy())
        syn.close()
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))


# (i) FIX_DELAY: the same mix, another store
def test_fix_delay(Engine, monkeypatch):
    sc = loop_scene(0x0E70, num_buses=2, voices_per_bus=40, nblocks=90, mode=2, stereo_p=0.8)
    _both(monkeypatch, sc, Engine, 80, batch=1 << 30)


# modes in which the form must stay off (Hermite, FIX_GAIN): still the oracle's bits with the switch on
@pytest.mark.parametrize("mode", [1, 4])
def test_other_modes_unchanged(Engine, monkeypatch, mode):
    sc = loop_scene(0x0E80 + mode, num_buses=2, voices_per_bus=16, nblocks=60, mode=mode)
    _both(monkeypatch, sc, Engine, 32, orders=("0",), batch=1 << 30)
