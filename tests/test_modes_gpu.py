"""GPU tier: every value of the engine's `mode` on the device.  `mode` sums ZLHIP_MODE_FIX_GAIN (1), ZLHIP_MODE_FIX_DELAY (2) and
ZLHIP_MODE_HERMITE (4); zl_launch_render and zl_launch_rt_loop dispatch all eight values, and the rest of the tier creates engines in modes
0 to 4 only.  Here every mode runs on every non-staged K2 launch shape (tests/mode_cases.py; tests/test_modes_cpu.py holds the table to the
launch decision: each row reaches the kernel its name says, together all 32 instantiations), through the offline bounce with direct and
with copy-engine delivery, through the resident real-time kernel on narrow and on wide buses, through the fused fan-out, and -- one case
added to tests/group_cases.py -- through an engine group's spanning-bus sum.

Everything is held to the oracle bit for bit (int32 views): audio, voice state and reports, the integer block peaks and the RMS extension
(tile offset 0 in the modes with ZLHIP_MODE_FIX_DELAY, else 1; they are read from a row's LAST call, which the table keeps at three blocks or
more of the kernel the row's name says), the 16-bit format of the bounce, the six fan-out rows per bus.  In the modes
with ZLHIP_MODE_FIX_DELAY some bus must hold a non-zero sample in frame 0 of some block, in the others frame 0 of every block must be +0: the
two forms of a block's stores are told apart in every test.

(ZLHIP_MODE_FIX_GAIN changes nothing next to ZLHIP_MODE_HERMITE -- zl_mix_frame's four-tap form has the whole-sample gain by definition --, so
a launcher that took mode 4's kernels for mode 5 would compute the same bits: DESIGN.md section 0 lists what was shown to fail these tests.)

The bounce runs its whole cross product (6 modes x 5 block lengths x 2 formats x 2 deliveries): no pair is dropped."""
import numpy as np
import pytest

from level_checks import check_levels
from mode_cases import (BATCH_CASES, BOUNCE_MODES, BOUNCE_SHAPES, FANOUT_BATCH, FANOUT_RT, FIX_DELAY, RT_CASES, RT_CYCLES, RT_NARROW, RT_WIDE,
                        bounce_scene, case_id, rt_scene)
from oracle import np_restatement as npr
from scenario import compare_runs, random_scene, run_backend, run_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(built):
    from libzl_amd import SamplerSynth
    return SamplerSynth


_oracle = {}


def oracle_of(key, sc, threads=1):
    """(bus, reports, synth) of the oracle's run of the scene: computed once per session, the bus read-only"""
    if key not in _oracle:
        bus, rep, osyn = run_oracle(sc, threads=threads)
        bus.setflags(write=False)
        _oracle[key] = (bus, rep, osyn)
    return _oracle[key]


def setenv(monkeypatch, env):
    monkeypatch.delenv("ZL_K2_STAGED", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_frame0(rows, mode, what):
    """rows: frame 0 of every block, any shape.  The delayed store of the reference leaves +0 there (quirk Q2); ZLHIP_MODE_FIX_DELAY stores the
    block's first sample"""
    rows = np.ascontiguousarray(rows)
    if mode & FIX_DELAY:
        assert (rows != 0).any(), f"{what}: frame 0 of every block is zero in mode {mode}"
    else:
        assert not rows.view(np.int32 if rows.dtype == np.float32 else rows.dtype).any(), f"{what}: frame 0 of a block is not +0 in mode {mode}"


def frame0(bus, N):
    """[B][2][K * N] -> [B][2][K]"""
    return bus.reshape(bus.shape[0], 2, -1, N)[..., 0]


# ---- (a) the batch matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BATCH_CASES, ids=case_id)
def test_every_mode_on_every_batch_shape(Engine, monkeypatch, case):
    setenv(monkeypatch, case.env)
    sc = case.make_scene()
    ref_bus, ref_rep, ref_syn = oracle_of(case.id, sc)
    bus, rep, syn, _ = run_backend(sc, Engine, **case.run)
    try:
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, sc.num_buses * sc.voices_per_bus)
        check_levels(syn, ref_bus, sc.nframes, off=0 if case.mode & FIX_DELAY else 1)
        check_frame0(frame0(bus, sc.nframes), case.mode, case.id)
    finally:
        syn.close()


# ---- (b) the offline bounce --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nframes", sorted(BOUNCE_SHAPES))
@pytest.mark.parametrize("mode", BOUNCE_MODES)
def test_bounce_direct_and_through_the_copy_engine(Engine, monkeypatch, mode, nframes):
    """zlhip_bounce in ragged sub-batches: the render kernel's own stores into the caller's page-locked buffer (store_bus, the A.host_out
    branch, whose frame 0 goes by ZLHIP_MODE_FIX_DELAY) and the copy-engine delivery (ZL_BOUNCE_DIRECT=0, or a pageable destination), fp32
    and the recorder's 16-bit format: the oracle's bus, npr.pcm16 of it, and the same bytes both ways.
    The engine does not say which delivery a bounce took (a page-locked destination without a device view would fall back to copies, and
    the two legs would still agree): that the `direct` leg runs the kernel's own stores on an MI355X is shown by the mutation of that
    branch listed in DESIGN.md section 0, which fails this test and nothing else."""
    setenv(monkeypatch, {})
    sub, how = BOUNCE_SHAPES[nframes]
    sc = bounce_scene(mode, nframes)
    V = sc.num_buses * sc.voices_per_bus
    ref_bus, ref_rep, ref_syn = oracle_of(("bounce", mode, nframes), sc)
    want_pcm = np.stack([npr.pcm16(ref_bus[:, 0]), npr.pcm16(ref_bus[:, 1])], axis=2)
    for fmt in ("f32", "pcm16"):
        outs = []
        for delivery in ("direct", "copy"):
            monkeypatch.delenv("ZL_BOUNCE_DIRECT", raising=False)
            extra = ()
            if delivery == "copy" and how == "env":
                monkeypatch.setenv("ZL_BOUNCE_DIRECT", "0")
            elif delivery == "copy":
                extra = ("pageable",)
            out, rep, syn, _ = run_backend(sc, Engine, bounce=(fmt, sub) + extra)
            try:
                what = f"mode {mode}, {nframes} frames, {fmt}, {delivery}"
                if fmt == "f32":
                    compare_runs(ref_bus, ref_rep, ref_syn, out, rep, V)
                    check_frame0(frame0(out, nframes), mode, what)
                else:
                    assert np.array_equal(out, want_pcm), (what, np.argwhere(out != want_pcm)[:4].tolist())
                    check_frame0(out.reshape(sc.num_buses, -1, nframes, 2)[:, :, 0], mode, what)
            finally:
                syn.close()
            outs.append(out)
        assert outs[0].tobytes() == outs[1].tobytes(), (mode, nframes, fmt)


# ---- (c) the resident real-time kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,mode,kw,period", RT_CASES, ids=[f"{c[0]}-mode{c[1]}" for c in RT_CASES])
def test_resident_kernel_in_every_mode(built, monkeypatch, what, mode, kw, period):
    """zl_k_rt_loop<mode, wide>: 24 cycles with commands and clip edits between them, fed cycle by cycle through zlhip_render; narrow buses
    (one workgroup per bus) and buses of 40 voices (one workgroup per voice); one launch of the kernel renders all of them"""
    from test_rt_persistent import _play_blockwise
    setenv(monkeypatch, {"ZL_RT_PERSISTENT": "1"})
    monkeypatch.delenv("ZL_RT_WIDE", raising=False)
    sc = rt_scene(what, mode, kw, period)
    ref_bus, ref_rep, ref_syn = oracle_of(("rt", what, mode), sc, threads=8 if what == "wide" else 1)
    bus, rep, syn = _play_blockwise(sc)
    try:
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, sc.num_buses * sc.voices_per_bus)
        assert syn.rt_stats() == (1, RT_CYCLES)
        check_frame0(frame0(bus, period), mode, f"{what}, mode {mode}")
    finally:
        syn.close()


# ---- (d) the fused fan-out ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", FANOUT_BATCH)
def test_fused_fanout_of_a_batch(Engine, monkeypatch, name, mode):
    """store_bus (bpw2, bpw1_narrow) and zl_k3_body (mix_groups) write the six JackPassthrough rows from the registers that hold the mix; where
    they put the block's first sample goes by ZLHIP_MODE_FIX_DELAY"""
    from test_rt_fanout import _oracle_fanout, _zoo
    case = next(c for c in BATCH_CASES if (c.name, c.mode) == (name, mode))
    setenv(monkeypatch, case.env)
    sc = case.make_scene()
    zoo = _zoo()
    params = [zoo[(b + 1) % len(zoo)] for b in range(sc.num_buses)]
    ref_bus, ref_rep, ref_syn = oracle_of(case.id, sc)
    bus, rep, syn, _ = run_backend(sc, Engine, fanout=params, **case.run)
    try:
        compare_runs(ref_bus, ref_rep, ref_syn, bus, rep, sc.num_buses * sc.voices_per_bus)
        want, got = _oracle_fanout(ref_bus, params), syn.fan_result
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got.view(np.int32) != want.view(np.int32))[:4].tolist()
        check_frame0(frame0(bus, sc.nframes), mode, case.id)
        assert (got.reshape(sc.num_buses, 6, -1, sc.nframes)[..., 0] != 0).any()
    finally:
        syn.close()


@pytest.mark.parametrize("what,mode", FANOUT_RT)
def test_fused_fanout_on_the_real_time_cycle(built, monkeypatch, what, mode):
    """zlhip_render_fanout through the resident kernel, narrow and wide: every cycle's bus and six rows per bus"""
    from test_rt_fanout import _clock, _engines, _oracle_fanout, _zoo
    setenv(monkeypatch, {"ZL_RT_PERSISTENT": "1"})
    monkeypatch.delenv("ZL_RT_WIDE", raising=False)
    kw, N = RT_WIDE if what == "wide" else RT_NARROW
    sc = random_scene(0x3F80 + 8 * (what == "wide") + mode, nframes=64, nblocks=1, events=False, mode=mode, **kw)
    syn, osyn = _engines(sc, max_frames=max(64, N), mode=mode)
    try:
        zoo = _zoo()
        t, front = 0, False
        for k in range(RT_CYCLES):
            params = [zoo[(b + k // 3) % len(zoo)] for b in range(sc.num_buses)]      # a knob moves every third cycle
            clk, t = _clock(sc, t, N)
            L, R, fan = syn.process_fanout(N, clk, params)
            bus, _ = osyn.render_batch(1, N, [clk])
            assert np.array_equal(L.view(np.int32), bus[:, 0].view(np.int32)) and np.array_equal(R.view(np.int32), bus[:, 1].view(np.int32)), (what, mode, k)
            want = _oracle_fanout(bus, params)
            assert np.array_equal(fan.view(np.int32), want.view(np.int32)), (what, mode, k, np.argwhere(fan.view(np.int32) != want.view(np.int32))[:4].tolist())
            front = front or bool((L[:, 0] != 0).any() and (fan[:, :, 0] != 0).any())
        assert front                                                   # (both modes hold ZLHIP_MODE_FIX_DELAY)
        assert syn.rt_stats() == (1, RT_CYCLES)
    finally:
        syn.close()
