"""The pair kernels' on-grid form for voice-blocks that hold one loop restart (libzl_amd/csrc/zl_render.h: zl_voice_ongrid2, zl_ongrid2_lane),
CPU tier: the predicate's truth table, the lane selection -- every n1, every lane, stereo and mono -- against zl_eval_control + zl_mix_frame<0>
with every address inside the source, and, with the host planner, the count of such voice-blocks in every scene of tests/test_k2_pair_wrap.py:
a GPU test cannot see which chunk function ran, so the cases it is there for are shown to occur here.  The harness is also built as a
program of its own under AddressSanitizer and UBSan and run here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import k2_pair_wrap_scenes as scenes
from libzl_amd import build
from scenario import run_backend

INT_MAX = 2 ** 31 - 1
N = 256
_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_pair_wrap_harness())
        l.zlwrap_predicate.argtypes = [C.c_uint] + [C.c_int] * 9 + [C.c_double] * 4 + [C.c_int]
        l.zlwrap_block.argtypes = [C.c_int, C.c_int, np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")] + [C.c_int] * 4 + [C.c_float] * 6 \
            + [np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
        l.zlwrap_scan.argtypes = [C.c_void_p, C.c_int, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
        _lib = l
    return _lib


# ---- the predicate ------------------------------------------------------------------------------------------------------------------
OK = dict(mode=0, ongrid=3, flags=1, cls=1, n_active=N, plan_flags=1, gains_finite=1, nseg=2, n1=100, N=N, step=1.0, step1=1.0, P0=5000.0, P1=40.0,
          duration=6000)


def pred(**kw):
    a = dict(OK); a.update(kw)
    return lib().zlwrap_predicate(a["mode"], a["ongrid"], a["flags"], a["cls"], a["n_active"], a["plan_flags"], a["gains_finite"], a["nseg"], a["n1"], a["N"],
                                  a["step"], a["step1"], a["P0"], a["P1"], a["duration"])


def test_predicate_each_condition_fails_alone():
    assert lib().zlwrap_sound_finite_flag() == 1
    assert pred() == 1
    assert pred(ongrid=1) == 0 and pred(ongrid=2) == 0 and pred(ongrid=0) == 0                    # the on-grid form, and this switch (ZL_K2_PAIR_WRAP)
    assert pred(mode=1) == 0 and pred(mode=4) == 0 and pred(mode=5) == 0 and pred(mode=2) == 1      # FIX_GAIN, Hermite; FIX_DELAY is the same mix
    assert pred(flags=0) == 0 and pred(flags=2) == 0                                                # ZL_SOUND_FINITE
    assert pred(cls=0) == 0 and pred(cls=3) == 0                                                    # idle; per-frame control
    assert pred(n_active=N - 1) == 0
    assert pred(plan_flags=1 | 4) == 0                                                              # ZL_PLAN_ENV
    assert pred(gains_finite=0) == 0
    assert pred(nseg=1) == 0 and pred(nseg=3) == 0
    assert pred(n1=0) == 0 and pred(n1=N) == 0 and pred(n1=INT_MAX) == 0 and pred(n1=-1) == 0
    assert pred(n1=1) == 1 and pred(n1=N - 1) == 1
    assert pred(step=np.nextafter(1.0, 2.0)) == 0 and pred(step=0.5) == 0 and pred(step1=np.nextafter(1.0, 0.0)) == 0 and pred(step1=2.0) == 0
    assert pred(P0=5000.5) == 0 and pred(P0=np.nextafter(5000.0, 0.0)) == 0 and pred(P1=40.25) == 0 and pred(P1=2.0 ** -30) == 0
    assert pred(P0=float(2 ** 30), duration=2 ** 31 - 1) == 0 and pred(P1=float(2 ** 30), duration=2 ** 31 - 1) == 0
    assert pred(P0=float(2 ** 30 - 200), duration=2 ** 31 - 1) == 1
    assert pred(P0=1e300) == 0 and pred(P1=1e300) == 0 and pred(P0=float("nan")) == 0 and pred(P1=float("nan")) == 0
    # every tap of both segments inside the source: the first segment's last frame is n1 - 1, the second's N - 1
    assert pred(P0=-1.0) == 0 and pred(P1=-1.0) == 0 and pred(P1=0.0) == 1 and pred(P0=0.0) == 1
    assert pred(P0=5900.0) == 1 and pred(P0=5901.0) == 0                                            # 5901 + 99 = the duration
    assert pred(P1=5844.0) == 1 and pred(P1=5845.0) == 0                                            # 5845 + 155 = the duration
    assert pred(P0=5999.0, n1=1) == 1 and pred(P0=6000.0, n1=1) == 0
    assert pred(P1=5999.0, n1=N - 1) == 1 and pred(P1=6000.0, n1=N - 1) == 0


# ---- the lane selection -------------------------------------------------------------------------------------------------------------
def block(stereo, src, length, P0, P1, n1):
    lohi = np.zeros(2, np.int32)
    bad = lib().zlwrap_block(stereo, length, src, P0, P1, n1, N, 0.7, 0.6, 0.9, 0.8, 0.25, 0.75, lohi)
    return bad, int(lohi[0]), int(lohi[1])


@pytest.mark.parametrize("stereo", [1, 0])
def test_every_n1_and_lane_against_the_definition(stereo):
    rng = np.random.default_rng(0x3C01 + stereo)
    ch = 2 if stereo else 1
    for n1 in range(1, N):
        for start in (0, 1, 6):                                       # P1 = 0 is frame 0 of the buffer
            loop = 700 + n1
            length = start + loop + 1                                # the loop ends one frame short of the source's last: interior
            src = np.zeros((length + 8) * ch, np.float32)            # (the arena keeps 8 frames of zeros behind a source)
            src[:length * ch] = rng.uniform(-1, 1, length * ch)
            src[:8:3] = -0.0; src[length * ch - 3] = 0.0
            P0, P1 = start + loop - n1, start
            assert pred(P0=float(P0), P1=float(P1), n1=n1, duration=length - 1) == 1
            bad, lo, hi = block(stereo, src, length, P0, P1, n1)
            assert bad == 0, (n1, start)
            assert 0 <= lo and hi <= length - 1, (n1, start, lo, hi)
            assert lo == min(P0, P1) and hi == (P0 + n1 if n1 & 1 else P0 + n1 - 1)      # a straddling lane's unused frame is P0 + n1
    # a single-segment voice of the same chunk (n1 = INT_MAX): the lane's own two frames
    bad, lo, hi = block(stereo, src, length, 17, 0, INT_MAX)
    assert bad == 0 and (lo, hi) == (17, 17 + N - 1)


def test_harness_as_a_sanitized_program(tmp_path):
    """pair_wrap_host.cpp with its own main, under AddressSanitizer and UBSan: sources in heap buffers of their exact size"""
    exe = str(tmp_path / "pair_wrap_asan")
    src = os.path.join(build.ROOT, "tests", "cpu_harness", "pair_wrap_host.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DZL_PAIR_WRAP_MAIN", "-ffp-contract=off",
           "-Wall", "-Wno-unused-function", "-I", build.CSRC, "-I", os.path.join(build.ROOT, "include"), "-o", exe, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "pair wrap: ok" in res.stdout, res.stdout + res.stderr


# ---- the scenes of the GPU tier, counted with the host planner --------------------------------------------------------------------------
def sim_lib():
    """the harness library as a SimSynth's library: it holds the planner itself (plan_host.cpp compiled into it), so the ZlSim that zlwrap_scan
    reads is made by the same shared object; the zlsim_* signatures are the ones tests/cpu_harness/sim.py declares"""
    from cpu_harness import sim
    l = lib()
    for name, fn in vars(sim.lib()).items():
        if name.startswith("zlsim_"):
            getattr(l, name).argtypes, getattr(l, name).restype = fn.argtypes, fn.restype
    return l


def scan(name):
    """per call: [K][V][6] of zlwrap_scan (class, n1, P0, P1, mono, source offset) -- the plans the host planner makes for the scene"""
    from cpu_harness.sim import SimSynth
    out = []

    class Scanning(SimSynth):
        def __init__(self, num_buses, voices_per_bus, *, mode=0, playback_sample_rate=48000.0, max_sounds=1024, voices_per_task=0, **kw):
            super().__init__(num_buses, voices_per_bus, mode=mode, playback_sample_rate=playback_sample_rate, max_sounds=max_sounds,
                             voices_per_task=voices_per_task, **kw)
            self.close()                                             # the same engine again, made by the harness library
            self.l = sim_lib()
            self.s = C.c_void_p(self.l.zlsim_create(num_buses, voices_per_bus, max_sounds, playback_sample_rate, mode, voices_per_task))

        def render_batch(self, nblocks, nframes, clocks, **kw):
            super().render_batch(nblocks, nframes, clocks, **kw)
            buf = np.zeros((nblocks, self.num_voices, 6), np.int32)
            assert lib().zlwrap_scan(self.s, 3, buf) == nblocks
            out.append(buf)

    sc = scenes.scene(name)
    _, _, syn, _ = run_backend(sc, Scanning, batch=scenes.calls(sc))
    syn.close()
    assert len(out) == 2                                             # two calls
    return sc, out


def chunks(sc, call):
    """(block, first voice, classes[8], rows[8]) of every chunk of 8 voices"""
    for k in range(call.shape[0]):
        for v0 in range(0, call.shape[1], 8):
            yield k, v0, call[k, v0:v0 + 8, 0], call[k, v0:v0 + 8]


def wrap_chunk(cls, rows):
    """chunk class 256: every voice on-grid in either form, one layout, a restart among them"""
    return bool((cls > 0).all() and (cls == 2).any() and len(set(rows[:, 4])) == 1)


_scans = {}


def scanned(name):
    if name not in _scans:
        _scans[name] = scan(name)
    return _scans[name]


def eligible(name):
    sc, cs = scanned(name)
    return [(c, k, v, cs[c][k, v]) for c in range(2) for k in range(cs[c].shape[0]) for v in range(cs[c].shape[1]) if cs[c][k, v, 0] == 2]


def test_every_scenes_launches_take_the_pair_kernels():
    """the launch table (zl_launch.h through tests/test_k2_launch_cpu.py's harness): with ZL_K2_PAIR=2 both calls of every scene go to
    zl_k2_pair_render in time order and to zl_k2_pair_phase_render in phase order, one bus per workgroup -- what is counted below is
    counted for launches that run the code under test"""
    import test_k2_launch_cpu as tl
    for name in scenes.SCENES:
        sc = scenes.scene(name)
        for order, kernel in ((False, tl.PAIR_RENDER), (True, tl.PAIR_PHASE_RENDER)):
            r = tl.launch(B=sc.num_buses, VPB=sc.voices_per_bus, K=scenes.calls(sc), N=sc.nframes, mode=sc.mode, want_pair=True, want_order=order)
            assert r["NB"] == 1 and r["kernel"] == kernel and r["threads"] == 128, (name, order, r)
    # (the shape the scenes must not have: two buses of eight voices are packed two to a workgroup and keep zl_k2_body's kernels)
    r = tl.launch(B=2, VPB=8, K=12, want_pair=True)
    assert r["NB"] == 2 and r["kernel"] == tl.RENDER


def test_every_scene_but_the_general_one_has_wrap_chunks_outside_the_last_block():
    for name in scenes.SCENES:
        sc, cs = scanned(name)
        n = sum(wrap_chunk(cls, rows) and k < call.shape[0] - 1 for call in cs for k, _, cls, rows in chunks(sc, call))
        assert (n == 0) if name == "mixed_and_pitched" else (n > 0), name


def test_listed_n1_values_odd_and_even_and_starts():
    el = eligible("n1_values")
    n1s = {int(r[1]) for _, _, _, r in el}
    assert {1, 2, 127, 128, 129, 254, 255} <= n1s
    # loop start 0 of the clip registered first in the arena; odd and even non-zero starts
    assert any(r[3] == 0 and r[5] == 0 for _, _, _, r in el)
    assert any(r[3] > 0 and r[3] % 2 == 1 for _, _, _, r in el) and any(r[3] > 0 and r[3] % 2 == 0 for _, _, _, r in el)
    # several voices restart in one block (block 4: seven of the chunk's eight)
    sc, cs = scanned("n1_values")
    assert max(int((cls == 2).sum()) for call in cs for _, _, cls, rows in chunks(sc, call) if wrap_chunk(cls, rows)) == 7
    assert all(r[4] == 0 for _, _, _, r in el)                        # stereo chunks


def test_mono_chunk_with_all_eight_restarting():
    sc, cs = scanned("mono_all_eight")
    full = [(k, rows) for call in cs for k, _, cls, rows in chunks(sc, call) if wrap_chunk(cls, rows) and (cls == 2).all()]
    assert full and all((rows[:, 4] == 1).all() for _, rows in full)
    el = eligible("mono_all_eight")
    assert any(r[3] == 0 and r[5] == 0 for _, _, _, r in el) and any(r[3] % 2 == 1 for _, _, _, r in el)
    assert any(r[1] % 2 == 1 for _, _, _, r in el) and any(r[1] % 2 == 0 for _, _, _, r in el)


def test_mixed_layout_and_pitched_chunks_stay_general():
    sc, cs = scanned("mixed_and_pitched")
    seen_mixed = seen_pitched = 0
    for call in cs:
        for k, v0, cls, rows in chunks(sc, call):
            assert not wrap_chunk(cls, rows)                         # neither chunk ever has the chunk class
            if v0 == 0 and (cls == 2).any():
                assert (cls > 0).all() and len(set(rows[:, 4])) == 2          # every voice on-grid, two layouts
                seen_mixed += 1
            if v0 == 8 and (cls == 2).any():
                assert cls[2] == 0                                   # the pitched voice is never on-grid
                seen_pitched += 1
    assert seen_mixed > 0 and seen_pitched > 0


def test_short_loops_and_loops_ending_at_the_last_frame_are_not_eligible():
    sc, cs = scanned("short_and_edge")
    assert all(call[:, 3, 0].max() == 0 for call in cs)              # a loop of 100 frames: no block of it is on-grid in either form
    edge = 8 + 6
    restarts = [(c, k) for c, call in enumerate(cs) for k in range(call.shape[0]) if call[k, edge, 1] < N and call[k, edge, 0] != 1]
    assert restarts and all(cs[c][k, edge, 0] == 0 for c, k in restarts)      # it restarts, and those blocks are not eligible
    assert any(call[:, edge, 0].max() == 1 for call in cs)           # (its other blocks are on-grid, one segment)
    assert any(v not in (3, edge) for _, _, v, _ in eligible("short_and_edge"))


def test_a_non_finite_source_is_never_on_grid_and_beat_locked_restarts_are():
    sc, cs = scanned("non_finite_and_beat")
    assert all(call[:, 1, 0].max() == 0 for call in cs)
    el = eligible("non_finite_and_beat")
    assert any(v in (0, 2, 3, 4, 5, 6, 7) for _, _, v, _ in el)
    assert any(v in (8, 9, 10) for _, _, v, _ in el)                  # restarted by the clock


def test_a_restart_in_each_calls_last_block():
    sc, cs = scanned("last_block")
    el = eligible("last_block")
    last = cs[0].shape[0] - 1
    assert any(c == 0 and k == last for c, k, _, _ in el) and any(c == 1 and k == last for c, k, _, _ in el)
    assert any(k < last for _, k, _, _ in el)


def test_adversarial_scene_has_stereo_and_mono_wrap_chunks():
    sc, cs = scanned("adversarial")
    kinds = {int(rows[0, 4]) for call in cs for k, _, cls, rows in chunks(sc, call) if wrap_chunk(cls, rows) and k < call.shape[0] - 1}
    assert kinds == {0, 1}
    assert {1, 2, 127, 128, 129, 254, 255} <= {int(r[1]) for _, _, _, r in eligible("adversarial")}
