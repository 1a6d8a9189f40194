"""The pair kernels' scalar records and fast workgroups (ZL_K2_PAIR_SCALAR; libzl_amd/csrc/zl_render.h: zl_voice_block_class, zl_pair_fast_bits,
zl_pair_group_need; zl_pair.h: zl_pair_scalar_window), CPU tier: the class K1c and the pair kernels' staging share against the text staging had
before, over the boundary values of every input; the 16 bits of a (block, group) and the mask of a bus's chunks; the host gate for bus widths;
and, with the host planner, the records of every scene of tests/test_k2_pair_scalar.py made the way K1c makes them, with the number of
workgroups that skip staging -- a GPU test cannot see which path ran, so the cases it is there for are shown to occur here.  The harness is
also built as a program of its own under AddressSanitizer and UBSan and run here."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import k2_pair_scalar_scenes as scenes
from libzl_amd import build
from scenario import run_backend

INT_MAX = 2 ** 31 - 1
N = 256
FIN = 1                                                              # ZL_SOUND_FINITE
_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_pair_scalar_harness())
        l.zlps_class.argtypes = [C.c_int, C.c_uint] + [C.c_int] * 6 + [C.c_float, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                                      C.c_float, C.c_float, C.c_float, C.c_int]
        l.zlps_fast_bits.argtypes = [C.c_ulonglong, C.c_ulonglong]; l.zlps_fast_bits.restype = C.c_uint
        l.zlps_group_need.argtypes = [C.c_int] * 3; l.zlps_group_need.restype = C.c_uint
        l.zlps_addr0.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_double, C.c_int]; l.zlps_addr0.restype = C.c_ulonglong
        l.zlps_tab_words.argtypes = [C.c_int, C.c_int]; l.zlps_tab_words.restype = C.c_ulonglong
        l.zlps_scan.argtypes = [C.c_void_p, C.c_int, np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")] \
            + [np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")] * 3
        _lib = l
    return _lib


# ---- the shared class ---------------------------------------------------------------------------------------------------------------------
OK = dict(mode=0, ongrid=1, trace=0, N=N, plan_flags=1, n_active=N, nseg=1, env=0.8, P0=743.0, step=1.0, n1=INT_MAX, P1=0.0, step1=0.0, channels=2,
          duration=999, lgain=0.7, rgain=0.6, vol=0.9, flags=FIN)
ORDER = ("mode", "ongrid", "trace", "N", "plan_flags", "n_active", "nseg", "env", "P0", "step", "n1", "P1", "step1", "channels", "duration", "lgain", "rgain", "vol", "flags")


def cls(which=0, **kw):
    a = dict(OK); a.update(kw)
    return lib().zlps_class(which, *[a[k] for k in ORDER])


def fast(**kw):
    return lib().zlps_voice_fast(cls(**kw)) == 1


def test_class_known_answers():
    # plays, simple, unit, interior, on-grid: 1 | 4 | 32 | 64 | 128; mono adds 16
    assert cls() == 1 | 4 | 32 | 64 | 128 and cls(channels=1) == 1 | 4 | 16 | 32 | 64 | 128
    assert fast() and fast(channels=1)
    # P0 + N - 1 at sample_duration - 1, at sample_duration and one over: interior needs the last position BELOW the duration
    assert fast(P0=743.0) and not fast(P0=744.0) and not fast(P0=745.0)
    assert cls(P0=744.0) == 1 | 4 | 32
    assert not fast(P0=17.5) and cls(P0=17.5) == 1 | 4 | 32 | 64              # not on the grid: the two-tap simple form
    for step in (np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 0.5):
        assert not fast(step=float(step)) and not cls(step=float(step)) & (32 | 128)
    assert not fast(nseg=2, n1=100) and cls(nseg=2, n1=100, P1=40.0, step1=1.0, ongrid=3) & 256     # a loop restart: class 256, not a fast voice-block
    assert not fast(plan_flags=1 | 4) and not fast(plan_flags=1 | 2) and not fast(plan_flags=0) and cls(plan_flags=0) == 0
    assert not fast(env=float("inf")) and not fast(env=float("nan")) and not fast(lgain=float("inf"))
    assert not fast(channels=3) and not fast(channels=0)
    assert not fast(n_active=N - 1) and not fast(trace=1) and not fast(flags=0) and not fast(ongrid=0)
    assert not fast(mode=1) and not fast(mode=4)
    # the duration at the limit of 32-bit byte offsets (0x1ffffff0 frames of 16 bytes are 2^33 bytes: such sources take the general path)
    assert fast(duration=0x1ffffff0 - 1) and not fast(duration=0x1ffffff0) and cls(duration=0x1ffffff0) == 1
    assert not fast(P0=float(2 ** 30), duration=INT_MAX)


def test_class_is_the_text_staging_had_over_every_boundary():
    P0s = (0.0, 17.0, 17.5, 743.0, 744.0, 745.0, float(2 ** 30), 1e300, -1.0, float("nan"))
    steps = (1.0, float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0)), 0.5)
    durs = (998, 999, 1000, 0x1ffffff0 - 1, 0x1ffffff0, INT_MAX)
    envs = (0.8, 0.0, float("inf"), float("nan"))
    n = nfast = 0
    for P0, step, dur, env, nseg, ch, pf, flags, ongrid, mode in itertools.product(P0s, steps, durs, envs, (1, 2, 3), (1, 2, 3), (0, 1, 3, 5), (FIN, 0), (0, 1, 3, 7), (0, 1, 4)):
        kw = dict(P0=P0, step=step, duration=dur, env=env, nseg=nseg, channels=ch, plan_flags=pf, flags=flags, ongrid=ongrid, mode=mode,
                  n1=100 if nseg == 2 else INT_MAX, P1=40.0, step1=1.0)
        a, b = cls(0, **kw), cls(1, **kw)
        assert a == b, kw
        n += 1; nfast += lib().zlps_voice_fast(a)
    assert 0 < nfast < n


def test_chunk_bits_and_bus_masks():
    l = lib()
    full = 2 ** 64 - 1
    assert l.zlps_fast_bits(full, 0) == 0x00ff and l.zlps_fast_bits(full, full) == 0xffff and l.zlps_fast_bits(0, 0) == 0
    for v in range(64):                                              # one voice not fast: its chunk's bit alone is clear
        assert l.zlps_fast_bits(full ^ (1 << v), 0) == 0xff ^ (1 << (v // 8))
        assert l.zlps_fast_bits(full, 1 << v) == 0xff ^ (1 << (v // 8))           # one mono voice among stereo ones: a mixed chunk is not fast
    assert l.zlps_fast_bits(full, 0xff << 16) == 0x00ff | (0x100 << 2)           # chunk 2 all mono: fast, and marked mono
    assert l.zlps_fast_bits(0xff, 0) == 1 and l.zlps_fast_bits(0xff << 56, 0xff << 56) == 0x8080
    # buses: 128 voices are groups 0 and 1 whole; 72 end inside a group; bus 1 of two buses of 72 begins at chunk 1 of group 1
    assert [l.zlps_group_need(0, 128, g) for g in range(3)] == [0xff, 0xff, 0]
    assert [l.zlps_group_need(0, 72, g) for g in range(3)] == [0xff, 0x01, 0]
    assert [l.zlps_group_need(72, 144, g) for g in range(4)] == [0, 0xfe, 0x03, 0]
    assert [l.zlps_group_need(8, 16, g) for g in range(2)] == [0x02, 0]
    # the address of frame 0: arena + 4 src_offset + 8 ipos (4 ipos mono), modulo 2^64 for a source in a grown segment below the first
    assert l.zlps_addr0(0x7f0000000000, 1024, 10.0, 0) == 0x7f0000000000 + 4096 + 80 and l.zlps_addr0(0x7f0000000000, 1024, 10.0, 1) == 0x7f0000000000 + 4096 + 40
    below = (2 ** 64 - 0x100000) // 4                                # src_offset of a segment 1 MiB BELOW the first one, in floats modulo 2^62
    assert l.zlps_addr0(0x7f0000000000, below, 3.0, 0) == 0x7f0000000000 - 0x100000 + 24
    # 8 bytes per (block, voice), 8 per voice, 2 per (block, 64 voices), rounded up to a word
    assert l.zlps_tab_words(8192, 1024) == 8192 * 1024 + 1024 + 8192 * 16 * 2 // 8 and l.zlps_tab_words(3, 72) == 3 * 72 + 72 + 2


def test_host_gate_for_bus_widths():
    g = lib().zlps_gate
    for vpb in (8, 16, 64, 72, 128, 1024):
        assert g(1, 1, 1, 1, vpb) == 1
    for vpb in (1, 4, 12, 60, 100, 127, 0):                           # not whole chunks of 8: some bus would begin or end inside a scalar load
        assert g(1, 1, 1, 1, vpb) == 0
    assert g(0, 1, 1, 1, 72) == 0                                    # ZL_K2_PAIR_SCALAR=0
    assert g(1, 0, 1, 1, 72) == 0 and g(1, 1, 0, 1, 72) == 0         # not a pair launch; time order (no run_end: zl_k2_pair_render stages)
    assert g(1, 1, 1, 0, 72) == 0                                    # no buffer (an engine in another mode)


def test_harness_as_a_sanitized_program(tmp_path):
    """pair_scalar_host.cpp with its own main, under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "pair_scalar_asan")
    src = os.path.join(build.ROOT, "tests", "cpu_harness", "pair_scalar_host.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DZL_PAIR_SCALAR_MAIN", "-ffp-contract=off",
           "-Wall", "-Wno-unused-function", "-I", build.CSRC, "-I", os.path.join(build.ROOT, "include"), "-o", exe, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "pair scalar: ok" in res.stdout, res.stdout + res.stderr


# ---- the scenes of the GPU tier, their records made with the host planner -------------------------------------------------------------------
def sim_lib():
    """the harness library as a SimSynth's library (it holds the planner itself: plan_host.cpp is compiled into it)"""
    from cpu_harness import sim
    l = lib()
    for name, fn in vars(sim.lib()).items():
        if name.startswith("zlsim_"):
            getattr(l, name).argtypes, getattr(l, name).restype = fn.argtypes, fn.restype
    return l


def scan(name):
    """per call: (bits[K][G], run_end[B], kind[K][B], cls[K][V]) of zlps_scan"""
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
            V, B = self.num_voices, sc.num_buses
            G = (V + 63) // 64
            bits, run_end = np.zeros((nblocks, G), np.uint16), np.zeros(B, np.int32)
            kind, cl = np.zeros((nblocks, B), np.int32), np.zeros((nblocks, V), np.int32)
            assert lib().zlps_scan(self.s, 3, bits, run_end, kind, cl) == 0     # K1c's bit is staging's class wherever a workgroup could be fast
            out.append((bits, run_end, kind, cl))

    sc = scenes.scene(name)
    _, _, syn, _ = run_backend(sc, Scanning, batch=sc.call)
    syn.close()
    return sc, out


_scans = {}


def scanned(name):
    if name not in _scans:
        _scans[name] = scan(name)
    return _scans[name]


def fast_workgroups(name):
    sc, cs = scanned(name)
    return [int((kind > 0).sum()) for _, _, kind, _ in cs]


def test_every_scenes_launches_take_the_phase_order_pair_kernel():
    """the launch table (zl_launch.h through tests/test_k2_launch_cpu.py's harness): with ZL_K2_PAIR=2 and ZL_K2_PHASE_ORDER=2 every call of every
    scene goes to zl_k2_pair_phase_render, one bus per workgroup, and the bus width passes the host gate"""
    import test_k2_launch_cpu as tl
    for name in scenes.SCENES:
        sc = scenes.scene(name)
        r = tl.launch(B=sc.num_buses, VPB=sc.voices_per_bus, K=sc.call, N=sc.nframes, mode=sc.mode, want_pair=True, want_order=True)
        assert r["NB"] == 1 and r["kernel"] == tl.PAIR_PHASE_RENDER and r["threads"] == 128, (name, r)
        assert lib().zlps_gate(1, 1, 1, 1, sc.voices_per_bus) == 1
        assert sc.call <= 96 and sc.nframes == 256 and 8 <= sc.voices_per_bus <= 128


# fast workgroups per call, counted once with this file's scan and held here: a change of the planner or of the scenes that loses them shows
EXPECTED = {"bus_8": [1, 2, 1], "bus_16": [4, 4, 3], "bus_128": [13, 18], "bus_72": [17, 20], "two_buses_72": [38, 49], "restarts": [10, 13],
            "all_mono": [13, 16], "grown_arena": [35, 47], "edits": [35, 37, 47, 0, 35]}      # (edits, fourth call: the bus is disabled, nothing plays)


@pytest.mark.parametrize("name", scenes.POSITIVE)
def test_positive_scenes_have_fast_workgroups(name):
    counts = fast_workgroups(name)
    sc, cs = scanned(name)
    assert sum(counts) > 0, (name, counts)
    for bits, run_end, kind, cl in cs:
        K = kind.shape[0]
        assert (kind[K - 1] == 0).all()                              # the call's last block: the report path stages
        for b in range(sc.num_buses):
            assert (kind[:run_end[b], b] == 0).all()                 # in front of run_end a record may be an inline run's: staged
    assert counts == EXPECTED[name], (name, counts)


@pytest.mark.parametrize("name", scenes.NEGATIVE)
def test_negative_scenes_have_none(name):
    """one voice of one chunk is not fast in any block behind run_end (or is idle / has ended): no workgroup of the bus skips staging, although
    the bus's other chunk is fast there"""
    sc, cs = scanned(name)
    assert sum(fast_workgroups(name)) == 0
    bad = scenes.OFFENDING_CHUNK.get(name, 0)
    other_fast = 0
    for bits, run_end, kind, cl in cs:
        K = kind.shape[0]
        # (while the one-shot plays in sustain its blocks are an inline run: they lie in front of run_end, where nobody is fast)
        assert not ((bits[run_end[0]:, 0] >> bad) & 1).any(), name
        other_fast += int(((bits[run_end[0]:K - 1, 0] >> (1 - bad)) & 1).sum())
    assert other_fast > 0, name
    if name == "neg_oneshot":
        cl = cs[0][3]                                                # it plays behind run_end and ends inside the first call's window (dead_from < K)
        assert (cl[cs[0][1][0], 3] & 1) and not (cl[-1, 3] & 1) and not cs[1][3][:, 3].any()


def test_both_sides_of_run_end_within_one_call():
    for name in ("bus_8", "bus_16"):
        sc, cs = scanned(name)
        bits, run_end, kind, cl = cs[0]
        assert 0 < run_end[0] < kind.shape[0] - 1 and (kind[run_end[0]:] > 0).any(), (name, run_end)
        for bits, run_end, kind, cl in cs[1:]:
            assert run_end[0] == 0 and (kind > 0).any()              # from the second call on no voice has an inline run


def test_wide_buses_span_k1c_waves():
    sc, cs = scanned("bus_128")
    assert any(((bits[:, 0] & 0xff) == 0xff).any() and ((bits[:, 1] & 0xff) == 0xff).any() for bits, _, _, _ in cs)
    # a block in which one group is fast throughout and the other is not: the workgroup stages
    assert any((((bits[:, 0] & 0xff) == 0xff) != ((bits[:, 1] & 0xff) == 0xff)).any() for bits, _, _, _ in cs)
    sc, cs = scanned("bus_72")
    assert all(((bits[:, 1] & 0xfe) == 0).all() for bits, _, _, _ in cs)       # group 1 holds one chunk of the bus, the rest of the wave has no voice
    sc, cs = scanned("two_buses_72")
    per_bus = np.sum([(kind > 0).sum(axis=0) for _, _, kind, _ in cs], axis=0)
    assert (per_bus > 0).all(), per_bus                              # bus 1 (voices 72..143: group 1 from chunk 1, group 2 to chunk 1) has fast workgroups too
    assert any(((kind[:, 0] > 0) != (kind[:, 1] > 0)).any() for _, _, kind, _ in cs)          # and not in the same blocks as bus 0


def test_restarts_stage_and_their_neighbours_do_not():
    sc, cs = scanned("restarts")
    seen = 0
    for bits, run_end, kind, cl in cs:
        K = kind.shape[0]
        restart = ((cl[:, :8] & (256 | 8 | 2)) != 0).any(axis=1)       # a second segment in the block, in whatever form it is rendered
        assert (kind[restart, 0] == 0).all()
        assert (kind[int(run_end[0]):K - 1, 0][~restart[int(run_end[0]):K - 1]] == 1).all()      # every other block behind run_end is fast
        for k in range(int(run_end[0]) + 1, K - 2):                  # the blocks right before and right after a restart
            seen += int(restart[k] and kind[k - 1, 0] == 1 and kind[k + 1, 0] == 1)
    assert seen > 0
    # voice 1's loop (1024 frames from frame 0) ends on a block's last frame: one segment in every block
    assert all(((cl[run_end[0]:, 1] & (256 | 8)) == 0).all() for _, run_end, _, cl in cs)


def test_all_mono_bus_is_the_mono_kind():
    sc, cs = scanned("all_mono")
    kinds = {int(k) for _, _, kind, _ in cs for k in kind.ravel()}
    assert kinds == {0, 2}
