"""K2's two-slot workgroups (ZL_K2_PAIR_LAPS; libzl_amd/csrc/zl_launch.h: zl_k2_launch with ZlK2In::pair_laps, zl_k2_pair_laps; zl_kernels.hip:
zl_k2_pair_fast2), CPU tier: the launch decision -- with the new input at its default every row of a sweep is the description the launch had
before, with 2 the grid is ceil(K / 2) exactly in a zl_k2_pair_phase_render launch and nothing else moves -- and, for every scene of
tests/test_k2_pair_laps.py, the number of workgroups that take the two-slot walk, counted from the host planner's records and the host order: a
GPU test cannot see which path ran, and a gate that never opens would pass it.  The harness is also built as a program of its own under
AddressSanitizer and UBSan and run here."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import k2_pair_laps_scenes as scenes
import test_k2_launch_cpu as tl
from libzl_amd import build
from scenario import run_backend

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_pair_laps_harness())
        ip = C.POINTER(C.c_int)
        l.zlpl_launch.argtypes = [ip, C.c_double, ip, C.c_int, ip]
        i32 = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
        l.zlpl_order.argtypes = [C.c_void_p, i32]
        u16 = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")
        l.zlpl_walks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u16, i32, i32, i32]
        l.zlpl_sort.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), i32]
        l.zlps_scan.argtypes = [C.c_void_p, C.c_int, np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS"), i32, i32, i32]
        _lib = l
    return _lib


OUT = tl.OUT + ("laps",)


def launch(pair_laps=0, loop=0.0, **kw):
    """tests/test_k2_launch_cpu.py's launch() with the new input (0: the member's default)"""
    a = dict(tl.BASE)
    vpb = kw.pop("VPB", 128)
    a.update(kw)
    if a["call_blocks"] is None:
        a["call_blocks"] = a["K"]
    if "NB" not in kw:
        a["NB"] = tl.lib().zllh_narrow_buses(a["call_blocks"], a["groups"], vpb, a["B"], a["N"])
    row = np.array([a[k] for k in tl.IN], dtype=np.int32)
    sw = np.array([tl.DEFAULT_SW[k] for k in tl.SW], dtype=np.int32)
    out = np.empty(len(OUT), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    lib().zlpl_launch(row.ctypes.data_as(ip), loop, sw.ctypes.data_as(ip), pair_laps, out.ctypes.data_as(ip))
    return {k: int(out[i]) for i, k in enumerate(OUT)}


def sweep():
    for K, N, B, VPB, mode, pm, om, tab, groups, staged in itertools.product((1, 2, 3, 47, 48, 375, 8191, 8192), (64, 128, 256, 512), (1, 8), (8, 128), (0, 1),
                                                                             (0, 2), (0, 2), (0, 1), (1, 2), (0, 1)):
        yield dict(K=K, N=N, B=B, VPB=VPB, mode=mode, pair_mode=pm, order_mode=om, order_table=tab, groups=groups, staged=staged)


def test_default_is_the_launch_as_it_was():
    """the member's default and an explicit 1: every row is what tests/test_k2_launch_cpu.py's harness (which does not know the field) answers"""
    n = 0
    for kw in sweep():
        old = tl.launch(**kw)
        for laps in (0, 1):
            new = launch(pair_laps=laps, **kw)
            assert new["laps"] == 1
            assert {k: new[k] for k in tl.OUT} == {k: old[k] for k in tl.OUT}, kw
        n += 1
    assert n > 1000


def test_two_slots_exactly_in_the_phase_order_pair_launch():
    n = two = 0
    for kw in sweep():
        old, new = launch(pair_laps=1, **kw), launch(pair_laps=2, **kw)
        want = old["kernel"] == tl.PAIR_PHASE_RENDER
        assert new["laps"] == (2 if want else 1), kw
        assert new["gy"] == ((kw["K"] + 1) // 2 if want else old["gy"]), kw
        assert {k: new[k] for k in tl.OUT if k != "gy"} == {k: old[k] for k in tl.OUT if k != "gy"}, kw
        n += 1; two += int(want)
    assert 0 < two < n


def test_known_answers():
    head = dict(order_mode=2, pair_mode=2)
    assert launch(pair_laps=2, K=8192, **head)["gy"] == 4096 and launch(pair_laps=2, K=8191, **head)["gy"] == 4096
    r = launch(pair_laps=2, K=8192, **head)
    assert r["kernel"] == tl.PAIR_PHASE_RENDER and r["laps"] == 2 and r["gz"] == 8 and r["threads"] == 128 and r["order"] == 1
    r = launch(pair_laps=2, K=1, call_blocks=1, **head)                 # one block: not a pair launch at all
    assert r["gy"] == 1 and r["laps"] == 1 and r["kernel"] == tl.RENDER
    assert launch(pair_laps=2, K=2, **head)["gy"] == 1 and launch(pair_laps=2, K=3, **head)["gy"] == 2 and launch(pair_laps=2, K=47, **head)["gy"] == 24
    # the time-order pair kernel and the one-frame kernels keep one block per workgroup
    assert launch(pair_laps=2, K=8192, pair_mode=2)["gy"] == 8192 and launch(pair_laps=2, K=8192, order_mode=2)["gy"] == 8192
    # the switch: 2 and above take two slots (the kernel is built for two), only where the window has the scalar records
    l = lib().zlpl_laps
    assert [l(sw, 1) for sw in (0, 1, 2, 3, 4)] == [1, 1, 2, 2, 2] and [l(sw, 0) for sw in (0, 1, 2, 4)] == [1, 1, 1, 1]


def test_harness_as_a_sanitized_program(tmp_path):
    """pair_laps_host.cpp with its own main, under AddressSanitizer and UBSan"""
    exe = str(tmp_path / "pair_laps_asan")
    src = os.path.join(build.ROOT, "tests", "cpu_harness", "pair_laps_host.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DZL_PAIR_LAPS_MAIN", "-ffp-contract=off",
           "-Wall", "-Wno-unused-function", "-I", build.CSRC, "-I", os.path.join(build.ROOT, "include"), "-o", exe, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "pair laps: ok" in res.stdout, res.stdout + res.stderr


# ---- the scenes of the GPU tier ---------------------------------------------------------------------------------------------------------------
def sim_lib():
    from cpu_harness import sim
    l = lib()
    for name, fn in vars(sim.lib()).items():
        if name.startswith("zlsim_"):
            getattr(l, name).argtypes, getattr(l, name).restype = fn.argtypes, fn.restype
    return l


def scan(name):
    """per call: (K, kind[K][B], run_end[B], order[B][K], walk[B][ceil(K / 2)], walks)"""
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
            V, B, K = self.num_voices, sc.num_buses, nblocks
            G = (V + 63) // 64
            bits, run_end = np.zeros((K, G), np.uint16), np.zeros(B, np.int32)
            kind, cl = np.zeros((K, B), np.int32), np.zeros((K, V), np.int32)
            assert lib().zlps_scan(self.s, 3, bits, run_end, kind, cl) == 0
            order, walk = np.zeros((B, K), np.int32), np.zeros((B, (K + 1) // 2), np.int32)
            lib().zlpl_order(self.s, order)
            # (a launch of one block is not a pair launch: no order, no records)
            walks = lib().zlpl_walks(K, B, sc.voices_per_bus, V, bits, run_end, order, walk) if K > 1 else 0
            out.append((K, kind, run_end, order, walk, walks))

    sc = scenes.scene(name)
    _, _, syn, _ = run_backend(sc, Scanning, batch=sc.call)
    syn.close()
    return sc, out


_scans = {}


def scanned(name):
    if name not in _scans:
        _scans[name] = scan(name)
    return _scans[name]


def test_every_scenes_launches_are_what_the_gpu_test_is_about():
    for name in scenes.SCENES:
        sc = scenes.scene(name)
        assert sc.call <= 48 and sc.nframes == 256
        r = launch(pair_laps=2, B=sc.num_buses, VPB=sc.voices_per_bus, K=sc.call, call_blocks=sc.call, N=sc.nframes, mode=sc.mode, order_mode=2, pair_mode=2)
        if sc.call == 1:
            assert r["kernel"] == tl.RENDER and r["laps"] == 1
        else:
            assert r["kernel"] == tl.PAIR_PHASE_RENDER and r["laps"] == 2 and r["gy"] == (sc.call + 1) // 2 and r["gz"] == sc.num_buses, (name, r)


@pytest.mark.parametrize("name", scenes.POSITIVE)
def test_positive_scenes_take_the_walk(name):
    sc, cs = scanned(name)
    assert sum(c[-1] for c in cs) > 0, name
    for K, kind, run_end, order, walk, walks in cs:
        for b in range(sc.num_buses):
            assert sorted(order[b]) == list(range(K))                # a bijection
            for w in np.nonzero(walk[b] == 2)[0]:
                kA, kB = order[b][2 * w], order[b][2 * w + 1]
                assert min(kA, kB) >= run_end[b] and max(kA, kB) != K - 1 and kind[kA, b] == kind[kB, b] != 0


@pytest.mark.parametrize("name", scenes.NEGATIVE)
def test_negative_scenes_do_not(name):
    sc, cs = scanned(name)
    assert sum(c[-1] for c in cs) == 0, name


def _mixed(cs, pred):
    """workgroups of two blocks that do not take the walk and whose blocks (kA, kB) satisfy pred(call, bus, kA, kB)"""
    n = 0
    for c in cs:
        K, kind, run_end, order, walk, walks = c
        for b in range(order.shape[0]):
            for w in range(K // 2):
                if walk[b][w] != 2:
                    n += int(pred(c, b, int(order[b][2 * w]), int(order[b][2 * w + 1])))
    return n


def test_the_mixed_workgroups_occur():
    """one block fast and one not (a restart); one block the call's last; one block in front of run_end and one behind it"""
    for name in ("bus_8", "bus_16", "restarts"):
        sc, cs = scanned(name)
        assert _mixed(cs, lambda c, b, kA, kB: (c[1][kA, b] != 0) != (c[1][kB, b] != 0)) > 0, name
        assert _mixed(cs, lambda c, b, kA, kB: max(kA, kB) == c[0] - 1) > 0, name
    for name in ("restarts", "two_buses_72", "edits"):               # (where run_end is odd in the order, or the key voice's buckets cut it)
        sc, cs = scanned(name)
        assert _mixed(cs, lambda c, b, kA, kB: (kA < c[2][b]) != (kB < c[2][b])) > 0, name
    # 47 blocks: the last workgroup holds one block
    sc, cs = scanned("blocks_47")
    assert all(c[0] == 47 and c[4].shape[1] == 24 and (c[4][:, 23] == 1).all() for c in cs)


def test_all_mono_is_the_mono_walk_and_two_layouts_stage():
    sc, cs = scanned("all_mono")
    assert {int(k) for c in cs for k in c[1].ravel()} == {0, 2}
    sc, cs = scanned("mono_and_stereo_chunks")
    assert all((c[1] == 0).all() for c in cs)


# ---- the order inside a phase bucket (zl_order.h: zl_order_sort_host, which K1o follows) -----------------------------------------------------------
SORT_MAX = 64
HEADLINE = 96000 - 64                                                # the headline's first key voice: loops of 96000 - 64 - v % 17 frames


def host_sort(M, K, t0=0, N=256):
    order, phase, bucket = np.zeros(K, np.int32), np.zeros(K, np.int64), np.zeros(K, np.int32)
    nbkt = lib().zlpl_sort(t0, M, N, K, order, phase, bucket)
    return nbkt, order, phase, bucket


@pytest.mark.parametrize("M", (100, 250, 257, 300, HEADLINE, HEADLINE - 9))     # loops shorter than a block, about one block, the headline's
@pytest.mark.parametrize("K", (1, 2, 3, 47, 48, 375, 8192))
def test_in_bucket_order(M, K):
    for t0 in (0, 5, -77):
        nbkt, order, phase, bucket = host_sort(M, K, t0)
        assert sorted(order.tolist()) == list(range(K))              # a bijection
        if nbkt == 0:                                                # the window is no longer than one pass: time order
            assert order.tolist() == list(range(K)) and K * 256 <= M
            continue
        b = bucket[order]
        assert (np.diff(b) >= 0).all()                               # buckets non-decreasing
        cuts = np.flatnonzero(np.diff(b)) + 1
        short = long_ = 0
        for seg in np.split(order, cuts):
            if len(seg) <= SORT_MAX:                                 # by exact phase, ties by block number
                keys = list(zip(phase[seg].tolist(), seg.tolist()))
                assert keys == sorted(keys), (M, K, t0)
                short += 1
            else:                                                    # longer buckets stay as the stable counting sort placed them: time order
                assert (np.diff(seg) > 0).all(), (M, K, t0)
                long_ += 1
        assert short + long_ == len(cuts) + 1
    if M < 300 and K == 8192:
        assert long_ > 0                                             # short loops: a few buckets hold the whole window
    if M >= HEADLINE - 9 and K == 8192:
        assert long_ == 0 and short == nbkt


def test_line_sharing_at_the_headline():
    """distinct 128-byte lines over lines requested by the two blocks of a workgroup, all voices of buses 0 and 1 of bench.py's scene (loops of
    96000 - 64 - v % 17 stereo frames from frame 0, 8192 blocks of 256 frames), under the host order of the bus's first voice.  A block with a loop
    restart of the voice counts as sharing nothing."""
    K, N = 8192, 256
    for bus in (0, 1):
        voices = range(128 * bus, 128 * bus + 128)
        L0 = 96000 - 64 - voices[0] % 17
        nbkt, order, phase, bucket = host_sort(L0, K)
        assert nbkt > 0
        kA, kB = order[0::2].astype(np.int64), order[1::2].astype(np.int64)
        distinct = requested = 0
        for v in voices:
            L = 96000 - 64 - v % 17
            pA, pB = (kA * N) % L, (kB * N) % L
            a0, a1, b0, b1 = pA * 8 // 128, ((pA + N) * 8 - 1) // 128, pB * 8 // 128, ((pB + N) * 8 - 1) // 128
            nA, nB = a1 - a0 + 1, b1 - b0 + 1
            both = np.maximum(0, np.minimum(a1, b1) - np.maximum(a0, b0) + 1)
            both[(pA + N > L) | (pB + N > L)] = 0
            distinct += int((nA + nB - both).sum()); requested += int((nA + nB).sum())
        assert distinct / requested <= 0.62, (bus, distinct / requested)
