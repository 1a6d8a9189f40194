"""K2's phase order (libzl_amd/csrc/zl_order.h), CPU tier: the keys, the key voice, the sort and the gate, built for the host.

The device kernel (K1o) runs the same key and bucket code; tests/test_k2_phase_order.py holds its parity on the GPU.
"""
import ctypes as C
import math

import numpy as np
import pytest

from libzl_amd import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_order_harness())
        ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
        fp = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
        l.zlord_build.restype = C.c_int
        l.zlord_build.argtypes = [C.c_int] * 6 + [ip] * 7
        l.zlord_shape.argtypes = [C.c_int] * 4
        l.zlord_window.argtypes = [C.c_int] * 5 + [C.c_double]
        l.zlord_loop_frames.restype = C.c_double
        l.zlord_loop_frames.argtypes = [C.c_int, C.c_double, ip, ip, ip, fp]
        _lib = l
    return _lib


def build_order(runs, VPB, NB, nslots, K, N):
    """runs: list of (per_t0, per_M, per_n, dead_from) per voice."""
    V = len(runs)
    cols = [np.ascontiguousarray([r[i] for r in runs], dtype=np.int32) for i in range(4)]
    order = np.zeros(nslots * K, np.int32)
    bucket = np.zeros(nslots * K, np.int32)
    keyv = np.zeros(nslots, np.int32)
    n = lib().zlord_build(V, VPB, NB, nslots, K, N, *cols, order, bucket, keyv)
    return n, order.reshape(nslots, K), bucket.reshape(nslots, K), keyv


def check_bijection(order, K):
    for row in order:
        assert np.array_equal(np.sort(row), np.arange(K, dtype=np.int32))


@pytest.mark.parametrize("K", [1, 2, 3, 7, 255, 256, 257, 375, 1000, 2048, 8192, 20000, 60000])
def test_bijection_and_sorted_keys_wide_buses(K):
    # 8 buses x 4 voices, 256-frame blocks, headline-like 2 s loops (per_M differs per voice by the bench's v % 17), the pass
    # starting at various offsets (negative: a cached pass shifted back)
    N, B, VPB = 256, 8, 4
    runs = [(-(v * 977) % 5000 - 100 * (v % 3), 96000 - 64 - (v % 17), 3, K) for v in range(B * VPB)]
    n, order, bucket, keyv = build_order(runs, VPB, 1, B, K, N)
    check_bijection(order, K)
    assert n == (B if K * N > 96000 - 64 else 0)
    for z in range(B):
        if keyv[z] >= 0 and K * N > runs[keyv[z]][1]:
            assert (np.diff(bucket[z]) >= 0).all()                 # keys come out non-decreasing
        else:
            assert np.array_equal(order[z], np.arange(K))


@pytest.mark.parametrize("K", list(range(1, 70)) + [511, 4097, 59999, 60000])
def test_bijection_every_small_K_short_loops(K):
    # loops far shorter than a block and around one block: many passes per window, buckets of one block's frames
    N = 256
    for M in (1, 100, 255, 256, 257, 300, 1000, 3 * 256 + 1):
        runs = [(17, M, 1, K), (0, M + 5, 1, K)]
        n, order, bucket, keyv = build_order(runs, 2, 1, 1, K, N)
        check_bijection(order, K)
        assert keyv[0] == 0
        if K * N > M:
            assert n == 1 and (np.diff(bucket[0]) >= 0).all()
            assert bucket[0].max() < math.ceil(M / N)


def test_bijection_all_K_up_to_60000_one_layout():
    # every K from 1 to 60000 for one layout (a periodic key voice, 256-frame blocks, a 2 s loop)
    N = 256
    lib_ = lib()
    per = [np.array([v], np.int32) for v in (-1234, 96000 - 70, 2, 0)]
    order = np.zeros(60000, np.int32)
    bucket = np.zeros(60000, np.int32)
    keyv = np.zeros(1, np.int32)
    for K in range(1, 60001):
        per[3][0] = K
        lib_.zlord_build(1, 1, 1, 1, K, N, *per, order, bucket, keyv)
        o = order[:K]
        seen = np.zeros(K, bool)
        seen[o] = True
        assert seen.all(), K
        if K * N > 96000 - 70:
            assert (np.diff(bucket[:K]) >= 0).all(), K


def test_narrow_buses_one_slot_and_partial_last_slot():
    # narrow buses: 16 buses x 8 voices, 16 buses per workgroup (one z-slot), then 12 buses of 8 with NB = 5 (last slot holds 2 buses)
    N, K = 256, 3000
    runs = [(0, 0, 0, K)] * 3 + [(40, 7000, 2, K)] + [(0, 9000, 1, K)] * 124
    n, order, bucket, keyv = build_order(runs, 8, 16, 1, K, N)
    check_bijection(order, K)
    assert keyv[0] == 3 and n == 1 and (np.diff(bucket[0]) >= 0).all()
    runs2 = [(0, 5000 + 3 * v, 1, K) for v in range(96)]
    n, order, bucket, keyv = build_order(runs2, 8, 5, 3, K, N)
    check_bijection(order, K)
    assert list(keyv) == [0, 40, 80] and n == 3


def test_key_voice_skips_voices_that_stop_or_do_not_loop():
    N, K = 256, 400
    runs = [(0, 5000, 0, K),         # no periodic part
            (0, 5000, 2, K - 1),     # stops inside the window
            (0, 0, 2, K),            # no pass length
            (10, 6000, 1, K)]        # the key
    n, order, bucket, keyv = build_order(runs, 4, 1, 1, K, N)
    assert keyv[0] == 3 and n == 1
    # no key voice at all: time order
    n, order, bucket, keyv = build_order(runs[:3], 3, 1, 1, K, N)
    assert keyv[0] == -1 and n == 0 and np.array_equal(order[0], np.arange(K))


def test_identity_when_window_not_longer_than_a_pass():
    N = 256
    for K, M in ((100, 100 * 256), (100, 100 * 256 + 1), (10, 96000), (375, 96000)):
        n, order, bucket, keyv = build_order([(5, M, 1, K)], 1, 1, 1, K, N)
        assert n == 0 and np.array_equal(order[0], np.arange(K))
    n, order, bucket, keyv = build_order([(5, 100 * 256 - 1, 1, 101)], 1, 1, 1, 101, N)
    assert n == 1


def test_long_pass_buckets_coarsen_to_the_lds_histogram():
    # a pass of 10 000 blocks: buckets of several blocks, at most ZL_ORDER_MAXBKT of them
    N, K = 256, 60000
    n, order, bucket, keyv = build_order([(0, 10000 * 256 + 3, 1, K)], 1, 1, 1, K, N)
    check_bijection(order, K)
    assert n == 1 and bucket.max() < 2048 and (np.diff(bucket[0]) >= 0).all()


def test_repeats_of_one_phase_are_neighbours():
    # the headline shape: 8192 blocks, 2 s loops -- each bucket holds the ~22 repeats of one phase, one per pass
    N, K, M = 256, 8192, 96000 - 64
    n, order, bucket, keyv = build_order([(0, M, 1, K)], 1, 1, 1, K, N)
    counts = np.bincount(bucket[0])
    assert counts[:-1].min() >= 21 and counts.max() <= 22        # (the last bucket is narrower than a block: some passes step over it)
    phase = (order[0].astype(np.int64) * N) % M
    for b in range(counts.size):
        p = phase[bucket[0] == b]
        assert p.max() - p.min() < N


def test_shape_gate():
    s = lib().zlord_shape
    assert s(1, 0, 8192, 256) == 1 and s(1, 0, 2, 512) == 1 and s(1, 0, 100, 100) == 1
    assert s(2, 0, 8192, 256) == 0            # mix groups
    assert s(1, 1, 8192, 256) == 0            # LDS-staged
    assert s(1, 0, 1, 256) == 0               # a single real-time block
    assert s(1, 0, 8192, 128) == 0 and s(1, 0, 8192, 64) == 0   # two / four blocks per workgroup


def test_window_gate():
    w = lib().zlord_window
    inf = float("inf")
    assert w(1, 1, 0, 256, 8192, 96000.0) == 1
    assert w(1, 1, 0, 256, 2048, 576000.0) == 0          # the HBM-only leg: 12 s loops, 2048-block windows
    assert w(1, 1, 0, 256, 8192, inf) == 0               # a voice that is not cheap to plan, or nothing loops
    assert w(1, 1, 1, 256, 8192, 96000.0) == 0           # bounce
    assert w(1, 1, 0, 128, 8192, 96000.0) == 0 and w(1, 1, 0, 200, 8192, 96000.0) == 0
    assert w(1, 0, 0, 256, 8192, 96000.0) == 0
    assert w(0, 1, 0, 256, 8192, 96000.0) == 0
    assert w(2, 1, 1, 100, 3, inf) == 1 and w(2, 0, 0, 256, 8192, 96000.0) == 0


def test_loop_frames_from_host_voice_state():
    f = lib().zlord_loop_frames

    def run(playing, cheap, looping, secs, fs=48000.0):
        a = lambda x: np.ascontiguousarray(x, dtype=np.int32)
        return f(len(playing), fs, a(playing), a(cheap), a(looping), np.ascontiguousarray(secs, dtype=np.float32))

    assert run([1, 1, 1], [1, 1, 1], [1, 1, 1], [2.0, 1.5, 3.0]) == pytest.approx(72000.0)
    assert run([1, 0, 1], [1, 0, 1], [1, 1, 1], [2.0, 0.1, 3.0]) == pytest.approx(96000.0)   # idle voices do not count ...
    assert math.isinf(run([1, 1, 1], [1, 0, 1], [1, 1, 1], [2.0, 1.5, 3.0]))                # ... a pitched one vetoes
    assert math.isinf(run([1, 1], [1, 1], [0, 0], [2.0, 1.5]))                              # nothing loops
    assert run([1, 1], [1, 1], [0, 1], [0.5, 1.0], fs=96000.0) == pytest.approx(96000.0)    # one-shots do not count
