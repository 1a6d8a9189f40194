"""The per-slot run summary behind K2's order table (libzl_amd/csrc/zl_order.h), CPU tier: run_end per z-slot, the dense dead_from per
voice, and the indices of both, built for the host from hand-made run lists.

K1o (zl_kernels.hip) writes the same words with the same functions; the pair kernel's staging leaves the run-list loads out in the
blocks at or behind run_end (tests/test_k2_stage_norun.py holds the parity on the GPU).  The harness is also built as a program of
its own under AddressSanitizer and UBSan and run here.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libzl_amd import build

INT_MAX = 2 ** 31 - 1
MAXRUNS = 6
_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_order_summary_harness())
        ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
        l.zlsum_build.argtypes = [C.c_int] * 6 + [ip] * 4
        for f in (l.zlsum_ints, l.zlsum_run_end_index, l.zlsum_dead_index):
            f.argtypes = [C.c_int] * 3
        _lib = l
    return _lib


def summary(voices, VPB, NB, nslots, K, on=1):
    """voices: list of (dead_from, [(k0, k1), ...] inline runs, optional stale entries behind n).  Returns (run_end[nslots], dead[V])."""
    V = len(voices)
    n = np.zeros(V, np.int32)
    dead = np.zeros(V, np.int32)
    kk = np.zeros((V, MAXRUNS, 2), np.int32)
    for v, vo in enumerate(voices):
        dead[v], runs = vo[0], vo[1]
        n[v] = len(runs)
        for j, r in enumerate(list(runs) + (list(vo[2]) if len(vo) > 2 else [])):
            kk[v, j] = r
    ints = lib().zlsum_ints(nslots, K, V)
    assert ints == nslots * K + nslots + V
    buf = np.full(ints, -7, np.int32)
    assert lib().zlsum_build(V, VPB, NB, nslots, K, on, n, dead, kk.reshape(-1), buf) == ints
    assert (buf[:nslots * K] == -7).all()                          # the order table is not the summary's to write
    assert (buf[nslots * K:] != -7).all()                          # every word of the tail is
    assert [lib().zlsum_run_end_index(nslots, K, z) for z in range(nslots)] == list(range(nslots * K, nslots * K + nslots))
    assert [lib().zlsum_dead_index(nslots, K, v) for v in range(V)] == list(range(nslots * K + nslots, ints))
    return buf[nslots * K:nslots * K + nslots].copy(), buf[nslots * K + nslots:].copy()


K = 96


def test_no_voice_has_a_run():
    run_end, dead = summary([(K, [])] * 8, 4, 1, 2, K)
    assert list(run_end) == [0, 0] and (dead == K).all()


def test_one_voice_with_two_runs_gives_its_last_k1():
    voices = [(K, [])] * 8
    voices[5] = (K, [(0, 30), (31, 61)], [(70, 95)])               # (an entry behind n is stale: it does not count)
    run_end, dead = summary(voices, 4, 1, 2, K)
    assert list(run_end) == [0, 61]
    # runs need not be sorted by k1 for the maximum to hold
    voices[1] = (K, [(50, 80), (0, 40)])
    voices[2] = (K, [(0, 12)])
    run_end, dead = summary(voices, 4, 1, 2, K)
    assert list(run_end) == [80, 61]


def test_an_idle_voice_and_a_voice_that_ends_mid_window():
    voices = [(K, []), (0, []), (41, []), (K, []), (K, []), (17, [(0, 17)]), (K, []), (K, [])]
    run_end, dead = summary(voices, 4, 1, 2, K)
    assert list(run_end) == [0, 17]
    assert list(dead) == [K, 0, 41, K, K, 17, K, K]


def test_the_last_slot_is_partial():
    # 10 voices in slots of 4: slot 2 holds voices 8 and 9 (ve clipped to V)
    voices = [(K, [])] * 10
    voices[9] = (K - 1, [(10 * j, 10 * j + 9) for j in range(MAXRUNS)])
    voices[3] = (K, [(2, 5)])
    run_end, dead = summary(voices, 4, 1, 3, K)
    assert list(run_end) == [5, 0, 59] and dead[9] == K - 1 and dead[8] == K
    # narrow buses: 2 buses of 4 voices per slot, the last slot holds one bus of two voices
    run_end, dead = summary(voices, 4, 2, 2, K)
    assert list(run_end) == [5, 59] and dead[9] == K - 1


def test_the_switch_off_gives_int_max():
    voices = [(K, [(0, 30)]), (0, []), (41, []), (K, [])]
    run_end, dead = summary(voices, 2, 1, 2, K, on=0)
    assert list(run_end) == [INT_MAX, INT_MAX]
    assert list(dead) == [K, 0, 41, K]                             # dead_from is written either way


def test_harness_as_a_sanitized_program(tmp_path):
    """order_summary_host.cpp with its own main, under AddressSanitizer and UBSan: the same cases, run as a program of its own"""
    exe = str(tmp_path / "order_summary_asan")
    src = os.path.join(build.ROOT, "tests", "cpu_harness", "order_summary_host.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DZL_ORDER_SUMMARY_MAIN",
           "-Wall", "-Wno-unused-function", "-I", build.CSRC, "-I", os.path.join(build.ROOT, "include"), "-o", exe, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and "order summary: ok" in res.stdout, res.stdout + res.stderr
