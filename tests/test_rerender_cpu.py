"""Clip re-render, CPU tier: the host build of libzl_amd/csrc/zl_stretch.h (the text the HIP kernels run) against the independent numpy
restatement (tests/stretch_ref.py) bit for bit -- data and seek offsets -- over the parameter grid; properties of the restatement;
the new C-ABI struct; the new kernels' resources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stretch_ref as sr_
from rerender_cases import GAINS, PITCHES, RATES, SPEEDS, cases, lengths, same_bits, source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(built):
    lib = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "_build", "libzl_stretch_host.so"))
    lib.zlst_geometry.argtypes = [C.c_double, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.zlst_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def host_render(lib, src, sr, gain, pitch, speed):
    ch, n = src.shape
    geo = np.zeros(9, np.int64)
    assert lib.zlst_geometry(sr, n, gain, pitch, speed, geo.ctypes.data) == 0
    N, nseg = int(geo[0]), int(geo[2])
    ident = gain == 0 and pitch == 0 and speed == 1
    out = np.zeros((ch, n if ident else N), f32)
    offs = np.zeros(max(nseg, 1), np.int32)
    L = np.ascontiguousarray(src[0]); R = np.ascontiguousarray(src[1]) if ch == 2 else None
    assert lib.zlst_render(L.ctypes.data, None if R is None else R.ctypes.data, n, sr, gain, pitch, speed,
                           out[0].ctypes.data, out[1].ctypes.data if ch == 2 else None, offs.ctypes.data) == 0
    return out, offs[:nseg]


def test_geometry_matches_the_restatement(host):
    for sr in RATES:
        for speed in SPEEDS:
            for pitch in PITCHES:
                for n in lengths(sr, speed, pitch):
                    geo = np.zeros(9, np.int64)
                    assert host.zlst_geometry(sr, n, 0.0, pitch, speed, geo.ctypes.data) == 0
                    g = sr_.geometry(sr, n, 0.0, pitch, speed)
                    assert list(geo[:6]) == [g["N"], g["N1"], g["nseg"], g["O"], g["S"], g["W"]], (sr, speed, pitch, n)
                    assert list(geo[6:8]) == [int(g["stretch"]), int(g["resample"])]
    geo = np.zeros(9, np.int64)
    for bad in ((0.0, 0.0, 0.2), (0.0, 0.0, 4.5), (0.0, 24.5, 1.0), (0.0, -25.0, 1.0), (float("inf"), 0.0, 1.0), (float("nan"), 0.0, 1.0), (0.0, float("nan"), 1.0)):
        assert host.zlst_geometry(48000.0, 1000, *bad, geo.ctypes.data) == -1, bad


GRID = cases()


@pytest.mark.parametrize("sr,ch,speed,pitch,gain,length", GRID, ids=[f"{int(c[0])}-{c[1]}ch-s{c[2]}-p{c[3]}-g{c[4]}-n{c[5]}" for c in GRID])
def test_host_build_equals_the_restatement(host, sr, ch, speed, pitch, gain, length):
    src = source(sr, ch, length, seed=length + 7 * ch)
    ref, roffs = sr_.render(src, sr, gain, pitch, speed)
    out, offs = host_render(host, src, sr, gain, pitch, speed)
    assert same_bits(out, ref), np.flatnonzero((out != ref).any(axis=0))[:10]
    assert np.array_equal(offs.astype(np.int64), roffs)


@pytest.mark.parametrize("kind", ["zeros", "special"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("speed,pitch,gain", [(1.25, 3.0, -6.0), (0.5, -12.0, 0.0), (2.0, 7.0, 3.0), (1.0, -5.0, 0.0), (0.8, 0.0, 3.0)])
def test_all_zero_and_special_values(host, kind, ch, speed, pitch, gain):
    sr = 48000.0
    src = source(sr, ch, 24000, seed=5, kind=kind)
    ref, roffs = sr_.render(src, sr, gain, pitch, speed)
    out, offs = host_render(host, src, sr, gain, pitch, speed)
    assert same_bits(out, ref)
    assert np.array_equal(offs.astype(np.int64), roffs)
    if kind == "zeros":
        assert not offs.any() and not out.any()              # every tie resolves to offset 0
    else:
        assert np.isnan(out).any()


# ---- properties of the restatement ------------------------------------------------------------------------------------------

def test_output_length_follows_the_formula():
    for sr in RATES:
        for speed in SPEEDS:
            for pitch in (-12.0, 0.0, 7.0):
                for n in (1, 37, 5000):
                    y, _ = sr_.render(source(sr, 1, n, 1), sr, 0.0, pitch, speed)
                    expect = n if (speed == 1 and pitch == 0) else max(1, int(np.floor(n / np.float64(np.float32(speed)))))
                    assert y.shape == (1, expect), (sr, speed, pitch, n)


def test_identity_returns_the_original_exactly():
    src = source(44100.0, 2, 10000, 3, kind="special")
    y, offs = sr_.render(src, 44100.0, 0.0, 0.0, 1.0)
    assert same_bits(y, src) and offs.size == 0


def _peak_hz(y, sr):
    spec = np.abs(np.fft.rfft(y.astype(np.float64) * np.hanning(len(y))))
    return np.argmax(spec) * sr / len(y), sr / len(y)


def test_pitch_and_speed_move_the_spectrum_as_expected():
    sr = 48000.0
    n = int(2 * sr)
    sine = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)).astype(f32)[None, :]
    y, _ = sr_.render(sine, sr, 0.0, 12.0, 1.0)
    hz, bin_ = _peak_hz(y[0], sr)
    assert abs(hz - 880.0) <= bin_, hz
    y, _ = sr_.render(sine, sr, 0.0, 0.0, 2.0)
    assert y.shape[1] == n // 2
    hz, bin_ = _peak_hz(y[0], sr)
    assert abs(hz - 440.0) <= bin_, hz


def test_gain_scales_by_exactly_g():
    src = source(48000.0, 2, 5000, 9)
    y, _ = sr_.render(src, 48000.0, -6.0, 0.0, 1.0)
    g = np.float32(10.0 ** (-6.0 / 20.0))
    assert same_bits(y, src * g)


# ---- C-ABI and kernels ------------------------------------------------------------------------------------------------------

def test_rerender_params_struct_layout(tmp_path):
    from libzl_amd import _abi
    prog = tmp_path / "p.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){printf("%d %d %d %d %d\\n",(int)sizeof(zlhip_rerender_params),'
                    '(int)offsetof(zlhip_rerender_params,gain_db),(int)offsetof(zlhip_rerender_params,pitch_semitones),'
                    '(int)offsetof(zlhip_rerender_params,speed_ratio),(int)offsetof(zlhip_rerender_params,reserved));return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _abi.RerenderParams
    assert got == [C.sizeof(P), P.gain_db.offset, P.pitch_semitones.offset, P.speed_ratio.offset, P.reserved.offset] == [16, 0, 4, 8, 12]


def test_rerender_kernels_have_no_scratch_memory(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_stretch_kernel_resources.txt")
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    seek = [r for n, r in rows.items() if "zl_k_stretch_seek" in n]
    synth = [r for n, r in rows.items() if "zl_k_stretch_synth" in n]
    assert len(seek) == 1 and len(synth) == 1, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    assert not any("zl_k2_render" in n or "zl_k_rt_loop" in n for n in rows)
