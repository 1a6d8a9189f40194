"""Clip re-render, CPU tier: the host build of libzl_amd/csrc/zl_stretch.h (the text the HIP kernels run) against the independent numpy
restatement (tests/stretch_ref.py) bit for bit -- data and seek offsets -- over the parameter grid; properties of the restatement;
the new C-ABI struct; the new kernels' resources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stretch_ref as sr_
from rerender_cases import (GAINS, LAST_FRAME_CASES, PITCHES, RATES, SPEEDS, TIE_SPEED, cases, edge_cases, edge_id, holds_ties,
                            last_frame_source, lengths, same_bits, source, tie_cases, tie_source)

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


def test_geometry_limits(host):
    """what the stretch accepts and rejects at the ends of the sample-rate range, host build and restatement alike: the seek window
    W + O may be 4608 frames and no more, the sequence must be longer than the overlap, and neither matters where the stretch
    does not run (tau == 1)"""
    def both(sr, speed, pitch):
        geo = np.zeros(9, np.int64)
        rc = host.zlst_geometry(sr, 1000, 0.0, pitch, speed, geo.ctypes.data)
        try:
            g = sr_.geometry(sr, 1000, 0.0, pitch, speed)
        except ValueError:
            assert rc == -1, (sr, speed, pitch)
            return None
        assert rc == 0, (sr, speed, pitch)
        assert list(geo[:8]) == [g["N"], g["N1"], g["nseg"], g["O"], g["S"], g["W"], int(g["stretch"]), int(g["resample"])]
        return g

    g = both(204800.0, 0.5, 0.0)
    assert g is not None and (g["W"], g["O"]) == (4096, 512) and g["W"] + g["O"] == sr_.MAX_WINDOW == 4608
    assert both(204850.0, 0.5, 0.0) is None                        # W = 4097
    assert int(np.floor(204850.0 * 20.0 / 1000.0)) == 4097
    g = both(204850.0, 2.0, 12.0)                                  # tau == 1: the stretch does not run
    assert g is not None and not g["stretch"] and g["nseg"] == 0 and g["resample"]
    g = both(204850.0, 2.0, 0.0)
    assert g is not None and g["stretch"] and g["W"] == 3072
    assert both(400.0, 4.0, 0.0) is None                           # S = 16 = O
    assert int(np.floor(400.0 * 40.0 / 1000.0)) == 16
    g = both(425.0, 4.0, 0.0)
    assert g is not None and (g["S"], g["O"], g["W"]) == (17, 16, 6)
    assert both(400.0, 4.0, 24.0) is not None                      # (tau == 1 again, at the low end)


def test_the_edge_cases_hold_the_geometries_they_are_there_for():
    """so that the list does not decay: from the restatement's geometry alone"""
    seen = {}
    for (sr, ch, speed, pitch, gain, length, kind) in EDGE:
        g = sr_.geometry(sr, length, gain, pitch, speed)
        seen.setdefault((sr, speed, pitch), []).append((g, length, ch, kind))
    assert all(sorted(c for _, _, c, _ in v) in ([1, 2], [1, 1, 1, 1, 2, 2, 2, 2]) for v in seen.values())    # mono and stereo each
    geo = {k: v[0][0] for k, v in seen.items()}
    g = geo[(425.0, 4.0, 0.0)]
    assert (g["O"], g["S"] - g["O"], g["W"]) == (16, 1, 6) and g["nseg"] > 4
    g = geo[(500.0, 0.5, 0.0)]
    assert g["O"] == 16 and g["S"] - g["O"] > g["O"] and g["W"] == 10 and g["nseg"] > 4
    assert geo[(2000.0, 2.0, 7.0)]["W"] == 34 and geo[(8000.0, 0.5, 0.0)]["W"] == 160
    assert geo[(47250.0, 1.25, 3.0)]["O"] == 376 and int(47250 * 0.008) == 378
    assert geo[(37800.0, 0.8, -5.0)]["O"] == 296 and int(37800 * 0.008) == 302
    for k in ((2000.0, 2.0, 7.0), (8000.0, 0.5, 0.0), (47250.0, 1.25, 3.0), (37800.0, 0.8, -5.0)):
        assert geo[k]["nseg"] == 5 and geo[k]["N1"] - 4 * (geo[k]["S"] - geo[k]["O"]) < 16, k      # four segments and a few frames
    for k in ((204800.0, 0.5, 0.0), (204800.0, 0.25, 0.0)):
        assert geo[k]["W"] + geo[k]["O"] == 4096 + 512 == sr_.MAX_WINDOW and geo[k]["nseg"] >= 3
    for k in ((96000.0, 1.25, 0.0), (96000.0, 0.8, 3.0)):
        assert geo[k]["O"] == 512 and all(kind == "rail" for _, _, _, kind in seen[k])
    rail = source(96000.0, 2, 30000, seed=1, kind="rail")
    assert set(np.unique(sr_.quantise(rail))) == {-32767, 32767}
    L = geo[(48000.0, 0.5, 0.0)]["S"] - geo[(48000.0, 0.5, 0.0)]["O"]
    assert [(g["nseg"], g["N1"]) for g, _, c, _ in seen[(48000.0, 0.5, 0.0)] if c == 1] == [(1, L - 2), (1, L), (2, L + 2), (2, 2 * L)]
    assert [g["N"] + 8 for g, _, c, _ in seen[(48000.0, 1.0, 3.0)] if c == 1] == [256, 257, 512, 513]
    assert all(g["stretch"] for g, _, _, _ in seen[(48000.0, 1.0, 3.0)])


GRID = cases()
EDGE = edge_cases()


@pytest.mark.parametrize("sr,ch,speed,pitch,gain,length,kind", [c + ("noise",) for c in GRID] + EDGE,
                         ids=[f"{int(c[0])}-{c[1]}ch-s{c[2]}-p{c[3]}-g{c[4]}-n{c[5]}" for c in GRID] + ["edge-" + edge_id(c) for c in EDGE])
def test_host_build_equals_the_restatement(host, sr, ch, speed, pitch, gain, length, kind):
    src = source(sr, ch, length, seed=length + 7 * ch, kind=kind)
    ref, roffs = sr_.render(src, sr, gain, pitch, speed)
    out, offs = host_render(host, src, sr, gain, pitch, speed)
    assert same_bits(out, ref), np.flatnonzero((out != ref).any(axis=0))[:10]
    assert np.array_equal(offs.astype(np.int64), roffs)
    if kind == "rail" or sr == 204800.0:
        assert roffs.any()                                         # (the scores differ: the seek has something to decide)


@pytest.mark.parametrize("sr,ch,period", tie_cases(), ids=[f"{int(c[0])}-{c[1]}ch-P{c[2]}" for c in tie_cases()])
def test_periodic_clips_tie_and_the_smallest_offset_wins(host, sr, ch, period):
    """candidates a period apart score the same to the bit; the host build and the restatement take the first of them"""
    src = tie_source(sr, ch, period)
    ref, roffs = sr_.render(src, sr, 0.0, 0.0, TIE_SPEED)
    out, offs = host_render(host, src, sr, 0.0, 0.0, TIE_SPEED)
    assert same_bits(out, ref) and np.array_equal(offs.astype(np.int64), roffs)
    assert same_bits(src[:, period:], src[:, :-period])
    holds_ties(sr, period, roffs)


@pytest.mark.parametrize("sr,pitch,speed", LAST_FRAME_CASES)
@pytest.mark.parametrize("ch", [1, 2])
def test_the_last_staged_frame_decides_a_seek(host, sr, pitch, speed, ch):
    src = last_frame_source(sr, ch, pitch, speed)
    ref, roffs = sr_.render(src, sr, 0.0, pitch, speed)
    out, offs = host_render(host, src, sr, 0.0, pitch, speed)
    assert same_bits(out, ref) and np.array_equal(offs.astype(np.int64), roffs)
    assert roffs[1] == 0 and roffs[2] == sr_.geometry(sr, src.shape[1], 0.0, pitch, speed)["W"] - 1


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
