"""K2's on-grid form (libzl_amd/csrc/zl_render.h), CPU tier: the one-tap mix against the plain linear expression with alpha = 0,
the predicate that selects it, and the host scan that sets a source's "verified finite" flag -- built for the host.

What "equal" means here is what reaches the outputs: a frame's (lout, rout) may differ in the SIGN OF A ZERO only (the dropped term
is a signed zero), the bus sum from +0.0f and the report peak may not differ at all.  tests/test_k2_ongrid.py holds the kernel's
parity with the oracle on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

from libzl_amd import build

_lib = None
FLT_MAX = np.finfo(np.float32).max
DEN = np.float32(1e-45)                      # the smallest denormal


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_ongrid_harness())
        fp = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
        l.zlog_mix.restype = None
        l.zlog_mix.argtypes = [C.c_int, C.c_int] + [fp] * 14
        l.zlog_sum_peak.restype = None
        l.zlog_sum_peak.argtypes = [C.c_int, C.c_int] + [fp] * 5
        l.zlog_predicate.restype = C.c_int
        l.zlog_predicate.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
        l.zlog_all_finite.restype = C.c_int
        l.zlog_all_finite.argtypes = [fp, C.c_longlong]
        l.zlog_sound_finite_flag.restype = C.c_int
        _lib = l
    return _lib


SAMPLES = np.array([0.0, -0.0, DEN, -DEN, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, 1.0, -1.0, 0.5, -0.25, 1e-20, 3e20], dtype=np.float32)
GAINS = np.array([0.0, -0.0, 1.0, -1.0, 0.7, -0.3, DEN, 1e-30, 1e30, -1e30, FLT_MAX, -FLT_MAX], dtype=np.float32)
PANS = np.array([0.0, 1.0, 0.5, 0.25, -0.0, 1e-30, DEN], dtype=np.float32)


def operands(rng, n):
    """n frames: samples and gains drawn half from the adversarial sets, half at random"""
    def draw(pool, lo, hi):
        a = rng.uniform(lo, hi, n).astype(np.float32)
        pick = rng.random(n) < 0.5
        a[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
        return np.ascontiguousarray(a)
    x = [draw(SAMPLES, -1, 1) for _ in range(4)]
    g = [draw(GAINS, -2, 2) for _ in range(4)]
    p = [draw(PANS, 0, 1) for _ in range(2)]
    return x, g, p


def mix(stereo, x, g, p):
    n = x[0].size
    out = [np.empty(n, np.float32) for _ in range(4)]
    lib().zlog_mix(n, stereo, *x, *g, *p, *out)
    return out


def same_or_both_zero(a, b):
    """equal bits, or both zero (any signs), or both NaN"""
    eq = a.view(np.int32) == b.view(np.int32)
    zz = (a == 0) & (b == 0)
    nn = np.isnan(a) & np.isnan(b)
    return eq | zz | nn


@pytest.mark.parametrize("stereo", [1, 0])
def test_frames_equal_up_to_the_sign_of_a_zero(stereo):
    rng = np.random.default_rng(61 + stereo)
    x, g, p = operands(rng, 1 << 20)
    fl, fr, sl, sr = mix(stereo, x, g, p)
    okl, okr = same_or_both_zero(fl, sl), same_or_both_zero(fr, sr)
    assert okl.all() and okr.all(), f"first differing frame {int(np.argmin(okl & okr))}"
    # every adversarial sample met every kind of gain: the pools are small against a million draws
    assert (np.isin(x[2], SAMPLES) & np.isin(g[0], GAINS)).sum() > 1000


@pytest.mark.parametrize("stereo", [1, 0])
def test_bus_sum_and_report_peak_bit_for_bit(stereo):
    """128 voices in voice order from +0.0f, 4096 frames: the sum and every voice's report peak carry no trace of the zero's sign"""
    V, F = 128, 4096
    rng = np.random.default_rng(67 + stereo)
    x, g, p = operands(rng, V * F)
    # frames in which EVERY voice is silent are where a -0 could survive in a sum: force a good share of them
    silent = rng.random(F) < 0.2
    for a in x:
        a.reshape(V, F)[:, silent] = np.where(rng.random((V, int(silent.sum()))) < 0.5, np.float32(0.0), np.float32(-0.0))
    fl, fr, sl, sr = mix(stereo, x, g, p)
    res = []
    for l, r in ((fl, fr), (sl, sr)):
        acc_l, acc_r, peak = np.empty(F, np.float32), np.empty(F, np.float32), np.empty(V, np.float32)
        lib().zlog_sum_peak(V, F, np.ascontiguousarray(l), np.ascontiguousarray(r), acc_l, acc_r, peak)
        res.append((acc_l, acc_r, peak))
    for a, b in zip(res[0], res[1]):
        nn = np.isnan(a) & np.isnan(b)                               # (FLT_MAX operands overflow to inf - inf in both forms alike)
        assert ((a.view(np.int32) == b.view(np.int32)) | nn).all()
    assert (res[0][0][silent].view(np.int32) == 0).all()             # +0.0f, not -0.0f


def test_a_non_finite_second_tap_is_why_the_flag_exists():
    one = np.ones(1, np.float32)
    for bad in (np.inf, -np.inf, np.nan):
        x = [one.copy(), one.copy(), np.full(1, bad, np.float32), one.copy()]
        fl, fr, sl, sr = mix(1, x, [one] * 4, [one * np.float32(0.5)] * 2)
        assert np.isnan(fl[0]) and not np.isnan(sl[0])


def test_predicate():
    l = lib()
    FIN = l.zlog_sound_finite_flag()
    assert FIN == 1
    ok = dict(mode=0, enabled=1, simple=1, unit=1, interior=1, P0=1234.0, step=1.0, flags=FIN)

    def pred(**kw):
        a = dict(ok); a.update(kw)
        return l.zlog_predicate(a["mode"], a["enabled"], a["simple"], a["unit"], a["interior"], a["P0"], a["step"], a["flags"])
    assert pred() == 1
    assert pred(P0=0.0) == 1 and pred(P0=float(2 ** 30 - 1)) == 1
    assert pred(mode=2) == 1                                         # FIX_DELAY: the same mix, another store
    assert pred(P0=1234.5) == 0 and pred(P0=1234.0 + 2.0 ** -40) == 0 and pred(P0=np.nextafter(1234.0, 0.0)) == 0
    assert pred(step=2.0) == 0 and pred(step=0.5) == 0 and pred(step=np.nextafter(1.0, 2.0)) == 0
    assert pred(flags=0) == 0 and pred(flags=2) == 0
    assert pred(mode=4) == 0 and pred(mode=1) == 0 and pred(mode=3) == 0 and pred(mode=6) == 0       # Hermite, FIX_GAIN
    assert pred(enabled=0) == 0
    assert pred(simple=0) == 0 and pred(unit=0) == 0 and pred(interior=0) == 0


def test_host_scan_sets_the_flag_only_for_finite_sources():
    l = lib()
    rng = np.random.default_rng(71)
    clean = rng.uniform(-1, 1, 5000).astype(np.float32)
    clean[::7] = SAMPLES[rng.integers(0, len(SAMPLES), clean[::7].size)]     # +-0, denormals, +-FLT_MAX: all finite
    assert l.zlog_all_finite(clean, clean.size) == 1
    for bad in (np.nan, np.inf, -np.inf, "snan"):
        for at in (0, 2500, 4999):
            x = clean.copy()
            if bad == "snan":
                x.view(np.int32)[at] = 0x7f800001                  # a signalling NaN's bits
            else:
                x[at] = bad
            assert l.zlog_all_finite(x, x.size) == 0
    assert l.zlog_all_finite(clean[:0].copy(), 0) == 1
