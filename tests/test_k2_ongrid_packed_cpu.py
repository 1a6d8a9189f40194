"""K2's packed on-grid mix, CPU tier: the operation sequence of zl_mix_acc_ongrid_pk (zl_kernels.hip) restated in plain C++
(zl_render.h, zl_mix_frame_ongrid_pk: a - b as a + (-b), the difference times 1.0f) against the two forms that define the frame --
zl_mix_frame_ongrid, and zl_mix_frame<0> with alpha = 0.  Equal means equal bits, or NaN on both sides.

The two-tap expression adds a zero whose sign is the second tap's and the gain chain's; it is called here as the definition of a frame
whose dropped term has the first tap's own sign (second tap = first tap, gains of 1), where it returns l = x0l and r = x0r to the bit.
What the sign of that zero may do to a frame otherwise -- and why it reaches no bus -- is tests/test_k2_ongrid_cpu.py's subject.
tests/test_k2_ongrid_packed.py holds the kernels' parity with the oracle on the GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from libzl_amd import build

FLT_MAX = np.finfo(np.float32).max
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, 1.0, -1.0], dtype=np.float32)   # ADVERSARIAL of test_k2_ongrid.py

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_ongrid_pk_harness())
        fp = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
        l.zlpk_mix.restype = None
        l.zlpk_mix.argtypes = [C.c_int] + [fp] * 10
        l.zlpk_sum.restype = None
        l.zlpk_sum.argtypes = [C.c_int, C.c_int] + [fp] * 8
        _lib = l
    return _lib


def pan_law(pan):
    """(lpan, rpan) of a clip's pan as K1 forms them (zl_plan.h, :193-194)"""
    pan = np.asarray(pan, dtype=np.float32).astype(np.float64)
    return (0.5 * (1.0 + pan)).astype(np.float32), (0.5 * (1.0 - pan)).astype(np.float32)


def same_bits_or_both_nan(a, b):
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


def mix(xl, xr, lp, rp):
    n = xl.size
    out = [np.empty(n, np.float32) for _ in range(6)]
    lib().zlpk_mix(n, *(np.ascontiguousarray(a, dtype=np.float32) for a in (xl, xr, lp, rp)), *out)
    return out


def check(xl, xr, lp, rp):
    pl, pr, ol, orr, tl, tr = mix(xl, xr, lp, rp)
    for name, a, b in (("left / one tap", pl, ol), ("right / one tap", pr, orr), ("left / two taps", pl, tl), ("right / two taps", pr, tr)):
        ok = same_bits_or_both_nan(a, b)
        i = int(np.argmin(ok))
        assert ok.all(), f"{name}: frame {i}: x = ({xl[i]!r}, {xr[i]!r}), pan = ({lp[i]!r}, {rp[i]!r}): {a[i]!r} != {b[i]!r}"


def test_a_million_random_frames():
    rng = np.random.default_rng(0x9C01)
    n = 1_000_000
    # half of them audio-sized, half spread over the whole exponent range (sums that overflow, products that go denormal)
    xl = rng.uniform(-1, 1, n).astype(np.float32)
    xr = rng.uniform(-1, 1, n).astype(np.float32)
    wide = rng.random(n) < 0.5
    with np.errstate(over="ignore"):
        xl[wide] *= np.exp2(rng.uniform(-149, 127, int(wide.sum()))).astype(np.float32)
        xr[wide] *= np.exp2(rng.uniform(-149, 127, int(wide.sum()))).astype(np.float32)
    xl[~np.isfinite(xl)] = FLT_MAX; xr[~np.isfinite(xr)] = -FLT_MAX
    pan = rng.uniform(-1, 1, n).astype(np.float32)
    fixed = rng.integers(0, 4, n)
    pan[fixed == 0] = -1.0; pan[fixed == 1] = 0.0; pan[fixed == 2] = 1.0
    check(xl, xr, *pan_law(pan))


def test_every_pairing_of_the_special_values():
    rng = np.random.default_rng(0x9C02)
    pans = np.concatenate([np.array([-1.0, 0.0, 1.0], np.float32), rng.uniform(-1, 1, 29).astype(np.float32)])
    trip = np.array(list(itertools.product(SPECIAL, SPECIAL, pans)), dtype=np.float32)
    assert trip.shape == (len(SPECIAL) ** 2 * 32, 3)
    check(np.ascontiguousarray(trip[:, 0]), np.ascontiguousarray(trip[:, 1]), *pan_law(trip[:, 2]))
    # ... and each special value against random ones, on either side
    r = rng.uniform(-1, 1, trip.shape[0]).astype(np.float32)
    check(np.ascontiguousarray(trip[:, 0]), r, *pan_law(trip[:, 2]))
    check(r, np.ascontiguousarray(trip[:, 1]), *pan_law(trip[:, 2]))
    # the overflow the pairings are there for did happen: FLT_MAX + FLT_MAX, and inf * 0 at a hard pan
    pl = mix(np.ascontiguousarray(trip[:, 0]), np.ascontiguousarray(trip[:, 1]), *pan_law(trip[:, 2]))[0]
    assert np.isnan(pl).any() and np.isinf(pl).any()


@pytest.mark.parametrize("mono", [False, True])
def test_bus_sums_in_voice_order(mono):
    """128 voices of 64 frames summed from +0.0f in voice order, special values among them: the accumulators agree to the bit"""
    rng = np.random.default_rng(0x9C03 + mono)
    V, F = 128, 64
    xl = rng.uniform(-1, 1, (V, F)).astype(np.float32)
    xr = xl.copy() if mono else rng.uniform(-1, 1, (V, F)).astype(np.float32)
    pick = rng.random((V, F)) < 0.2
    xl[pick] = SPECIAL[rng.integers(0, len(SPECIAL) - 2, int(pick.sum()))]
    if mono:
        xr = xl.copy()                                               # a mono source passes (x, x)
    pan = rng.uniform(-1, 1, V).astype(np.float32)
    pan[:3] = (-1.0, 0.0, 1.0)
    lp, rp = pan_law(pan)
    out = [np.empty(F, np.float32) for _ in range(4)]
    lib().zlpk_sum(V, F, np.ascontiguousarray(xl), np.ascontiguousarray(xr), lp, rp, *out)
    assert same_bits_or_both_nan(out[0], out[2]).all() and same_bits_or_both_nan(out[1], out[3]).all()
