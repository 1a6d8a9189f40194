"""The loop crossfade restated in numpy and Python integers, independently of libzl_amd/csrc/zl_xfade.h: the
resolve, the exact correlation sums, the finish and the weights in float64 (only *, / and sqrt: correctly rounded, so they equal the
header's doubles), the output in float32 with two rounded multiplies and one rounded add, and the arena's layout of an extent.
Clips are planar float32 arrays [channels, frames]."""
import math

import numpy as np

f32 = np.float32
AUTO, LINEAR, EQUAL_POWER = 0, 1, 2
MAX_FADE = 65536
PAD = 8
RESULT_INTS = ("applied", "fade_frames", "start_frame", "stop_frame", "curve", "sab", "saa", "sbb")


def resolve(rate, length, s, e, X=0, curve=AUTO):
    """the frames to fade (0: nothing to fade), or None where the request is refused"""
    if not (0 <= s < e <= length) or curve not in (AUTO, LINEAR, EQUAL_POWER) or not (0.0 < rate < 1e9):
        return None
    most = min(s, e - s, MAX_FADE)
    if X == 0:
        return int(min(np.rint(0.020 * rate), most))
    return X if 1 <= X <= most else None


def q16(v):
    """section 8's quantisation: clamp(rint(4096 v), +-32767) in float32, NaN -> 0"""
    v = np.asarray(v, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.rint(v * f32(4096.0))
    t = np.where(np.isnan(v), f32(0.0), np.clip(t, f32(-32767.0), f32(32767.0)))
    return t.astype(np.int64)


def sums(x, s, e, X):
    """(sab, saa, sbb) as Python integers"""
    m = q16(x).sum(axis=0)
    a = [int(v) for v in m[e - X:e]]
    b = [int(v) for v in m[s - X:s]]
    return sum(p * r for p, r in zip(a, b)), sum(p * p for p in a), sum(r * r for r in b)


def finish(sab, saa, sbb):
    """(correlation, rho)"""
    corr = 0.0 if saa == 0 or sbb == 0 else float(sab) / math.sqrt(float(saa) * float(sbb))
    return corr, min(1.0, max(0.0, corr))


def curve_rho(curve, measured):
    return 1.0 if curve == LINEAR else 0.0 if curve == EQUAL_POWER else measured


def design(X, rho):
    """the weight pairs, float32 [X, 2]"""
    t = np.arange(1, X + 1, dtype=np.float64) / np.float64(X)
    u = 1.0 - t
    d = np.sqrt(((u * u) + (t * t)) + ((2.0 * np.float64(rho)) * (t * u)))
    return np.stack([(u / d).astype(f32), (t / d).astype(f32)], axis=1)


def apply(x, s, e, ab):
    """the crossfaded clip, planar"""
    X = ab.shape[0]
    y = np.array(x, f32, copy=True)
    a, b = ab[:, 0][None, :], ab[:, 1][None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        p = (a * x[:, e - X:e]).astype(f32)
        r = (b * x[:, s - X:s]).astype(f32)
        y[:, e - X:e] = (p + r).astype(f32)
    return y


def extent(y):
    """a planar clip as it lies in the arena: interleaved, 8 zero frames behind, zeros up to the 16-byte boundary"""
    ch, n = y.shape
    floats = ((n + PAD) * ch + 3) & ~3
    out = np.zeros(floats, f32)
    out[:n * ch] = y.T.reshape(-1)
    return out


def crossfade(x, rate, s, e, X=0, curve=AUTO, ints=None, ab=None):
    """(result dict, crossfaded planar clip).  ints: (sab, saa, sbb) taken from elsewhere instead of computed here; ab: a weight table
    taken from elsewhere instead of designed here"""
    X = resolve(rate, x.shape[1], s, e, X, curve)
    assert X is not None
    if X == 0:
        return dict(applied=0, fade_frames=0, start_frame=0, stop_frame=0, curve=0, sab=0, saa=0, sbb=0, correlation=0.0, rho=0.0), np.array(x, f32, copy=True)
    sab, saa, sbb = sums(x, s, e, X) if ints is None else ints
    corr, rho = finish(sab, saa, sbb)
    rho = curve_rho(curve, rho)
    if ab is None:
        ab = design(X, rho)
    res = dict(applied=1, fade_frames=X, start_frame=s, stop_frame=e, curve=curve, sab=sab, saa=saa, sbb=sbb, correlation=corr, rho=rho)
    return res, apply(x, s, e, ab)


def all_finite(y, s, e, X):
    return bool(np.all(np.isfinite(y[:, e - X:e])))


# ---- signals ------------------------------------------------------------------------------------------------------------------------
def noise(seed, ch, n, level=0.25):
    return (np.random.default_rng(seed).standard_normal((ch, n)) * level).astype(f32)


def tone(period, ch, n, level=0.3, decay=None):
    """two harmonics of `period` frames; decay: the time constant in frames of an exponential decay"""
    t = np.arange(n, dtype=np.float64)
    v = level * (np.sin(2.0 * np.pi * t / period) + 0.5 * np.sin(4.0 * np.pi * t / period + 0.7))
    if decay is not None:
        v = v * np.exp(-t / decay)
    return np.stack([v * (1.0 - 0.1 * c) for c in range(ch)]).astype(f32)


def ms_db(y, lo, hi):
    """10 log10 of the mean square of frames [lo, hi) over the channels"""
    return 10.0 * np.log10(float(np.mean(y[:, lo:hi].astype(np.float64) ** 2)))
