"""The clip edit restated in numpy, independently of libzl_amd/csrc/zl_edit.h: the resolve, the exact trim
(smallest and largest loud frame, float32 comparisons), the kept region in Python integers, the fades cut to half the result, the
weights in float64 in the written order (only *, /, - and sqrt: correctly rounded, so they equal the header's doubles) rounded to
float32, the output with one rounded float32 multiply per faded sample, and the arena's layout of an extent.  Clips are planar float32
arrays [channels, frames]."""
import numpy as np

f32 = np.float32
TRIM, REVERSE = 1, 2
LINEAR, SQRT, SMOOTH = 0, 1, 2
THRESHOLD = f32(2.0 ** -10)
PAD = 8
CHUNK = 2048        # frames of a scanning workgroup, WG: 16-byte groups of a render workgroup (what the cases aim their edges at)
WG = 256
RESULT_FIELDS = ("applied", "silent", "first_frame", "num_frames", "first_loud", "last_loud", "fade_in_frames", "fade_out_frames", "length", "reversed", "curve")
REQUEST_KEYS = ("first_frame", "num_frames", "flags", "pre_roll_frames", "hold_frames", "fade_in_frames", "fade_out_frames", "curve", "threshold")


def request(**kw):
    """a request's fields, missing ones 0"""
    q = {k: 0 for k in REQUEST_KEYS}
    q["threshold"] = 0.0
    q.update(kw)
    return q


def resolve(length, q):
    """(a, b, threshold as float32), or None where the request is refused"""
    a, num = q["first_frame"], q["num_frames"]
    if length < 1 or a < 0 or num < 0:
        return None
    if (a >= length) if num == 0 else (a + num > length):
        return None
    if q["flags"] & ~(TRIM | REVERSE) or q["curve"] not in (LINEAR, SQRT, SMOOTH):
        return None
    thr = f32(q["threshold"])
    if not (thr == 0 or (thr > 0 and np.isfinite(thr))):
        return None
    if min(q["pre_roll_frames"], q["hold_frames"], q["fade_in_frames"], q["fade_out_frames"]) < 0:
        return None
    return a, (length if num == 0 else a + num), (THRESHOLD if thr == 0 else thr)


def loud(x, thr):
    """per frame: some channel's sample is not below the threshold in float32 (NaN and inf are loud, |x| == threshold is loud)"""
    with np.errstate(invalid="ignore"):
        return np.any(~(np.abs(x.astype(f32)) < f32(thr)), axis=0)


def scan(x, a, b, thr):
    """(F, Z): the smallest and the largest loud frame of [a, b), or None"""
    at = np.flatnonzero(loud(x[:, a:b], thr))
    return None if at.size == 0 else (a + int(at[0]), a + int(at[-1]))


def design(X, curve):
    """the rising weights, float32 [X]"""
    t = np.arange(X, dtype=np.float64) / np.float64(max(X, 1))
    if curve == SQRT:
        t = np.sqrt(t)
    elif curve == SMOOTH:
        t = (t * t) * (3.0 - (2.0 * t))
    return t.astype(f32)


def edit(x, q, w_in=None, w_out=None):
    """(result dict, the clip afterwards, planar).  w_in, w_out: weight tables taken from elsewhere instead of designed here"""
    length = x.shape[1]
    r = resolve(length, q)
    assert r is not None
    a, b, thr = r
    res = dict(applied=0, silent=0, first_frame=a, num_frames=b - a, first_loud=-1, last_loud=-1, fade_in_frames=0, fade_out_frames=0,
               length=length, reversed=0, curve=q["curve"])
    a2, b2 = a, b
    if q["flags"] & TRIM:
        fz = scan(x, a, b, thr)
        if fz is None:
            res["silent"] = 1
            return res, np.array(x, f32, copy=True)
        res["first_loud"], res["last_loud"] = fz
        a2, b2 = max(a, fz[0] - q["pre_roll_frames"]), min(b, fz[1] + 1 + q["hold_frames"])
    n = b2 - a2
    assert n >= 1
    Xi, Xo = min(q["fade_in_frames"], n // 2), min(q["fade_out_frames"], n // 2)
    rev = bool(q["flags"] & REVERSE)
    res.update(first_frame=a2, num_frames=n, length=n)
    if a2 == 0 and n == length and not rev and Xi == 0 and Xo == 0:
        return res, np.array(x, f32, copy=True)
    res.update(applied=1, fade_in_frames=Xi, fade_out_frames=Xo, reversed=int(rev))
    y = np.array(x[:, a2:b2], f32, copy=True)
    if rev:
        y = np.ascontiguousarray(y[:, ::-1])
    wi = design(Xi, q["curve"]) if w_in is None else np.asarray(w_in, f32)
    wo = design(Xo, q["curve"]) if w_out is None else np.asarray(w_out, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        if Xi:
            y[:, :Xi] = (wi[None, :] * y[:, :Xi]).astype(f32)
        if Xo:
            y[:, n - Xo:] = (wo[::-1][None, :] * y[:, n - Xo:]).astype(f32)
    return res, y


def faded_finite(y, Xi, Xo):
    n = y.shape[1]
    return bool(np.all(np.isfinite(y[:, :Xi])) and np.all(np.isfinite(y[:, n - Xo:] if Xo else y[:, :0])))


def extent(y):
    """a planar clip as it lies in the arena: interleaved, 8 zero frames behind, zeros up to the 16-byte boundary"""
    ch, n = y.shape
    floats = ((n + PAD) * ch + 3) & ~3
    out = np.zeros(floats, f32)
    out[:n * ch] = y.T.reshape(-1)
    return out
