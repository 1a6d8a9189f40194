"""numpy / Python-integer restatement of the pitch detection (include/zlhip.h, zlhip_sound_pitch), written from the
definition and not from libzl_amd/csrc/zl_pitch.h:

    lags     t_min = max(2, ceil(rate / f_max)), t_max = floor(rate / f_min); W = window (0: min(4096, roundup(2 t_max, 64)));
             L = W + t_max + 1
    frames   n < L: none; hop = W, K = (n - L) // hop + 1; K > max_frames: K = max_frames, hop = (n - L) // (max_frames - 1)
    mix      m[f] = sum over the channels of clamp(rint(4096 v), +-32767), NaN -> 0
    gate     e = sum of m^2 over the frame's first W samples; e < W channels gate^2: silent
    shift    sh = max(0, bitlength(max |m| over the L samples) - 12); x = m >> sh (arithmetic)
    d[t]     sum over j < W of (x[j] - x[j + t])^2, t in [1, t_max + 1];  C[t] = d[1] + ... + d[t]
    t0       the smallest t in [t_min, t_max] with d[t] t 1024 < threshold C[t]; none: unvoiced
    lag      the first t >= t0 with t = t_max or d[t + 1] >= d[t];  clarity = level(C[lag] + 1) - level(d[lag] lag + 1)
    vote     lower median of the voiced lags; consistent: |lag - med| <= med >> 5; representative: largest clarity, then earliest
    finish   den = (d_lo - 2 d_mid) + d_hi; delta = (d_lo - d_hi) / (2 den) if den > 0 else 0, clamped to +-0.5; hz = rate / (lag + delta);
             note = 69 + 12 log2(hz / 440); root_note = clamp(rint(note), 0, 127); cents = 100 (note - root_note);
             confidence = consistent / frames; the four floats cast to float32
"""
import math

import numpy as np

VOICED, SILENT, UNVOICED = 0, 1, 2
FRAME_INTS = ("lag", "clarity", "shift", "flag", "d_lo", "d_mid", "d_hi", "cum")
RESULT_INTS = ("root_note", "frames", "voiced", "consistent", "frame", "lag", "shift", "clarity", "d_lo", "d_mid", "d_hi", "cum")


def lags(rate, f_min, f_max):
    return max(2, math.ceil(rate / f_max)), math.floor(rate / f_min)


def resolve(sample_rate, num_frames=100000, window=0, max_frames=0, f_min=0.0, f_max=0.0, threshold=0, gate=0, first_frame=0):
    """the fields given as 0 filled with their defaults; None where a limit that needs no sound is broken"""
    if not (0.0 < sample_rate < 1e9) or first_frame < 0 or num_frames < 1:
        return None
    f_min = float(np.float32(f_min)) or 55.0
    f_max = float(np.float32(f_max)) or 1760.0
    threshold = threshold or 154
    gate = gate or 8
    max_frames = max_frames or 64
    if not (math.isfinite(f_min) and math.isfinite(f_max) and 20.0 <= f_min < f_max < sample_rate / 2.0):
        return None
    tmin, tmax = lags(sample_rate, f_min, f_max)
    if tmax + 1 > 2048:
        return None
    if window == 0:
        window = min(4096, -(-2 * tmax // 64) * 64)
    if window % 64 or not 256 <= window <= 4096 or tmax + 1 > window:
        return None
    if not (1 <= threshold <= 1024 and 1 <= gate <= 32767 and 1 <= max_frames <= 256):
        return None
    return dict(window=int(window), max_frames=int(max_frames), f_min=f_min, f_max=f_max, threshold=int(threshold), gate=int(gate))


def frames_of(n, window, tmax, max_frames):
    """(K, hop)"""
    L = window + tmax + 1
    if n < L:
        return 0, window
    K = (n - L) // window + 1
    if K <= max_frames:
        return K, window
    return max_frames, ((n - L) // (max_frames - 1) if max_frames > 1 else window)


def quantise(x):
    """clamp(rint(4096 v), +-32767) in float32 as the device does, NaN -> 0; x: float32 [channels][frames] -> int64 mono mix [frames]"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint(x * np.float32(4096.0))
    t = np.where(np.isnan(x), np.float32(0.0), np.clip(t, np.float32(-32767.0), np.float32(32767.0)))
    return t.astype(np.int64).sum(axis=0)


def level(x):
    """section 12's L(x), x >= 1"""
    p = x.bit_length() - 1
    m = x - (1 << p)
    return 64 * p + (m >> (p - 6) if p >= 6 else m << (6 - p))


def diff(x, W, tmax):
    """d[1 .. t_max + 1] as Python integers; x: int64 [L], |x| <= 2^12.  e(0) + e(t) - 2 r(t): the correlation runs in float64, whose sums
    of integers stay below 2^12 * 2^12 * 4096 = 2^36 and are therefore exact"""
    assert len(x) == W + tmax + 1 and int(np.abs(x).max(initial=0)) <= 4096
    sq = np.concatenate([[0], np.cumsum(x * x)])
    e = sq[W:] - sq[:-W]                                           # e[t] = sum of x[t .. t + W)^2, t in [0, t_max + 1]
    r = np.correlate(x.astype(np.float64), x[:W].astype(np.float64), "valid")
    assert len(r) == tmax + 2
    d = int(e[0]) + e[1:] - 2 * r[1:].astype(np.int64)
    return [int(v) for v in d]


def diff_direct(x, W, tmax):
    return [int(((x[:W] - x[t:t + W]) ** 2).sum()) for t in range(1, tmax + 2)]


def pick(d, tmin, tmax, threshold, silent, shift):
    """a frame's record from d (d[t] at d[t - 1])"""
    rec = dict(lag=0, clarity=0, shift=shift, flag=SILENT if silent else UNVOICED, d_lo=0, d_mid=0, d_hi=0, cum=0)
    if silent:
        return rec
    C, t0 = [0], 0
    for t in range(1, tmax + 2):
        C.append(C[-1] + d[t - 1])
    for t in range(tmin, tmax + 1):
        if d[t - 1] * t * 1024 < threshold * C[t]:
            t0 = t
            break
    if t0 == 0:
        return rec
    t = t0
    while not (t == tmax or d[t] >= d[t - 1]):
        t += 1
    return dict(lag=t, clarity=level(C[t] + 1) - level(d[t - 1] * t + 1), shift=shift, flag=VOICED, d_lo=d[t - 2], d_mid=d[t - 1], d_hi=d[t], cum=C[t])


def vote(frames):
    K = len(frames)
    res = dict(root_note=0, frames=K, voiced=0, consistent=0, frame=0, lag=0, shift=0, clarity=0, d_lo=0, d_mid=0, d_hi=0, cum=0)
    voiced = sorted(f["lag"] for f in frames if f["lag"] > 0)
    if not voiced:
        return res
    med = voiced[(len(voiced) - 1) // 2]
    cons = [k for k, f in enumerate(frames) if f["lag"] > 0 and abs(f["lag"] - med) <= med >> 5]
    rep = max(cons, key=lambda k: (frames[k]["clarity"], -k))
    f = frames[rep]
    res.update(voiced=len(voiced), consistent=len(cons), frame=rep, lag=f["lag"], shift=f["shift"], clarity=f["clarity"], d_lo=f["d_lo"], d_mid=f["d_mid"],
               d_hi=f["d_hi"], cum=f["cum"])
    return res


def finish(res, rate):
    """hz, note, cents, confidence (float32) and root_note into the integer result"""
    res.update(hz=np.float32(0.0), note=np.float32(0.0), cents=np.float32(0.0), confidence=np.float32(0.0), root_note=0)
    if res["lag"] == 0:
        return res
    lo, mid, hi = float(res["d_lo"]), float(res["d_mid"]), float(res["d_hi"])
    den = (lo - 2.0 * mid) + hi
    delta = (lo - hi) / (2.0 * den) if den > 0.0 else 0.0
    delta = min(0.5, max(-0.5, delta))
    hz = rate / (float(res["lag"]) + delta)
    note = 69.0 + 12.0 * math.log2(hz / 440.0)
    root = min(127.0, max(0.0, float(np.rint(note))))
    res.update(hz=np.float32(hz), note=np.float32(note), root_note=int(root), cents=np.float32(100.0 * (note - root)),
               confidence=np.float32(float(res["consistent"]) / float(res["frames"])))
    return res


def pitch(x, rate, first=0, n=None, window=0, max_frames=0, f_min=0.0, f_max=0.0, threshold=0, gate=0, want_d=False):
    """the whole request over x: float32 [channels][frames] -> (result dict, frame records[, d per frame])"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    n = x.shape[1] - first if n is None else n
    q = resolve(rate, n, window, max_frames, f_min, f_max, threshold, gate, first)
    assert q is not None and first + n <= x.shape[1]
    tmin, tmax = lags(rate, q["f_min"], q["f_max"])
    W = q["window"]
    L = W + tmax + 1
    K, hop = frames_of(n, W, tmax, q["max_frames"])
    m = quantise(x[:, first:first + n])
    recs, ds = [], []
    for k in range(K):
        seg = m[k * hop:k * hop + L]
        e = int((seg[:W] * seg[:W]).sum())
        shift = max(0, int(np.abs(seg).max()).bit_length() - 12)
        d = diff(seg >> shift, W, tmax)
        recs.append(pick(d, tmin, tmax, q["threshold"], e < W * x.shape[0] * q["gate"] ** 2, shift))
        ds.append(d)
    res = finish(vote(recs), rate)
    return (res, recs, ds) if want_d else (res, recs)


# ---- the signals of the accuracy cases ----------------------------------------------------------------------------------------------
def hz_of(note):
    return 440.0 * 2.0 ** ((note - 69.0) / 12.0)


def _harmonics(rate, seconds, f, amps):
    t = np.arange(int(rate * seconds)) / rate
    y = np.zeros(len(t))
    for h, a in amps:
        if h * f < rate / 2.0:
            y += a * np.sin(2.0 * np.pi * h * f * t)
    return t, y


def sine(rate, seconds, f):
    return _harmonics(rate, seconds, f, [(1, 1.0)])[1]


def saw(rate, seconds, f):
    return _harmonics(rate, seconds, f, [(h, 1.0 / h) for h in range(1, 21)])[1]


def pluck(rate, seconds, f):
    t, y = _harmonics(rate, seconds, f, [(h, 1.0 / h) for h in range(1, 9)])
    return y * np.exp(-2.0 * t)                                    # (-17 dB after a second: still 12 dB above the cases' noise)


def missing_fundamental(rate, seconds, f):
    return _harmonics(rate, seconds, f, [(h, 1.0) for h in range(2, 7)])[1]


SIGNALS = (sine, saw, pluck, missing_fundamental)


def clip(signal, rate, note, level, seconds=1.0, seed=0):
    """a mono float32 clip [1][frames]: the signal at the power of a sine of peak `level` (measured over the whole clip), with 1 % of
    `level` as white noise"""
    y = signal(rate, seconds, hz_of(note))
    y = y / np.sqrt(2.0 * np.mean(y * y))
    rng = np.random.default_rng(seed)
    return (level * (y + 0.01 * rng.standard_normal(len(y)))).astype(np.float32)[None, :]
