"""numpy / Python-integer restatement of the tempo estimate (include/zlhip.h, zlhip_sound_tempo), written from the
definition and not from libzl_amd/csrc/zl_tempo.h:

    E[h]     section 12's hop energies (onset_ref.energy)
    R[h]     floor(sqrt(E[h])), R[-1] = 0;  s = max(0, bitlength(max R) - 16);  W[h] = max(0, R[h] - R[h-1]) >> s;  S = sum of W
    lags     l_min = max(1, ceil(60 rate / (hop bpm_max))), l_max = min(floor(60 rate / (hop bpm_min)), cap), cap = (hops - 1) // 2
    A[l]     sum over h >= l of W[h] W[h-l], for l = 0 and l in [max(1, l_min - 1), min(8 l_max + 8, cap + 1)]
    order    a beats b iff A[a] (hops - b) > A[b] (hops - a); equal goes to the smaller lag
    coarse   the best lag in [l_min, l_max];  doublings: m <- best of {2m-1, 2m, 2m+1} while K < 3 and 2m + 1 <= cap
    no tempo l_min > l_max or A[0] == 0: everything 0 except hops, shift, sum and acf_zero
    finish   y_d = A[m+d] / (hops - m - d); den = (y- - 2 y0) + y+; delta = (y- - y+) / (2 den) if den < 0 else 0, clamped to +-0.5;
             period = (m + delta) / 2^K; bpm = 60 rate / (hop period); mu = S / hops; confidence = (y0 - mu^2) / (A[0] / hops - mu^2),
             0 where that denominator is not positive; both cast to float32
"""
import math

import numpy as np

import onset_ref as onr

MAX_LAG = 1024
MAX_HOPS = 65536


def resolve(sample_rate, num_frames=1000, hop=0, bpm_min=0.0, bpm_max=0.0, first_frame=0):
    """the fields given as 0 filled with their defaults; None where a limit that needs no sound is broken"""
    if not (0.0 < sample_rate < 1e9) or first_frame < 0 or num_frames < 1:
        return None
    if hop == 0:
        r = onr.resolve(sample_rate)
        if r is None:
            return None
        hop = r["hop"]
    if hop % 16 or not 64 <= hop <= 4096:
        return None
    bpm_min = float(np.float32(bpm_min)) or 75.0
    bpm_max = float(np.float32(bpm_max)) or 150.0
    if not (math.isfinite(bpm_min) and math.isfinite(bpm_max) and 20.0 <= bpm_min < bpm_max <= 400.0):
        return None
    if -(-num_frames // hop) > MAX_HOPS:
        return None
    if lags(sample_rate, hop, bpm_min, bpm_max, 1 << 30)[1] > MAX_LAG:
        return None
    return dict(hop=int(hop), bpm_min=bpm_min, bpm_max=bpm_max)


def isqrt(x):
    return math.isqrt(int(x))


def flux(E):
    """(W uint16 [hops], shift, sum)"""
    R = [isqrt(v) for v in E]
    s = max(0, max(R).bit_length() - 16)
    W = [max(0, a - b) >> s for a, b in zip(R, [0] + R[:-1])]
    assert max(W) < 1 << 16
    return np.array(W, np.uint16), s, sum(W)


def lags(rate, hop, bpm_min, bpm_max, hops):
    """(l_min, l_max, cap), l_max already cut to cap"""
    lmin = max(1, math.ceil((60.0 * rate) / (float(hop) * bpm_max)))
    lmax = math.floor((60.0 * rate) / (float(hop) * bpm_min))
    cap = (hops - 1) // 2
    return lmin, min(lmax, cap), cap


def lag_range(lmin, lmax, cap):
    """the lags besides 0 that are evaluated: (first, last), empty where first > last"""
    return max(1, lmin - 1), min(8 * lmax + 8, cap + 1)


def acf_at(W, lag):
    w = W.astype(np.uint64)
    return int((w[lag:] * w[:len(w) - lag]).sum(dtype=np.uint64)) if lag < len(w) else 0


def acf(W, first, last):
    """A over [first, last] as a list of Python integers (FFT-free: exact integer products, 8-lag blocks)"""
    w = W.astype(np.int64)
    out = []
    for lag in range(first, last + 1):
        out.append(int(np.dot(w[lag:], w[:len(w) - lag])) if lag < len(w) else 0)   # (below 2^48: exact in int64)
    return out


def beats(A, hops, a, b):
    """lag a strictly before lag b in the order"""
    x, y = A[a] * (hops - b), A[b] * (hops - a)
    assert x < 1 << 64 and y < 1 << 64
    return x > y or (x == y and a < b)


def best(A, hops, cands):
    m = None
    for c in cands:
        if m is None or beats(A, hops, c, m):
            m = c
    return m


def finish(rate, hop, rec):
    """(bpm, confidence) as float32 from the integer record"""
    if rec["lag_fine"] == 0:
        return np.float32(0.0), np.float32(0.0)
    m, K, hops = rec["lag_fine"], rec["doublings"], rec["hops"]
    ym = float(rec["acf_lo"]) / float(hops - m + 1)
    y0 = float(rec["acf_mid"]) / float(hops - m)
    yp = float(rec["acf_hi"]) / float(hops - m - 1)
    den = (ym - 2.0 * y0) + yp
    d = (ym - yp) / (2.0 * den) if den < 0.0 else 0.0
    d = min(0.5, max(-0.5, d))
    period = (float(m) + d) / float(1 << K)
    bpm = (60.0 * rate) / (float(hop) * period)
    mu = float(rec["sum"]) / float(hops)
    cden = float(rec["acf_zero"]) / float(hops) - mu * mu
    conf = (y0 - mu * mu) / cden if cden > 0.0 else 0.0
    return np.float32(bpm), np.float32(conf)


def tempo_from_energy(E, rate, hop, bpm_min=75.0, bpm_max=150.0):
    """the result record (a dict of the C struct's fields) plus W, first_lag and A over the evaluated lags"""
    hops = len(E)
    W, s, total = flux(E)
    lmin, lmax, cap = lags(rate, hop, float(np.float32(bpm_min)), float(np.float32(bpm_max)), hops)
    first, last = lag_range(lmin, lmax, cap)
    a0 = acf_at(W, 0)
    rec = dict(bpm=np.float32(0), confidence=np.float32(0), lag_coarse=0, lag_fine=0, doublings=0, shift=s, hops=hops, acf_lo=0, acf_mid=0,
               acf_hi=0, acf_zero=a0, sum=total)
    if lmin > lmax:
        return rec, W, first, []
    vals = acf(W, first, last)
    if a0 == 0:
        return rec, W, first, vals
    A = {0: a0}
    A.update({first + i: v for i, v in enumerate(vals)})
    coarse = best(A, hops, range(lmin, lmax + 1))
    m, K = coarse, 0
    while K < 3 and 2 * m + 1 <= cap:
        m = best(A, hops, (2 * m - 1, 2 * m, 2 * m + 1))
        K += 1
    rec.update(lag_coarse=coarse, lag_fine=m, doublings=K, acf_lo=A[m - 1], acf_mid=A[m], acf_hi=A[m + 1])
    rec["bpm"], rec["confidence"] = finish(rate, hop, rec)
    return rec, W, first, vals


def tempo(planar, rate, first=0, n=None, hop=0, bpm_min=0.0, bpm_max=0.0):
    """planar: float32 [channels][length] -> tempo_from_energy's tuple over the request"""
    planar = np.ascontiguousarray(planar, np.float32)
    n = planar.shape[1] - first if n is None else n
    r = resolve(rate, n, hop, bpm_min, bpm_max, first)
    assert r is not None and first + n <= planar.shape[1]
    E = onr.energy(planar, first, n, r["hop"])
    return tempo_from_energy(E, rate, r["hop"], r["bpm_min"], r["bpm_max"])


# ---- the test patterns ----------------------------------------------------------------------------------------
def _bursts(rate, seconds, bpm, hits, seed):
    """hits: (position in beats within a bar of 4, amplitude); noise bursts with a decay of 300 samples"""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * rate))
    x = np.zeros(n + 4096, np.float64)
    env = np.exp(-np.arange(4096) / 300.0)
    beat = 60.0 * rate / bpm
    bar = 0
    while True:
        placed = False
        for pos, amp in hits:
            f = int(round((4 * bar + pos) * beat))
            if f < n:
                x[f:f + 4096] += amp * env * rng.uniform(-1.0, 1.0, 4096)
                placed = True
        if not placed:
            break
        bar += 1
    return x[:n].astype(np.float32)[None, :]


def pattern_a(rate, seconds, bpm, seed=1):
    hits = [(0, 0.8), (1, 0.5), (2, 0.5), (3, 0.5)] + [(k + 0.5, 0.15) for k in range(4)]
    return _bursts(rate, seconds, bpm, hits, seed)


def pattern_b(rate, seconds, bpm, seed=2):
    hits = [(0, 0.8), (1, 0.6), (2, 0.8), (3, 0.6)] + [(k + j / 4.0, 0.1) for k in range(4) for j in (1, 2, 3)]
    return _bursts(rate, seconds, bpm, hits, seed)
