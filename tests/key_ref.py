"""numpy / Python-integer restatement of the key detection (include/zlhip.h, zlhip_sound_key), written from the
definition and not from libzl_amd/csrc/zl_key.h.  The bin table and the cosine table are INPUTS (the library's, zlhip_key_design), so
that a libm difference in exp2 or cos cannot enter; design() is numpy's own version of them, for the test of the table itself.

    table    bin of MIDI note n: f = a4 2^((n - 69) / 12); N = rint(q rate / f), + 1 if odd, at most 32768; step = rint(f / rate 2^32);
             wstep = 2^32 // N;  T[i] = rint(32767 cos(2 pi i / 4096)), int16
    frames   L = the largest N; n < L: none; K = (n - L) // hop + 1; K > max_frames: K = max_frames, hop = (n - L) // (max_frames - 1);
             frame k spans [first + k hop, + L); bin b reads [off, off + N) of it, off = (L - N) // 2
    mix      m[f] = sum over the channels of clamp(rint(4096 v), +-32767), NaN -> 0
    gate     e = sum of m^2 over the span; e < L channels gate^2: silent (re = im = 0, contributes nothing)
    bin      w = (32767 - T[(j wstep mod 2^32) >> 20]) >> 1; v = (m w) >> 15; ph = j step mod 2^32; c = T[ph >> 20];
             s = T[((ph - 2^30) mod 2^32) >> 20]; re = sum v c, im = sum v s
    energy   a = trunc(re / N) >> 8, b = trunc(im / N) >> 8 (shifts arithmetic); e = a^2 + b^2
    bin gate e counts only if e L >= the frame's span energy (a bin under -33 dB of a tone of the frame's power is leakage and rounding)
    totals   B[b] = sum of the counting e over the sounding frames; C[p] = sum of B[b] over the bins with n mod 12 = p
    finish   x = float(C); Pearson's r with the 24 rotated Krumhansl-Kessler profiles in serial double arithmetic; the best and the
             runner-up, equal values to the smaller index; no frames, no sounding frame or zero variance: tonic = -1, the rest 0
"""
import math

import numpy as np

from pitch_ref import quantise

MAJOR = (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)
MINOR = (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)
RESULT_INTS = ("tonic", "mode", "second_tonic", "second_mode", "frames", "sounding")
M32 = (1 << 32) - 1


def hz_of(note, a4=440.0):
    return a4 * 2.0 ** ((note - 69.0) / 12.0)


def resolve(sample_rate, num_frames=100000, hop=0, max_frames=0, a4_hz=0.0, note_lo=0, note_hi=0, q=0, gate=0, first_frame=0):
    """the fields given as 0 filled with their defaults; None where a limit that needs no sound is broken"""
    if not (0.0 < sample_rate < 1e9) or first_frame < 0 or num_frames < 1:
        return None
    a4 = float(np.float32(a4_hz)) or 440.0
    note_lo, note_hi, q, hop, max_frames, gate = note_lo or 36, note_hi or 95, q or 34, hop or 8192, max_frames or 256, gate or 8
    if not (math.isfinite(a4) and 220.0 <= a4 <= 880.0):
        return None
    if not (1 <= note_lo <= note_hi <= 127 and note_hi - note_lo + 1 <= 96):
        return None
    if not (1 <= q <= 256 and 1 <= hop <= 1 << 24 and 1 <= gate <= 32767 and 1 <= max_frames <= 256):
        return None
    top = hz_of(note_hi, a4)
    if not top < sample_rate / 2.0 or round(q * sample_rate / top) < 32:
        return None
    return dict(hop=hop, max_frames=max_frames, a4_hz=a4, note_lo=note_lo, note_hi=note_hi, q=q, gate=gate)


def design(rate, a4=440.0, note_lo=36, note_hi=95, q=34):
    """numpy's own table: ([(note, N, step, wstep)], T int16 [4096])"""
    bins = []
    for n in range(note_lo, note_hi + 1):
        f = hz_of(n, a4)
        N = int(np.rint(q * rate / f))
        N = min(32768, N + (N & 1))
        bins.append((n, N, int(np.rint(f / rate * 4294967296.0)), (1 << 32) // N))
    T = np.rint(32767.0 * np.cos(2.0 * np.pi * np.arange(4096) / 4096.0)).astype(np.int16)
    return bins, T


def library_table(z, rate, **f):
    """the library's table (z: the bound libzlhip) of a request's fields at a rate: ([(note, N, step, wstep)], T int16 [4096]), or None
    where the library refuses the request"""
    import ctypes as C
    from libzl_amd import _abi
    r = _abi.KeyRequest(0, 0, 1, f.get("hop", 0), f.get("max_frames", 0), f.get("a4_hz", 0.0), f.get("note_lo", 0), f.get("note_hi", 0), f.get("q", 0), f.get("gate", 0))
    n = C.c_int32(0)
    if z.zlhip_key_design(rate, C.byref(r), None, 0, C.byref(n), None) != 0:
        return None
    bins = (_abi.KeyBin * n.value)()
    T = np.zeros(4096, np.int16)
    assert z.zlhip_key_design(rate, C.byref(r), C.addressof(bins), n.value, C.byref(n), T.ctypes.data) == 0
    return [(b.note, b.n, b.step, b.wstep) for b in bins], T


def frames_of(n, L, hop, max_frames):
    """(K, hop)"""
    if n < L:
        return 0, hop
    K = (n - L) // hop + 1
    if K <= max_frames:
        return K, hop
    return max_frames, ((n - L) // (max_frames - 1) if max_frames > 1 else hop)


def factors(b, T):
    """a bin's window, cosine and sine factors per j, int64 [N] each"""
    _, N, step, wstep = b
    T = np.asarray(T, np.int64)
    j = np.arange(N, dtype=np.int64)
    w = (32767 - T[((j * wstep) & M32) >> 20]) >> 1
    ph = (j * step) & M32
    return w, T[ph >> 20], T[((ph - (1 << 30)) & M32) >> 20]


def correlate(seg, fac):
    """(re, im) of a bin over its N mixed samples, as Python integers; the sums stay below 2^46"""
    w, c, s = fac
    v = (seg * w) >> 15
    assert int(np.abs(seg * w).max(initial=0)) < 1 << 31 and int(np.abs(v * c).max(initial=0)) < 1 << 31 and int(np.abs(v * s).max(initial=0)) < 1 << 31
    return int((v * c).sum()), int((v * s).sum())


def _tdiv(a, n):
    return -((-a) // n) if a < 0 else a // n


def energy(re, im, N):
    a, b = _tdiv(re, N) >> 8, _tdiv(im, N) >> 8
    assert abs(a) <= 1 << 23 and abs(b) <= 1 << 23
    return a * a + b * b


def correlation(x, mx, sxx, i):
    prof = MAJOR if i < 12 else MINOR
    tonic = i % 12
    y = [prof[(p - tonic + 12) % 12] for p in range(12)]
    my = 0.0
    for p in range(12):
        my += y[p]
    my /= 12.0
    sxy = syy = 0.0
    for p in range(12):
        sxy += (x[p] - mx) * (y[p] - my)
        syy += (y[p] - my) * (y[p] - my)
    return sxy / math.sqrt(sxx * syy)


def finish(chroma, frames, sounding):
    res = dict(tonic=-1, mode=0, second_tonic=0, second_mode=0, frames=frames, sounding=0, confidence=0.0, second_confidence=0.0, chroma=(0,) * 12)
    x = [float(c) for c in chroma]
    mx = 0.0
    for p in range(12):
        mx += x[p]
    mx /= 12.0
    sxx = 0.0
    for p in range(12):
        sxx += (x[p] - mx) * (x[p] - mx)
    if frames == 0 or sounding == 0 or not sxx > 0.0:
        return res
    r = [correlation(x, mx, sxx, i) for i in range(24)]
    best = max(range(24), key=lambda i: (r[i], -i))
    second = max((i for i in range(24) if i != best), key=lambda i: (r[i], -i))
    res.update(tonic=best % 12, mode=best // 12, confidence=r[best], second_tonic=second % 12, second_mode=second // 12, second_confidence=r[second],
               sounding=sounding, chroma=tuple(int(c) for c in chroma))
    return res


def key(x, rate, bins, T, first=0, n=None, hop=0, max_frames=0, gate=0):
    """the whole request over x: float32 [channels][frames], with the table (bins: [(note, N, step, wstep)], T) as resolved by the
    library -> (result dict, per-bin totals [int], frames [dict(silent, re [int], im [int])])"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    n = x.shape[1] - first if n is None else n
    hop, max_frames, gate = hop or 8192, max_frames or 256, gate or 8
    assert first >= 0 and n >= 1 and first + n <= x.shape[1] and len(bins) <= 96 and max_frames <= 256
    bins = [tuple(int(v) for v in b) for b in bins]
    L = max(b[1] for b in bins)
    assert L == bins[0][1] and all(b[1] % 2 == 0 and 32 <= b[1] <= 32768 for b in bins)
    K, hop = frames_of(n, L, hop, max_frames)
    m = quantise(x[:, first:first + n])
    fac = [factors(b, T) for b in bins]
    recs, totals, sounding = [], [0] * len(bins), 0
    for k in range(K):
        seg = m[k * hop:k * hop + L]
        assert len(seg) == L
        e = int((seg * seg).sum())
        silent = e < L * x.shape[0] * gate * gate
        rec = dict(silent=silent, re=[0] * len(bins), im=[0] * len(bins))
        if not silent:
            sounding += 1
            for i, b in enumerate(bins):
                off = (L - b[1]) // 2
                rec["re"][i], rec["im"][i] = correlate(seg[off:off + b[1]], fac[i])
                eb = energy(rec["re"][i], rec["im"][i], b[1])
                assert eb * L < 1 << 62
                totals[i] += eb if eb * L >= e else 0
        recs.append(rec)
    assert all(t < 1 << 55 for t in totals)
    chroma = [sum(t for t, b in zip(totals, bins) if b[0] % 12 == p) for p in range(12)]
    assert all(c < 1 << 62 for c in chroma)
    return finish(chroma, K, sounding), totals, recs


def exact_bin(seg, note, N, rate, a4=440.0):
    """|re + i im| of a bin in float64 with an exact cosine and an exact Hann window, over the bin's N mixed samples, on the integer
    sums' scale (w -> 32767 hann / 32768 ... : 32767^2 / 32768)"""
    j = np.arange(N)
    hann = 0.5 * (1.0 - np.cos(2.0 * np.pi * j / N))
    z = (seg * hann * np.exp(-2j * np.pi * hz_of(note, a4) / rate * j)).sum()
    return abs(z) * 32767.0 * 32767.0 / 32768.0


def match_shift(clip_tonic, clip_mode, tonic, mode):
    """libzl_hotpath_clip_match_key's rule"""
    src = clip_tonic if clip_mode == mode else (clip_tonic + (9 if clip_mode == 0 else 3)) % 12
    return (tonic - src + 6) % 12 - 6


# ---- the cadences ---------------------------------------------------------------------------------------------------------------
def chord(rate, seconds, root, minor):
    """a triad plus the bass an octave under its root, four harmonics at 1 / h"""
    t = np.arange(int(rate * seconds)) / rate
    y = np.zeros(len(t))
    for note in (root - 12, root, root + (3 if minor else 4), root + 7):
        for h in range(1, 5):
            y += np.sin(2.0 * np.pi * h * hz_of(note) * t) / h
    return y


def cadence(rate, tonic, minor, seconds=0.75):
    """I-IV-V-I (major) or i-iv-v-i (natural minor), tonic 0 .. 11, root in the octave of MIDI 48; 16-bit; mono float32 [1][frames]"""
    root = 48 + tonic
    y = np.concatenate([chord(rate, seconds, root + d, minor) for d in (0, 5, 7, 0)])
    y = np.rint(0.5 * y / np.abs(y).max() * 32767.0) / 32768.0
    return y.astype(np.float32)[None, :]


def repitch(x, semitones):
    """a pure re-pitch: the samples read 2^(semitones / 12) times as fast, linearly interpolated"""
    x = np.atleast_2d(x)
    r = 2.0 ** (semitones / 12.0)
    pos = np.arange(int((x.shape[1] - 1) / r)) * r
    return np.stack([np.interp(pos, np.arange(x.shape[1]), c) for c in x]).astype(np.float32)
