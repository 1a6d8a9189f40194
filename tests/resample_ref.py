"""The sample-rate conversion restated in numpy, independently of libzl_amd/csrc/zl_resample.h: the ratio, the
Kaiser-windowed sinc table (np.sinc, np.i0, in double) and the convolution (vectorised over the output frames; per tap one fp32
multiply, then one fp32 add, in tap order), and in Python integers a frame's position and the span of input frames a workgroup of 256
output frames stages.  The tests hold the header's host build and the kernel against it."""
from math import gcd

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
PAD = 8
BETA = 10.0
CUTOFF = 0.95
BASE_HALF = 32


def geometry(fs, ft):
    """(L, M, half, taps, row floats) of a conversion from fs to ft, or None where the definition does not take it"""
    if fs != int(fs) or ft != int(ft) or not (1000 <= fs <= 768000 and 1000 <= ft <= 768000):
        return None
    fs, ft = int(fs), int(ft)
    g = gcd(fs, ft)
    L, M = ft // g, fs // g
    if L > 2048 or M > 8 * L:
        return None
    half = BASE_HALF if L >= M else -((-BASE_HALF * M) // L)        # ceil(32 / s), s = min(1, L / M)
    taps = 2 * half
    row = (taps + 3) // 4 * 4
    if L * row > 262144:
        return None
    return L, M, half, taps, row


def design64(fs, ft):
    """the rows in double, each of unit sum: [L, taps]"""
    L, M, half, taps, _ = geometry(fs, ft)
    s = min(1.0, L / M)
    c = CUTOFF * s
    p = np.arange(L, dtype=f64)[:, None]
    t = np.arange(taps, dtype=f64)[None, :]
    d = (t - half + 1) - p / L
    u = d / half
    w = np.where(np.abs(d) < half, np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA), 0.0)
    h = c * np.sinc(c * d) * w
    return h / h.sum(axis=1, keepdims=True)


def design(fs, ft):
    """the table as it is stored: float32 [L, row], zeros in the pad"""
    L, _, _, taps, row = geometry(fs, ft)
    table = np.zeros((L, row), f32)
    table[:, :taps] = design64(fs, ft).astype(f32)
    return table


def out_frames(fs, ft, length):
    L, M = geometry(fs, ft)[:2]
    return (int(length) * L + M - 1) // M


WG = 256                                                          # output frames of a workgroup
STAGE_FRAMES = (WG - 1) * 8 + 512 + 1                             # what a workgroup stages at most: M <= 8 L, T <= 512


def position(fs, ft, j):
    """(i, p) of output frame j, in Python integers"""
    L, M = geometry(fs, ft)[:2]
    return (j * M) // L, (j * M) % L


def span(fs, ft, N, w):
    """(first, count): the input frames workgroup w of a clip of N output frames stages"""
    L, M, half, taps, _ = geometry(fs, ft)
    j0 = w * WG
    j1 = min(j0 + WG, N) - 1
    return (j0 * M) // L - half + 1, (j1 * M) // L - (j0 * M) // L + taps


def staged_counts(fs, ft, length):
    """the staged count of every workgroup of a clip of `length` source frames"""
    N = out_frames(fs, ft, length)
    return [span(fs, ft, N, w)[1] for w in range((N + WG - 1) // WG)]


def lengths_for(fs, ft, N):
    """the source lengths that put the output at N frames; where no length does (an upsampling ratio skips output counts: 1:6 gives
    multiples of 6 only) the two lengths whose counts lie closest below and above N"""
    L, M = geometry(fs, ft)[:2]
    n = max(1, ((N - 1) * M) // L)
    while out_frames(fs, ft, n) < N:
        n += 1
    if out_frames(fs, ft, n) == N or n == 1:
        return [n]
    return [n - 1, n]


def convert(table, fs, ft, x):
    """x: float32 [length, channels] -> float32 [N, channels] with the given table ([L, row] float32)"""
    L, M, half, taps, _ = geometry(fs, ft)
    x = np.asarray(x, f32)
    n, ch = x.shape
    N = (n * L + M - 1) // M
    xp = np.zeros((n + 2 * half, ch), f32)                        # +0 outside [0, length)
    xp[half:half + n] = x
    q = np.arange(N, dtype=i64) * M
    i, p = q // L, q % L
    acc = np.zeros((N, ch), f32)
    with np.errstate(all="ignore"):
        for t in range(taps):
            m = table[p, t][:, None] * xp[i + 1 + t]               # frame i - half + 1 + t
            acc = acc + m
    assert acc.dtype == f32
    return acc


def extent(y):
    """the arena extent of a converted clip: interleaved, PAD zero frames behind, zeros to the 16-byte boundary"""
    N, ch = y.shape
    floats = ((N + PAD) * ch + 3) // 4 * 4
    out = np.zeros(floats, f32)
    out[:N * ch] = y.reshape(-1)
    return out


def linear(fs, ft, x):
    """what the voice's own resampler does to a clip at a foreign rate: two taps at position j * fs / ft (double), no filter"""
    x = np.asarray(x, f64)
    N = out_frames(fs, ft, x.shape[0])
    pos = np.arange(N, dtype=f64) * (fs / ft)
    i = np.minimum(pos.astype(i64), x.shape[0] - 1)
    frac = pos - i
    nxt = np.minimum(i + 1, x.shape[0] - 1)
    return (x[i] * (1.0 - frac)[:, None] + x[nxt] * frac[:, None]).astype(f32)


def ulp32(v):
    v = np.abs(np.asarray(v, f32))
    return (np.nextafter(v, f32(np.inf)) - v).astype(f64)
