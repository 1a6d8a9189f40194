"""Independent numpy restatement of the clip re-render (zlhip_sound_rerender), written from the definition and
not from the C++ of libzl_amd/csrc/zl_stretch.h.

    r = 2^(pitch/12), tau = speed / r (float64);  N = max(1, floor(len / speed)) output frames at the source's rate
    stretch (tau != 1): WSOLA in segments of S - O frames, each cross-faded over O frames from the tail of the previous one and
        placed by an exact integer correlation seek over W candidate offsets;  x has N1 = floor(len / tau) frames
    resample (pitch != 0): linear, y[j] = x[i](1 - a) + x[i+1] a, p = j r, i = floor(p), a = float32(p - i);  x = 0 beyond N1
    gain (gain_db != 0): y * float32(10^(gain_db/20))
    identity (0 dB, 0 semitones, speed 1): the source itself

Float arithmetic is float32 with one rounding per operation; the seek is int64 plus one float64 division and square root per
candidate.  render() returns (planar float32 [ch, N], offsets int64 [nseg])."""
from __future__ import annotations

import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

f32 = np.float32
MAX_WINDOW = 4608          # W + O, the longest seek window a render may have


def geometry(sr: float, length: int, gain_db: float, pitch: float, speed: float) -> dict:
    gain_db, pitch, speed = f32(gain_db), f32(pitch), f32(speed)
    if not (0.25 <= speed <= 4.0) or not (-24.0 <= pitch <= 24.0) or not np.isfinite(gain_db):
        raise ValueError("parameters out of range")
    r = math.pow(2.0, float(pitch) / 12.0)
    tau = float(speed) / r
    N = max(1, math.floor(length / float(speed)))
    O = min(512, max(16, math.floor(sr * 0.008)))
    O -= O % 8
    # SoundTouch 2.x automatic sequence / seek lengths as restated (unpinned)
    seq_ms = min(max(90 + (40 - 90) / 1.5 * (tau - 0.5), 40), 90)
    seek_ms = min(max(20 + (15 - 20) / 1.5 * (tau - 0.5), 15), 20)
    S = math.floor(sr * seq_ms / 1000)
    W = math.floor(sr * seek_ms / 1000)
    stretch = tau != 1.0
    # a source the stretch cannot take: the sequence must be longer than the overlap it is cross-faded over (rates below 425 Hz at
    # tau >= 2), there must be a candidate to seek over, and the seek window W + O must fit the 4608 frames the seek stages per
    # channel (rates from 204850 Hz at tau <= 0.5).  Where the stretch does not run there is nothing to reject
    if stretch and (S <= O or W < 1 or W + O > MAX_WINDOW):
        raise ValueError("a sample rate the stretch cannot take")
    N1 = math.floor(length / tau) if stretch else length
    nseg = -(-N1 // (S - O)) if stretch else 0
    return dict(r=r, tau=tau, N=N, N1=N1, O=O, S=S, W=W, nseg=nseg, stretch=stretch, resample=bool(pitch != 0),
                gain=bool(gain_db != 0), g=f32(math.pow(10.0, float(gain_db) / 20.0)), step=tau * (S - O))


def quantise(v: np.ndarray) -> np.ndarray:
    """q(v) = clamp(rint(v * 4096), -32767, 32767), ties to even, NaN -> 0; float32 product."""
    t = np.rint(v.astype(f32) * f32(4096.0))
    t = np.where(np.isnan(t), f32(0.0), t)
    return np.clip(t, -32767.0, 32767.0).astype(np.int64)


def _stretch(src: np.ndarray, geo: dict):
    ch, length = src.shape
    O, S, W, nseg, N1 = geo["O"], geo["S"], geo["W"], geo["nseg"], geo["N1"]
    L = S - O
    if nseg == 0:
        return np.zeros((ch, 0), f32), np.zeros(0, np.int64)
    bases = [math.floor(k * geo["step"]) for k in range(nseg)]
    total = max(length, bases[-1] + W + S + O + 1)
    pad = np.zeros((ch, total), f32)
    pad[:, :length] = src
    q = quantise(pad)
    energy = np.concatenate([[0], np.cumsum((q * q).sum(axis=0))])       # exact int64 prefix sums of sum_ch q^2
    i = np.arange(O, dtype=np.int64)
    weight = i * (O - i)
    offs = np.zeros(nseg, np.int64)
    prev = 0
    for k in range(1, nseg):
        base = bases[k]
        ref = (quantise(pad[:, prev + L: prev + L + O]) * weight) >> 16              # [ch, O], arithmetic shift
        win = sliding_window_view(q[:, base: base + W + O - 1], O, axis=1)        # [ch, W, O]
        corr = np.einsum("cwo,co->w", win, ref)
        norm = energy[base + O: base + O + W] - energy[base: base + W]
        score = np.zeros(W, np.float64)
        nz = norm != 0
        score[nz] = corr[nz].astype(np.float64) / np.sqrt(norm[nz].astype(np.float64))
        offs[k] = int(np.argmax(score))                                           # the first maximum: ties go to the smallest offset
        prev = base + int(offs[k])
    x = np.zeros((ch, nseg * L), f32)
    nfade = min(O, L)
    w = np.arange(nfade).astype(f32) / f32(O)
    for k in range(nseg):
        b = bases[k] + int(offs[k])
        seg = pad[:, b: b + L].copy()
        if k > 0:
            bp = bases[k - 1] + int(offs[k - 1])
            mid = pad[:, bp + L: bp + L + nfade]
            seg[:, :nfade] = mid * (f32(1.0) - w) + seg[:, :nfade] * w
        x[:, k * L: (k + 1) * L] = seg
    return x[:, :N1], offs


def render(src: np.ndarray, sr: float, gain_db: float = 0.0, pitch: float = 0.0, speed: float = 1.0):
    """src: planar float32 [ch, len].  Returns (planar float32 [ch, N], seek offsets [nseg])."""
    src = np.asarray(src, dtype=f32)
    ch, length = src.shape
    geo = geometry(sr, length, gain_db, pitch, speed)
    if f32(gain_db) == 0 and f32(pitch) == 0 and f32(speed) == 1:
        return src.copy(), np.zeros(0, np.int64)
    if geo["stretch"]:
        x, offs = _stretch(src, geo)
    else:
        x, offs = src, np.zeros(0, np.int64)
    N = geo["N"]
    if geo["resample"]:
        p = np.arange(N, dtype=np.int64) * geo["r"]
        i = np.floor(p).astype(np.int64)
        a = (p - i).astype(f32)
        xe = np.zeros((ch, int(i[-1]) + 2), f32)
        n = min(x.shape[1], xe.shape[1])
        xe[:, :n] = x[:, :n]
        y = xe[:, i] * (f32(1.0) - a) + xe[:, i + 1] * a
    else:
        y = np.zeros((ch, N), f32)
        n = min(x.shape[1], N)
        y[:, :n] = x[:, :n]
    if geo["gain"]:
        y = y * geo["g"]
    return y.astype(f32), offs
