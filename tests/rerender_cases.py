"""The parameter grid of the clip re-render tests (tests/test_rerender_cpu.py against the host build, tests/test_rerender_gpu.py
against the device): every speed x pitch pair for every sample rate and channel count, the gains and lengths dealt round robin."""
from __future__ import annotations

import numpy as np

SPEEDS = (0.25, 0.5, 0.8, 1.0, 1.25, 2.0, 4.0)
PITCHES = (-24.0, -12.0, -5.0, 0.0, 3.0, 7.0, 12.0, 24.0)
GAINS = (-6.0, 0.0, 3.0)
RATES = (44100.0, 48000.0, 96000.0)


def lengths(sr: float, speed: float, pitch: float):
    """1, O - 1, S, S + W + O and 3 s for the rate and the parameters (from the restatement's geometry)."""
    from stretch_ref import geometry
    g = geometry(sr, 1000, 0.0, pitch, speed)
    return (1, g["O"] - 1, g["S"], g["S"] + g["W"] + g["O"], int(3 * sr))


def cases(long_every: int = 1):
    """(sr, channels, speed, pitch, gain, length).  long_every > 1 keeps only every n-th 3-second case (the rest get S + W + O)."""
    out, n, nlong = [], 0, 0
    for sr in RATES:
        for ch in (1, 2):
            for speed in SPEEDS:
                for pitch in PITCHES:
                    lens = lengths(sr, speed, pitch)
                    length = lens[n % len(lens)]
                    if length == lens[-1]:
                        nlong += 1
                        if nlong % long_every:
                            length = lens[3]
                    out.append((sr, ch, speed, pitch, GAINS[n % len(GAINS)], length))
                    n += 1
    return out


def source(sr: float, ch: int, length: int, seed: int, kind: str = "noise") -> np.ndarray:
    """planar float32 [ch, length]: "noise" (uniform, with a 440 Hz sine under it), "zeros", or "special" (noise with NaN and
    +-1e6 samples sprinkled in)."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((ch, length), np.float32)
    t = np.arange(length) / sr
    x = (0.5 * np.sin(2 * np.pi * 440.0 * t)[None, :] + rng.uniform(-0.4, 0.4, (ch, length))).astype(np.float32)
    if kind == "special":
        idx = rng.integers(0, length, (ch, max(1, length // 500)))
        for c in range(ch):
            x[c, idx[c][0::3]] = np.nan
            x[c, idx[c][1::3]] = 1e6
            x[c, idx[c][2::3]] = -1e6
    return x


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal bit for bit, NaN positions compared as NaN (x86 and gfx950 need not agree on NaN payloads)."""
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))
