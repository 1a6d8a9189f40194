"""The parameter grid of the clip re-render tests (tests/test_rerender_cpu.py against the host build, tests/test_rerender_gpu.py
against the device): every speed x pitch pair for every sample rate and channel count, the gains and lengths dealt round robin.
Next to it the edge cases both tiers share (tests/test_rerender_edges_gpu.py on the device): the limits of the geometry, clips at the
rails, periodic clips whose candidates tie, a clip whose seek hangs on the last frame a candidate reads, and the helpers that go
with them (references computed once, an arena dirtied with noise, a clip's extent as the arena holds it)."""
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


SYNTH_WG = 256        # frames per workgroup of the synthesis kernel
PAD = 8               # zero frames behind every extent


def edge_cases():
    """(sr, channels, speed, pitch, gain, length, kind): the limits of the geometry and of the kernels' launch shapes, mono and stereo
    each.  Lengths that depend on the geometry come from the restatement's; with L = S - O, "four segments" is ceil(4 L tau) + 7."""
    import math
    from stretch_ref import geometry

    def four(sr, speed, pitch):
        g = geometry(sr, 1000, 0.0, pitch, speed)
        return math.ceil(4 * (g["S"] - g["O"]) * g["tau"]) + 7

    rows = [
        (425.0, 4.0, 0.0, 50, "noise"),                            # O = 16 (the minimum), L = 1 < O, W = 6
        (500.0, 0.5, 0.0, 65, "noise"),                            # O = 16, L = 29 > O, W = 10
        (2000.0, 2.0, 7.0, four(2000.0, 2.0, 7.0), "noise"),       # W = 34: less than one wave
        (8000.0, 0.5, 0.0, four(8000.0, 0.5, 0.0), "noise"),       # W = 160: less than one pass, five waves idle
        (47250.0, 1.25, 3.0, four(47250.0, 1.25, 3.0), "noise"),   # O: 378 -> 376
        (37800.0, 0.8, -5.0, four(37800.0, 0.8, -5.0), "noise"),   # O: 302 -> 296
        (204800.0, 0.5, 0.0, 18000, "noise"),                      # W + O = 4096 + 512 = 4608: the staging at its limit
        (204800.0, 0.25, 0.0, 18000, "noise"),
        (96000.0, 1.25, 0.0, 30000, "rail"),                       # O = 512, |q| = 32767 everywhere: the int32 pair bound
        (96000.0, 0.8, 3.0, 30000, "rail"),
    ]
    g = geometry(48000.0, 1000, 0.0, 0.0, 0.5)                     # tau = 0.5: N1 = 2 len
    L = g["S"] - g["O"]
    assert L % 2 == 0
    rows += [(48000.0, 0.5, 0.0, n, "noise") for n in (L // 2 - 1, L // 2, L // 2 + 1, L)]       # nseg = 1; N1 = L; L + 2; 2 L
    rows += [(48000.0, 1.0, 3.0, n - PAD, "noise") for n in (SYNTH_WG, SYNTH_WG + 1, 2 * SYNTH_WG, 2 * SYNTH_WG + 1)]   # N = len
    out = []
    for sr, speed, pitch, length, kind in rows:
        for ch in (1, 2):
            out.append((sr, ch, speed, pitch, GAINS[len(out) % len(GAINS)], length, kind))
    return out


TIE_LENGTH, TIE_SPEED = 30000, 0.8


def tie_cases():
    """(sr, channels, period) of the periodic clips (TIE_LENGTH frames at TIE_SPEED, pitch 0): the candidates o, o + P, o + 2 P ... of
    a window inside the clip score the same to the bit.  P = 37: they lie in different lanes of one wave; P = 64: in the same lane
    of neighbouring waves; P = 512: in one thread, on successive passes"""
    return [(sr, ch, P) for sr, P in ((48000.0, 37), (48000.0, 64), (48000.0, 512), (96000.0, 512)) for ch in (1, 2)]


def tie_source(sr: float, ch: int, period: int) -> np.ndarray:
    return source(sr, ch, TIE_LENGTH, seed=period + ch, kind="periodic", period=period)


def segments_inside(sr: float, length: int, pitch: float, speed: float, offs) -> list:
    """the segments k >= 1 whose seek window [base_k, base_k + W + O) and whose predecessor's cross-fade source
    [b_{k-1} + L, b_{k-1} + L + O) lie wholly inside the clip"""
    import math
    from stretch_ref import geometry
    g = geometry(sr, length, 0.0, pitch, speed)
    L = g["S"] - g["O"]
    base = [math.floor(k * g["step"]) for k in range(g["nseg"])]
    return [k for k in range(1, g["nseg"])
            if base[k] + g["W"] + g["O"] <= length and base[k - 1] + int(offs[k - 1]) + L + g["O"] <= length]


def holds_ties(sr: float, period: int, roffs):
    """so that a tie case cannot pass emptily, on the restatement's own offsets: every segment inside the clip takes an offset
    below the period (the first of its tying candidates), there are at least 4 of them and they take at least 4 values"""
    ks = segments_inside(sr, TIE_LENGTH, 0.0, TIE_SPEED, roffs)
    vals = [int(roffs[k]) for k in ks]
    assert len(ks) >= 4 and all(v < period for v in vals) and len(set(vals)) >= 4, (ks, vals)


def last_frame_source(sr: float, ch: int, pitch: float, speed: float) -> np.ndarray:
    """Silence but for two frames, placed so that the seek of segment 2 is decided by the last frame of its window that any candidate
    reads: segment 1 sees silence and stays at offset 0; the last frame of its cross-fade tail (in[base_1 + L + O - 1]) is the only
    non-zero weight of segment 2's reference; the only non-zero frame of segment 2's window is base_2 + W + O - 2, which candidate
    W - 1 alone reaches, with its last product.  So off_2 = W - 1, and 0 for a seek that misses that frame.  (The seek stages W + O
    frames; frame W + O - 1 is staged and never read: candidate o reads [o, o + O).)"""
    import math
    from stretch_ref import geometry
    g = geometry(sr, 1000, 0.0, pitch, speed)
    O, W, L = g["O"], g["W"], g["S"] - g["O"]
    b1, b2 = math.floor(g["step"]), math.floor(2 * g["step"])
    first, second = b1 + L + O - 1, b2 + W + O - 2
    assert L > W and not (b2 <= first < b2 + W + O) and first != second
    x = np.zeros((ch, max(math.ceil(3 * L * g["tau"]) + 7, first + 1 + PAD, second + 1 + PAD)), np.float32)
    x[:, first] = 7.5
    x[:, second] = 7.5
    return x


LAST_FRAME_CASES = [(204800.0, 0.0, 0.5), (48000.0, 0.0, 1.25)]     # (sr, pitch, speed): W + O = 4608, the staging's last slot; W + O = 1224


_references = {}


def reference(src_key, make, sr, gain, pitch, speed):
    """(source, restated render, restated offsets) of a case, computed once per session and shared read-only"""
    from stretch_ref import render
    key = (src_key, sr, gain, pitch, speed)
    if key not in _references:
        src = make()
        ref, offs = render(src, sr, gain, pitch, speed)
        for a in (src, ref, offs):
            a.setflags(write=False)
        _references[key] = (src, ref, offs)
    return _references[key]


def edge_reference(case):
    sr, ch, speed, pitch, gain, length, kind = case
    return reference(("edge", ch, length, kind), lambda: source(sr, ch, length, seed=length + 7 * ch, kind=kind), sr, gain, pitch, speed)


def edge_id(case) -> str:
    sr, ch, speed, pitch, gain, length, kind = case
    return f"{int(sr)}-{ch}ch-s{speed}-p{pitch}-g{gain}-n{length}-{kind}"


def dirty(syn, floats: int, rate: float = 48000.0):
    """noise over the first `floats` floats of a fresh arena, released again: what is allocated next lies on it, so that a float of an
    extent that nobody writes does not read as zero by luck"""
    x = np.random.default_rng(99).uniform(1.0, 2.0, floats - PAD).astype(np.float32)
    syn.unregister_clip(syn.register_clip(x, None, rate))


def extent_of(planar: np.ndarray) -> np.ndarray:
    """what the arena holds for a clip: its frames interleaved, then PAD zero frames"""
    ch, n = planar.shape
    out = np.zeros((n + PAD) * ch, np.float32)
    out[:n * ch] = planar.T.reshape(-1)
    return out


def source(sr: float, ch: int, length: int, seed: int, kind: str = "noise", period: int = 0) -> np.ndarray:
    """planar float32 [ch, length]: "noise" (uniform, with a 440 Hz sine under it), "zeros", "special" (noise with NaN and
    +-1e6 samples sprinkled in), "rail" (+10 or -10 by a coin: the seek's quantisation is +-32767 everywhere) or "periodic" (one
    uniform(-0.9, 0.9) block of `period` frames per channel, tiled: exactly periodic in fp32)."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((ch, length), np.float32)
    if kind == "rail":
        return np.where(rng.integers(0, 2, (ch, length)) == 1, 10.0, -10.0).astype(np.float32)
    if kind == "periodic":
        block = rng.uniform(-0.9, 0.9, (ch, period)).astype(np.float32)
        return np.ascontiguousarray(np.tile(block, (1, -(-length // period)))[:, :length])
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
