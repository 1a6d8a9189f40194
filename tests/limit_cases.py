"""The case grid of the peak measurement and the limiter: the smallest shapes at which the kernels can still go
wrong.  A case is dict(tag, x [channels][n] fp32, rate, q request fields); tests/test_limit_cpu.py asserts from the restatement alone
that every case hits the edge it is aimed at, tests/test_limit_gpu.py runs the grid in one call."""
import numpy as np

import limit_ref as lr

f32 = np.float32
C = lr.CEILING
TILE = lr.TILE


def quiet(ch, n, seed, amp=0.3):
    return (np.random.default_rng(seed).uniform(-amp, amp, (ch, n))).astype(f32)


def case(tag, x, q=None, rate=48000.0):
    return dict(tag=tag, x=np.ascontiguousarray(x, f32), rate=float(rate), q=dict(q or {}))


def sine45(n, amp=1.0, ch=1):
    """fs/4 sampled at 45 degrees: every sample is +-amp / sqrt(2), the peak between the samples is amp"""
    t = np.arange(n)
    s = (amp * np.sin(2 * np.pi * t / 4 + np.pi / 4)).astype(f32)
    return np.stack([s] * ch)


def grid():
    g = []
    seed = [100]

    def noise(ch, n):
        seed[0] += 1
        return quiet(ch, n, seed[0])

    # the identity first: a clip under the ceiling
    g.append(case("identity", noise(2, 700)))
    # lengths, mono and stereo, a hot frame at frame 0 and at the last frame
    for ch in (1, 2):
        for n in (1, 2, 240, 241, 1023, 1024, 1025, 3 * TILE + 5):
            x = noise(ch, n)
            x[0, 0] = 1.0
            x[ch - 1, n - 1] = -1.25
            g.append(case("length", x))
    # look-ahead and hold at their limits; hot at a tile's last frame (= a chunk's last) or at the next one's first
    k = 0
    for L in (1, 2, 0, 512):
        for H in (0, 1, 512):
            x = noise(1 + k % 2, 3 * TILE + 5)
            at = TILE - 1 if k % 2 == 0 else TILE
            x[0, at] = 1.5
            g.append(case("tile edge, last frame" if at == TILE - 1 else "tile edge, first frame", x, dict(lookahead_frames=L, hold_frames=H)))
            k += 1
    # a quiet tile within L before, and within L + H behind, a hot frame of the neighbour tile
    x = noise(2, 3 * TILE); x[1, TILE + 100] = 1.1
    g.append(case("quiet tile before", x, dict(lookahead_frames=240)))
    x = noise(2, 3 * TILE); x[0, TILE - 300] = 1.1
    g.append(case("quiet tile behind", x, dict(lookahead_frames=100, hold_frames=400)))
    # the right channel only
    x = noise(2, 900); x[1, 450] = -1.0
    g.append(case("right channel only", x))
    # exactly at the ceiling (not hot: the identity) and one ulp above
    x = noise(1, 600); x[0, 300] = C
    g.append(case("at the ceiling", x))
    x = noise(1, 600); x[0, 300] = np.nextafter(C, f32(2))
    g.append(case("one ulp above", x))
    x = noise(1, 600); x[0, 300] = -np.nextafter(C, f32(2))
    g.append(case("one ulp above", x))
    # two hot frames within reach of each other, different g
    x = noise(2, 1500); x[0, 500] = 1.0; x[1, 600] = 1.5
    g.append(case("two hot frames", x, dict(lookahead_frames=240)))
    # a hot stretch longer than 2 L + H: a plateau of constant G
    x = noise(1, 1200); x[0, 400:520] = 1.2
    g.append(case("plateau", x, dict(lookahead_frames=16, hold_frames=8)))
    # gain: a cold clip made hot; nothing hot
    g.append(case("gain makes it hot", quiet(2, 2100, 7, 0.5), dict(gain=2.0)))
    g.append(case("gain, nothing hot", quiet(2, 2100, 8, 0.5), dict(gain=0.5)))
    # overflow: v is infinite
    x = noise(1, 800); x[0, 400] = 3e38
    g.append(case("overflow", x, dict(gain=4.0)))
    # true peak: a hot sample at each factor
    for rate in (48000.0, 96000.0, 192000.0):
        x = noise(2, 2 * TILE + 77); x[0, 1100] = 1.3
        g.append(case("true peak, hot sample", x, dict(flags=lr.TRUE_PEAK, lookahead_frames=64), rate))
    # fs/4 at 45 degrees: hot with the flag only
    for ch in (1, 2):
        g.append(case("sine45, flag", sine45(2 * TILE + 300, 1.0, ch), dict(flags=lr.TRUE_PEAK, lookahead_frames=32)))
        g.append(case("sine45, no flag", sine45(2 * TILE + 300, 1.0, ch), dict(lookahead_frames=32)))
    x = sine45(2 * TILE + 300, 1.0, 1)
    g.append(case("sine45, flag", x, dict(flags=lr.TRUE_PEAK), 96000.0))
    # an inter-sample peak in the first and in the last 32 frames: the taps outside the region are +0
    x = np.zeros((1, 1500), f32); x[0, :24] = sine45(24)[0]
    g.append(case("inter-sample peak at the start", x, dict(flags=lr.TRUE_PEAK, lookahead_frames=8)))
    x = np.zeros((2, 1500), f32); x[1, -24:] = sine45(24)[0]
    g.append(case("inter-sample peak at the end", x, dict(flags=lr.TRUE_PEAK, lookahead_frames=8)))
    # an inter-sample peak between a chunk's last frame and the next one's first: the frame behind is hot through ips[f - 1]
    x = np.zeros((1, 2 * TILE), f32); x[0, TILE - 12:TILE + 12] = sine45(24)[0]
    g.append(case("inter-sample peak at a chunk edge", x, dict(flags=lr.TRUE_PEAK, lookahead_frames=4)))
    # the identity last
    g.append(case("identity", noise(1, 1)))
    return g


def peak_cases():
    """the analysis: (x, rate, first_frame, num_frames, flags) -- regions from frame 0, from an odd frame, of one frame at the end, ending at and one
    behind a chunk's edge; non-finite samples (+0 to the analysis) and samples whose filtered sum overflows"""
    rng = np.random.default_rng(5)
    x1 = rng.uniform(-1, 1, (2, 3 * lr.CHUNK + 17)).astype(f32)
    x1[0, 100] = np.nan; x1[1, 2050] = np.inf; x1[1, 5] = -np.inf
    x2 = sine45(2 * lr.CHUNK + 3, 0.9, 1)
    x3 = rng.uniform(-1, 1, (1, 40)).astype(f32)
    x3[0, 10] = 1e38; x3[0, 11] = -1e38
    out = []
    for x, rate in ((x1, 48000.0), (x2, 44100.0), (x2, 96000.0), (x2, 192000.0), (x3, 48000.0)):
        n = x.shape[1]
        for first, num in ((0, n), (1, n - 1), (7, min(n - 7, lr.CHUNK)), (n - 1, 1), (3, min(n - 3, lr.CHUNK + 1))):
            for flags in (0, lr.TRUE_PEAK):
                out.append((x, rate, first, num, flags))
    return out
