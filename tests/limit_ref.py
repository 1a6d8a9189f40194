"""The peak measurement and the look-ahead limiter restated in numpy, independently of libzl_amd/csrc/zl_limit.h:
fp32 arrays, one numpy operation per operator of the definition, sums in the defined order.  The filter rows are an INPUT (tables:
{F: array [F][64]}, from zlhip_resample_design or the harness), so that libm does not enter the comparison."""
import numpy as np

f32, u32 = np.float32, np.uint32
TRUE_PEAK = 1
CHUNK, TILE, WG = 1024, 1024, 256
MAX_L, MAX_H = 512, 512
HALF, TAPS, PAD = 32, 64, 8
CEILING = f32(0.8912509381337456)
REQUEST_KEYS = ("flags", "lookahead_frames", "hold_frames", "ceiling", "gain")
RESULT_FIELDS = ("applied", "lookahead_frames", "hold_frames", "oversampling", "frames_reduced", "peak_before", "min_gain", "ceiling", "gain")


def oversampling(rate):
    return 4 if rate < 70000 else (2 if rate < 140000 else 1)


def rate_ok(rate):
    return 1000 <= rate <= 768000 and rate == int(rate) and rate * oversampling(rate) <= 768000


def resolve(rate, q):
    """the request with its defaults filled in, or None"""
    q = dict(flags=0, lookahead_frames=0, hold_frames=0, ceiling=0.0, gain=0.0) | dict(q)
    c, g = f32(q["ceiling"]), f32(q["gain"])
    if q["flags"] & ~TRUE_PEAK or (q["flags"] & TRUE_PEAK and not rate_ok(rate)):
        return None
    if not (c == 0 or (0 < c <= 1)) or not (g == 0 or (0 < g and np.isfinite(g))):
        return None
    if not (0 <= q["lookahead_frames"] <= MAX_L and 0 <= q["hold_frames"] <= MAX_H):
        return None
    if q["lookahead_frames"] == 0:
        q["lookahead_frames"] = int(min(max(np.floor(rate * 0.005 + 0.5), 1), MAX_L))
    q["ceiling"] = CEILING if c == 0 else c
    q["gain"] = f32(1) if g == 0 else g
    return q


def design(L):
    S = (L + 1) * (L + 2) * (L + 3) // 6
    return np.array([np.float64((k + 1) * (L + 1 - k)) / np.float64(S) for k in range(L + 1)], np.float64).astype(f32)


def extent_floats(n, channels):
    return ((n + PAD) * channels + 3) & ~3


def absbits(v):
    return np.ascontiguousarray(v, f32).view(u32) & u32(0x7FFFFFFF)


def inter_peaks(v, F, tables):
    """v: [channels][n] fp32, +0 assumed outside.  ips as bits [channels][n]"""
    ch, n = v.shape
    out = np.zeros((ch, n), u32)
    if F == 1:
        return out
    pad = np.zeros((ch, n + TAPS), f32)
    pad[:, HALF - 1:HALF - 1 + n] = v                                # pad index of frame f - 31 + t is f + t
    h = np.asarray(tables[F], f32)
    for p in range(1, F):
        acc = np.zeros((ch, n), f32)
        for t in range(TAPS):
            acc = acc + h[p, t] * pad[:, t:t + n]
        out = np.maximum(out, absbits(acc).reshape(ch, n))
    return out


def detector(v, F, tables):
    """p[f] as bits, and (sample bits, ips bits) per channel"""
    sp = absbits(v).reshape(v.shape)
    ips = inter_peaks(v, F, tables)
    prev = np.concatenate([np.zeros((v.shape[0], 1), u32), ips[:, :-1]], axis=1)
    return np.maximum(np.maximum(sp, ips), prev).max(axis=0), sp, ips


def peak(x, rate, first, num, flags, tables):
    """the analysis over x[:, first:first + num]: (result dict, chunk records [chunks][4] fp32)"""
    x = np.asarray(x, f32)
    F = oversampling(rate) if flags & TRUE_PEAK else 1
    v = x[:, first:first + num].copy()
    v[~np.isfinite(v)] = 0
    v = v * f32(1)
    _, sp, ips = detector(v, F, tables)
    chunks = (num + CHUNK - 1) // CHUNK
    rec = np.zeros((chunks, 4), u32)
    for k in range(chunks):
        for c in range(x.shape[0]):
            rec[k, c] = sp[c, k * CHUNK:(k + 1) * CHUNK].max()
            rec[k, 2 + c] = ips[c, k * CHUNK:(k + 1) * CHUNK].max()
    m = rec.max(axis=0)
    res = dict(sample_peak=(m[:2].view(f32)[0], m[:2].view(f32)[1]), true_peak=tuple(np.maximum(m[:2], m[2:]).view(f32)), oversampling=F, chunks=chunks)
    return res, rec.view(f32)


def limit(x, rate, q, tables):
    """x: [channels][n] finite fp32; q: a request.  (result dict, extent floats or None, finite flag, details dict)"""
    x = np.asarray(x, f32)
    ch, n = x.shape
    q = resolve(rate, q)
    L, H, c, gain = q["lookahead_frames"], q["hold_frames"], f32(q["ceiling"]), f32(q["gain"])
    F = oversampling(rate) if q["flags"] & TRUE_PEAK else 1
    with np.errstate(all="ignore"):
        v = x * gain
        pb, _, _ = detector(v, F, tables)
        p = pb.view(f32)
        hot = p > c
        g = np.where(hot, c / np.where(hot, p, f32(1)), f32(1)).astype(f32)
        r = f32(1) - g
        res = dict(applied=0, lookahead_frames=L, hold_frames=H, oversampling=F, frames_reduced=0, peak_before=pb.max().view(f32), min_gain=f32(1), ceiling=c, gain=gain)
        if gain == 1 and not (pb.max() > c.view(u32)):
            return res, None, True, dict(hot=hot, G=np.ones(n, f32), v=v)
        # mr[i], i in [-L, n - 1]: index i + L
        rp = np.concatenate([np.zeros(L + H, f32), r, np.zeros(L, f32)])         # rp index of frame j is j + L + H
        mr = np.lib.stride_tricks.sliding_window_view(rp, L + H + 1).max(axis=1)  # window of i starts at frame i - H: rp index i + L
        assert mr.size == n + L
        w = design(L)
        R = np.zeros(n, f32)
        for k in range(L + 1):
            R = R + w[k] * mr[L - k:L - k + n]
        G = np.maximum(f32(1) - R, f32(0)).astype(f32)
        y = v * G[None, :]
        out = np.where(y > c, c, np.where(y < -c, -c, y)).astype(f32)
    res.update(applied=1, frames_reduced=int((G < 1).sum()), min_gain=G.min())
    ext = np.zeros(extent_floats(n, ch), f32)
    ext[:n * ch] = out.T.reshape(-1)
    return res, ext, bool(np.isfinite(out).all()), dict(hot=hot, G=G, v=v, y=y, out=out, w=w)
