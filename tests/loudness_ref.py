"""An independent numpy restatement of the loudness measurement (libzl_amd/csrc/zl_loudness.h): ITU-R BS.1770-4 /
EBU R 128 integrated loudness over sub-blocks that are each filtered from zero state one sub-block early.  It walks FRAMES (the
product walks 16-byte groups), a Python loop over the steps, vectorised across the sub-blocks and the channels; every operator is
one IEEE double operation (numpy does not contract), so the sums equal the product's bit for bit when both use the same ten
coefficients -- measure(..., coeffs=...) takes the library's (zlhip_loudness_design), so that a libm difference in tan / pow cannot
enter a comparison made with ==."""
import math

import numpy as np

GATE_ABS = 1.1724653045822981e-07          # 10^((-70 + 0.691) / 10)
SUB_MIN, SUB_MAX, MAX_ITEMS, MAX_CALL_ITEMS = 16, 131072, 65536, 1048576

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): the shelf's b0 b1 b2 a1 a2, the high-pass's a1 a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)


def design(rate):
    """the ten coefficients: shelf b0 b1 b2 a1 a2, high-pass 1 -2 1 a1 a2"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def default_sub(rate):
    return int(math.floor(rate * 0.1 + 0.5))


def items_of(num, sub):
    S = num // sub
    return S if S >= 4 else -(-num // sub)


def resolve(rate, first, num, sub):
    """the resolved sub_frames, or None where the request is outside the limits that need no sound"""
    if first < 0 or num < 1:
        return None
    if sub == 0:
        sub = default_sub(rate)
    if not (SUB_MIN <= sub <= SUB_MAX) or items_of(num, sub) > MAX_ITEMS:
        return None
    return sub


def batch(requests):
    """requests: (src, rate, first, num, sub, coeffs) each, src planar [channels, frames] float32, num None = to the end, coeffs None =
    design(rate) -> per request (sums [items, 2] float64, peaks [items, 2] float32, sub).  One loop over the steps for all of them."""
    W, S0, S1, LEN, OFF, CO, count, subs = [], [], [], [], [], [], [], []
    xs, total = [], 0
    for src, rate, first, num, sub, coeffs in requests:
        src = np.asarray(src, np.float32)
        ch, length = src.shape
        num = length - first if num is None else num
        sub = resolve(rate, first, num, sub)
        assert sub is not None and first + num <= length
        n = items_of(num, sub)
        k = np.arange(n)
        s0 = first + k * sub                                       # the item's own frames [s0, s1), the peak's [s0, pe), the walk's [w, pe)
        s1 = np.minimum(s0 + sub, first + num)
        w = np.where(k > 0, s0 - sub, s0)
        pe = s1.copy()
        pe[-1] = first + num
        two = np.zeros((2, length), np.float32)                    # a mono sound: a second channel of zeros gives sum[1] = peak[1] = 0
        two[:ch] = src
        xs.append(two)
        W.append(w); S0.append(s0); S1.append(s1); LEN.append(pe - w); OFF.append(np.full(n, total)); count.append(n); subs.append(sub)
        CO.append(np.tile(np.array(design(rate) if coeffs is None else list(coeffs), np.float64)[:, None], (1, n)))
        total += length
    raw = np.concatenate(xs, 1)
    finite = np.isfinite(raw)
    x = np.where(finite, raw, np.float32(0)).astype(np.float64)    # (double)v, a non-finite sample is 0
    mag = np.where(finite, np.abs(raw), np.float32(0))
    w, s0, s1, lens, off = (np.concatenate(v) for v in (W, S0, S1, LEN, OFF))
    order = np.argsort(-lens, kind="stable")                       # the longest walks first: the items still walking at step t are a prefix
    w, s0, s1, lens, off = (v[order] for v in (w, s0, s1, lens, off))
    c = np.concatenate(CO, 1)[:, order, None]                      # [10, items, 1]
    n = w.size
    st = np.zeros((4, n, 2))
    sums = np.zeros((n, 2))
    peaks = np.zeros((n, 2), np.float32)
    for t in range(int(lens[0])):
        m = int(np.searchsorted(-lens, -t, side="left"))           # items with lens > t
        f = off[:m] + w[:m] + t
        v = x[:, f].T                                              # [m, 2]
        own = w[:m] + t >= s0[:m]
        peaks[:m] = np.where(own[:, None], np.maximum(peaks[:m], mag[:, f].T), peaks[:m])
        y = c[0, :m] * v + st[0, :m]
        n0 = (c[1, :m] * v - c[3, :m] * y) + st[1, :m]
        n1 = c[2, :m] * v - c[4, :m] * y
        z = c[5, :m] * y + st[2, :m]
        n2 = (c[6, :m] * y - c[8, :m] * z) + st[3, :m]
        n3 = c[7, :m] * y - c[9, :m] * z
        st[0, :m] = n0; st[1, :m] = n1; st[2, :m] = n2; st[3, :m] = n3
        sums[:m] = np.where((own & (w[:m] + t < s1[:m]))[:, None], sums[:m] + z * z, sums[:m])
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    sums, peaks = sums[back], peaks[back]
    out, at = [], 0
    for m, sub in zip(count, subs):
        out.append((sums[at:at + m], peaks[at:at + m], sub))
        at += m
    return out


def sub_blocks(src, rate, first=0, num=None, sub=0, coeffs=None):
    """the records: (sums [items, 2] float64, peaks [items, 2] float32, sub).  src: planar [channels, frames] float32"""
    return batch([(src, rate, first, num, sub, coeffs)])[0]


def measure_batch(requests):
    """batch(), finished: per request (result, sums, peaks)"""
    res = []
    for (src, rate, first, num, sub, coeffs), (sums, peaks, rsub) in zip(requests, batch(requests)):
        num = np.asarray(src).shape[1] - first if num is None else num
        res.append((finish(sums, peaks, num, rsub), sums, peaks))
    return res


def finish(sums, peaks, num, sub):
    """zlhip_loudness's fields from the records (Python floats, in index order)"""
    S, n = num // sub, items_of(num, sub)
    u = [float(sums[k, 0]) + float(sums[k, 1]) for k in range(n)]
    if S >= 4:
        z = [(((u[j] + u[j + 1]) + u[j + 2]) + u[j + 3]) / float(4 * sub) for j in range(S - 3)]
    else:
        t = 0.0
        for v in u:
            t += v
        z = [t / float(num)]
    res = dict(lufs=-math.inf, mean_square=0.0, relative_gate=0.0, peak=(float(peaks[:, 0].max()), float(peaks[:, 1].max())), sub_blocks=n, blocks=len(z),
               above_absolute=0, above_relative=0)
    total, A = 0.0, 0
    for v in z:
        if v > GATE_ABS:
            total += v
            A += 1
    if A:
        rel = (total / float(A)) / 10.0
        tot, B = 0.0, 0
        for v in z:
            if v > GATE_ABS and v > rel:
                tot += v
                B += 1
        ms = tot / float(B)
        res.update(lufs=-0.691 + 10.0 * math.log10(ms), mean_square=ms, relative_gate=rel, above_absolute=A, above_relative=B)
    return res


def measure(src, rate, first=0, num=None, sub=0, coeffs=None):
    """(result, sums, peaks)"""
    src = np.asarray(src, np.float32)
    num = src.shape[1] - first if num is None else num
    sums, peaks, sub = sub_blocks(src, rate, first, num, sub, coeffs)
    return finish(sums, peaks, num, sub), sums, peaks


def same(got, want, tol=1e-9):
    """a result dict against the restatement's: integers, peaks, mean_square and relative_gate with ==, lufs within tol (two log10s)"""
    if any(int(got[k]) != int(want[k]) for k in ("sub_blocks", "blocks", "above_absolute", "above_relative")):
        return False
    if tuple(np.float32(v) for v in got["peak"]) != tuple(np.float32(v) for v in want["peak"]):
        return False
    if got["mean_square"] != want["mean_square"] or got["relative_gate"] != want["relative_gate"]:
        return False
    if math.isinf(want["lufs"]):
        return got["lufs"] == want["lufs"]
    return abs(got["lufs"] - want["lufs"]) <= tol
