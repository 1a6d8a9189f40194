"""numpy restatement of the waveform overview (include/zlhip.h, zlhip_sound_overview), written from the definition:

    column c covers [lo, hi): lo = first + floor(c * n / columns), hi = first + floor((c + 1) * n / columns); hi == lo -> [lo, lo + 1)
    samples are ordered by an integer key of their 32 bits (a negative value: all bits flipped; a non-negative one: the sign bit
    flipped), minimum and maximum are taken over the keys and mapped back
    per column (minL, maxL, minR, maxR); a mono sound repeats its channel
"""
import numpy as np


def bounds(first, n, columns):
    """(lo, hi) int64 arrays of the columns' frame ranges"""
    c = np.arange(columns, dtype=np.int64)
    lo = first + (c * n) // columns
    hi = first + ((c + 1) * n) // columns
    return lo, np.where(hi == lo, lo + 1, hi)


def key(bits):
    """uint32 sample bits -> sortable uint32 keys"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)


def overview(planar, columns, first=0, n=None, loop=False):
    """planar: float32 [channels][length] -> float32 [columns][4], bit-exact (compare as uint32).  loop=True: column by column
    over [lo, hi), the definition word for word; otherwise the same with reduceat (columns <= n: the columns tile the request, column
    c ends where c + 1 begins) or a gather (columns > n: every column is the one frame lo)."""
    planar = np.ascontiguousarray(planar, np.float32)
    ch, length = planar.shape
    n = length - first if n is None else n
    assert 1 <= columns and first >= 0 and n >= 1 and first + n <= length
    lo, hi = bounds(first, n, columns)
    out = np.zeros((columns, 4), np.uint32)
    for c_ in range(2):
        k = key(planar[min(c_, ch - 1)].view(np.uint32))
        if loop:
            for c in range(columns):
                seg = k[lo[c]:hi[c]]
                out[c, 2 * c_] = seg.min()
                out[c, 2 * c_ + 1] = seg.max()
        elif columns <= n:
            out[:, 2 * c_] = np.minimum.reduceat(k[:first + n], lo)
            out[:, 2 * c_ + 1] = np.maximum.reduceat(k[:first + n], lo)
        else:
            out[:, 2 * c_] = out[:, 2 * c_ + 1] = k[lo]
    return unkey(out).view(np.float32)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
