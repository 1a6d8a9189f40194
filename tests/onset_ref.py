"""numpy / Python-integer restatement of the transient detection (include/zlhip.h, zlhip_sound_onsets), written
from the definition and not from libzl_amd/csrc/zl_onset.h:

    q = clamp(rint(4096 v), +-32767), NaN -> 0;  e[f] = sum over the channels of q^2
    E[h] = sum of e over hop h (hop frames from `first` on, the last hop cut at the request's end), E[-1] = 0
    F = hop * channels * gate^2;  L(x) = 64 p + floor((x - 2^p) * 64 / 2^p), p = floor(log2 x)
    N[h] = max(0, L(E[h] + F) - L(E[h-1] + F))
    candidate: N[h] >= threshold, N[h] > N[j] for j in [h - min_gap, h), N[h] >= N[j] for j in (h, h + min_gap]
    select: the max_onsets largest N, equal N to the smaller h
    refine: S = hop / 16, sub-blocks from max(first, first + (h-1) hop) up to first + (h+1) hop, cut to the request's end; the start of
            the first one with 4 e_s > E[h-1] + F, else first + h hop
"""
from fractions import Fraction

import numpy as np


def resolve(sample_rate, hop=0, gate=0, threshold=0, min_gap=0, max_onsets=0):
    """the fields given as 0 filled with their defaults; None where a limit is broken"""
    sr = Fraction(sample_rate)
    if hop == 0:
        hop = 16 * min(256, max(4, round(sr / 3000)))              # (round: half to even, exact on a Fraction)
    if hop % 16 or not 64 <= hop <= 4096:
        return None
    gate = gate or 8
    threshold = threshold or 128
    if min_gap == 0:
        min_gap = max(1, -((-sr / 20) // hop))                     # ceil(0.05 sample_rate / hop)
    max_onsets = max_onsets or 128
    if not (1 <= gate <= 32767 and 1 <= threshold <= 4096 and 1 <= min_gap <= 1024 and 1 <= max_onsets <= 1024):
        return None
    return dict(hop=int(hop), gate=int(gate), threshold=int(threshold), min_gap=int(min_gap), max_onsets=int(max_onsets))


def quantise(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        t = np.rint(x * np.float32(4096.0))
        t = np.where(np.isnan(t), np.float32(0.0), np.clip(t, -32767.0, 32767.0))
    return t.astype(np.int64)


def level(x):
    x = int(x)
    assert x >= 1
    p = x.bit_length() - 1
    return 64 * p + ((x - (1 << p)) * 64) // (1 << p)


def frame_energy(planar):
    q = quantise(planar)
    return (q * q).sum(axis=0)


def energy(planar, first, n, hop):
    """E as uint64 [hops]"""
    e = frame_energy(planar)[first:first + n]
    return np.add.reduceat(e, np.arange(0, n, hop)).astype(np.uint64)


def novelty(E, F):
    lv = [level(int(v) + F) for v in E]
    prev = [level(F)] + lv[:-1]
    return np.array([max(0, a - b) for a, b in zip(lv, prev)], np.int32)


def candidates(N, threshold, min_gap):
    hops = len(N)
    out = []
    for h in np.flatnonzero(N >= threshold):
        h = int(h)
        before = N[max(0, h - min_gap):h]
        after = N[h + 1:min(hops, h + min_gap + 1)]
        if (before.size == 0 or N[h] > before.max()) and (after.size == 0 or N[h] >= after.max()):
            out.append(h)
    return out


def select(N, cand, max_onsets):
    return sorted(sorted(cand, key=lambda h: (-int(N[h]), h))[:max_onsets])


def refine(e, E, F, first, n, hop, h):
    """e: the energy of every frame of the sound"""
    S = hop // 16
    ep = (int(E[h - 1]) if h > 0 else 0) + F
    a = max(first, first + (h - 1) * hop)
    end = first + n
    while a < first + (h + 1) * hop and a < end:
        if 4 * int(e[a:min(a + S, end)].sum()) > ep:
            return a
        a += S
    return first + h * hop


def onsets(planar, first=0, n=None, hop=256, gate=8, threshold=128, min_gap=10, max_onsets=128):
    """planar: float32 [channels][length] -> (onsets int32 [count][2] (frame, strength), E uint64 [hops], N int32 [hops])"""
    planar = np.ascontiguousarray(planar, np.float32)
    ch, length = planar.shape
    n = length - first if n is None else n
    assert first >= 0 and n >= 1 and first + n <= length
    e = frame_energy(planar)
    E = energy(planar, first, n, hop)
    F = hop * ch * gate * gate
    N = novelty(E, F)
    kept = select(N, candidates(N, threshold, min_gap), max_onsets)
    out = np.array([(refine(e, E, F, first, n, hop, h), int(N[h])) for h in kept], np.int32).reshape(-1, 2)
    return out, E, N
