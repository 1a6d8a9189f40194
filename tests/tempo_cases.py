"""The tempo estimate's tie cases, shared by the CPU tier (tests/test_tempo_cpu.py asserts every case's predicate from the restatement
alone and walks the list through the host build of the header) and the GPU tier (tests/test_tempo_edges_gpu.py runs it through the
kernels).  zl_k_tempo_pick reduces the coarse argmax per lane (lag l_min + tid + 256 k on pass k), then by wave shuffle, then over the
waves in LDS; real sound never makes two lags tie, so every case is a clip built to make lags tie EXACTLY in the order of DESIGN.md
section 13 ("equal goes to the smaller lag"), at a chosen step of that reduction.

Every sample is k / 4096 for an integer k.  A hop carries samples of one magnitude a_h, so E[h] = hop a_h^2 with hop a square: the root
is exact, R[h] = sqrt(hop) a_h.  A case is a dict:

    name     what it is
    x        planar float32 [1][frames]
    rate     the clip's sample rate
    req      (first_frame, num_frames, hop, bpm_min, bpm_max)
    pred     a predicate over the restatement's (record, W, first_lag, A): the case hits its edge
    expect   fields of the record that are asserted literally
"""
import functools
import math

import numpy as np

import tempo_ref as tr

f32 = np.float32
SR = 48000.0
THREADS, WAVE = 256, 64


def planar(k):
    k = np.atleast_2d(np.asarray(k, np.int64))
    assert int(np.abs(k).max(initial=0)) <= 32767
    return (k / 4096.0).astype(f32)


def from_hops(a, hop):
    """hop h carries +-a[h]: E[h] = hop a[h]^2"""
    assert math.isqrt(hop) ** 2 == hop
    sign = np.where(np.arange(hop) % 2 == 0, 1, -1)
    return np.concatenate([int(v) * sign for v in a])


def place(l, lmin):
    """where the pick kernel looks at lag l: (lane, wave, pass)"""
    tid, k = (l - lmin) % THREADS, (l - lmin) // THREADS
    return tid % WAVE, tid // WAVE, k


def lags_of(c):
    first, n, hop, lo, hi = c["req"]
    return tr.lags(c["rate"], hop, float(f32(lo)), float(f32(hi)), -(-n // hop))


def table(first_lag, A, a0):
    t = {0: a0}
    t.update({first_lag + i: v for i, v in enumerate(A)})
    return t


def want(c):
    """the restatement of a case: (record, W, first_lag, A)"""
    first, n, hop, lo, hi = c["req"]
    return tr.tempo(c["x"], c["rate"], first, n, hop, lo, hi)


def literal(c, rec):
    for k, v in c["expect"].items():
        assert int(rec[k]) == v, (c["name"], k, int(rec[k]), v)


def holds(c, out=None):
    rec, W, first_lag, A = want(c) if out is None else out
    assert c["pred"](rec, W, first_lag, A), (c["name"], "misses its edge", rec)
    literal(c, rec)
    return rec, W, first_lag, A


def _case(name, k, req, pred, expect, rate=SR):
    x = planar(k)
    assert req[0] + req[1] <= x.shape[1]
    return dict(name=name, x=x, rate=rate, req=req, pred=pred, expect=dict(expect))


def _constant():
    """a_h = h + 1 over 700 hops of 256: W == 16, A[l] = 256 (hops - l): every lag ties with every other"""
    hops, hop = 700, 256
    req = (0, hops * hop, hop, 75.0, 150.0)

    def pred(rec, W, first_lag, A):
        return bool((W == 16).all()) and A == [256 * (hops - first_lag - i) for i in range(len(A))] and first_lag == 74
    return [_case("constant flux: every lag ties", from_hops(np.arange(1, hops + 1), hop), req, pred,
                  dict(lag_coarse=75, lag_fine=4 * 75 - 3, doublings=2, shift=0, hops=hops))]


def _periodic(name, p, hop, hops, lo, hi, pattern, where):
    """a flux of period p (the period's last hop is silent, so hop 0's W fits the period) over a whole number of periods: exactly the
    multiples of p tie, and they are the maxima"""
    assert hops % p == 0 and len(pattern) == p and pattern[-1] == 0
    req = (0, hops * hop, hop, lo, hi)
    c = _case(name, from_hops(np.tile(pattern, hops // p), hop), req, None, {})
    lmin, lmax, cap = lags_of(c)
    mult = [l for l in range(lmin, lmax + 1) if l % p == 0]
    assert len(mult) >= 2 and lmax <= cap and where([place(l, lmin) for l in mult]), (name, lmin, lmax, cap, [place(l, lmin) for l in mult])

    def pred(rec, W, first_lag, A):
        t = table(first_lag, A, rec["acf_zero"])
        Wp = [int(v) for v in W]
        if Wp != Wp[:p] * (hops // p) or rec["shift"] != 0:
            return False
        ties = all(t[a] * (hops - mult[0]) == t[mult[0]] * (hops - a) for a in mult)
        above = all(t[mult[0]] * (hops - l) > t[l] * (hops - mult[0]) for l in range(lmin, lmax + 1) if l % p)
        return ties and above and rec["lag_coarse"] == mult[0]
    c["pred"] = pred
    c["expect"] = dict(lag_coarse=mult[0], hops=hops)
    return c


def _periodics():
    def pattern(p, at):
        a = np.zeros(p, np.int64)
        for j, v in at.items():
            a[j] = v
        return a
    return [
        _periodic("period 3: the ties in neighbouring lanes of a wave", 3, 256, 699, 75.0, 150.0, pattern(3, {0: 10, 1: 40}),
                  lambda at: {(lane, wave, k) for lane, wave, k in at} >= {(0, 0, 0), (3, 0, 0), (6, 0, 0)}),
        _periodic("period 64: the ties in one lane of all four waves", 64, 64, 704, 140.0, 400.0, pattern(64, {0: 10, 1: 40, 20: 25}),
                  lambda at: len(at) == 4 and len({lane for lane, _, _ in at}) == 1 and [wave for _, wave, _ in at] == [0, 1, 2, 3] and {k for _, _, k in at} == {0}),
        _periodic("period 256: the ties in one thread on successive passes", 256, 64, 1280, 87.0, 200.0, pattern(256, {0: 10, 1: 40, 100: 25}),
                  lambda at: len(at) == 2 and at[0][:2] == at[1][:2] and [k for _, _, k in at] == [0, 1])]


def _triple():
    """single samples in otherwise silent hops (E = a^2, R = a): the pair at distance 150 is the only lag of the coarse range with a
    product, and in the doubling's triple A[300] = 20 * 30 and A[301] = 599 * 1 over 600 and 599 terms: an exact tie, 299 has nothing"""
    hops, hop = 900, 64
    k = np.zeros(hops * hop, np.int64)
    for h, a in {0: 1000, 150: 1000, 200: 20, 500: 30, 520: 599, 821: 1}.items():
        k[h * hop + 7] = a
    req = (0, hops * hop, hop, 250.0, 400.0)

    def pred(rec, W, first_lag, A):
        t = table(first_lag, A, rec["acf_zero"])
        return (t[300], t[301], t[299]) == (600, 599, 0) and t[300] * (hops - 301) == t[301] * (hops - 300) and t[150] == 10 ** 6 and len(set(A)) > 3
    return [_case("a tie inside a doubling's triple", k, req, pred, dict(lag_coarse=150, lag_fine=300, doublings=1, acf_mid=600, acf_hi=599, acf_lo=0, hops=hops))]


@functools.lru_cache(maxsize=None)
def cases():
    out = _constant() + _periodics() + _triple()
    assert len({c["name"] for c in out}) == len(out)
    return out


def too_short():
    """requests without a lag to look at: too few hops for the range, and one hop"""
    x = planar(from_hops(np.arange(1, 91), 256))
    return [dict(name="90 hops under the default range", x=x, rate=SR, req=(0, 90 * 256, 256, 75.0, 150.0)),
            dict(name="one hop", x=x, rate=SR, req=(3, 200, 256, 75.0, 150.0))]
