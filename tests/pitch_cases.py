"""The pitch detection's edge cases, shared by the CPU tier (tests/test_pitch_cpu.py asserts every case's predicate from the restatement
alone and walks the list through the host build of the header) and the GPU tier (tests/test_pitch_edges_gpu.py runs it through the
kernels).  The pick and vote kernels can only be reached through clips, so every case is a clip built to put one decision of DESIGN.md
section 14 on its edge: the threshold at equality, a plateau under the descent, a descent that ends at t_max, t0 and the stop in
neighbouring lanes and waves of the pick kernel, a valley outside [t_min, t_max], the gate at equality, every shift at both sides of
its limit, the lower median at an even count and on the lane and wave boundaries of the vote's histogram scan, the edge of the
consistent band, clarity ties within and across waves, 256 frames, and the geometries the grid leaves out.

Every sample is k / 4096 for an integer k, so the quantisation is exact and equalities are exact.  A case is a dict:

    name     what it is
    x        planar float32 [channels][frames]
    rate     the clip's sample rate
    req      zlhip_pitch_request's fields but the sound
    pred     a predicate over the restatement's (result, frame records, d per frame): the case hits its edge
    expect   fields of the result that are asserted literally
    flags    the frames' flags, asserted literally (None: not stated)
    shift    (the shift cases) the one frame's shift, asserted literally
"""
import functools

import numpy as np

import pitch_ref as pr

f32 = np.float32
SR = 48000.0


def fmin_for(rate, tmax):
    """an f_min whose floor(rate / f_min) is tmax"""
    f = float(f32(rate / (tmax + 0.5)))
    assert pr.lags(rate, f, rate / 4)[1] == tmax
    return f


def fmax_for(rate, tmin):
    """an f_max whose ceil(rate / f_max) is tmin (t_min >= 3: f_max stays below rate / 2)"""
    f = float(f32(rate / (tmin - 0.5)))
    assert tmin >= 3 and pr.lags(rate, 20.0, f)[0] == tmin
    return f


def planar(k):
    """integers [channels][frames] or [frames] -> the float32 clip k / 4096, exactly"""
    k = np.atleast_2d(np.asarray(k, np.int64))
    assert int(np.abs(k).max(initial=0)) <= 32767
    x = (k / 4096.0).astype(f32)
    assert np.array_equal(pr.quantise(x), k.sum(axis=0))
    return x


def sine(n, period, amp=3000, phase=0.0):
    return np.rint(amp * np.sin(2.0 * np.pi * np.arange(n) / period + phase)).astype(np.int64)


def train(n, period, amp=1000, phase=0):
    k = np.zeros(n, np.int64)
    k[phase::period] = amp
    return k


def cum(d):
    """C[t] at C[t], C[0] = 0"""
    C = [0]
    for v in d:
        C.append(C[-1] + v)
    return C


def geometry(c):
    """(t_min, t_max, W, L, K, hop, threshold, gate) of a case"""
    r = c["req"]
    n = r.get("num_frames", c["x"].shape[1] - r.get("first_frame", 0))
    q = pr.resolve(c["rate"], n, *(r.get(k, 0) for k in ("window", "max_frames", "f_min", "f_max", "threshold", "gate")), r.get("first_frame", 0))
    tmin, tmax = pr.lags(c["rate"], q["f_min"], q["f_max"])
    K, hop = pr.frames_of(n, q["window"], tmax, q["max_frames"])
    return tmin, tmax, q["window"], q["window"] + tmax + 1, K, hop, q["threshold"], q["gate"]


def energies(c):
    """the gate's sums of a case's frames"""
    tmin, tmax, W, L, K, hop, _, _ = geometry(c)
    first = c["req"].get("first_frame", 0)
    m = pr.quantise(c["x"])
    return [int((m[first + k * hop:first + k * hop + W] ** 2).sum()) for k in range(K)]


def want(c):
    """the restatement of a case: (result, frame records, d per frame)"""
    r = c["req"]
    return pr.pitch(c["x"], c["rate"], r.get("first_frame", 0), r.get("num_frames"), *(r.get(k, 0) for k in ("window", "max_frames", "f_min", "f_max", "threshold", "gate")),
                    want_d=True)


def holds(c, out=None):
    """the case hits its edge and gives its named outcome, by the restatement (or by `out`, the same triple from somewhere else)"""
    res, recs, ds = want(c) if out is None else out
    assert c["pred"](res, recs, ds), (c["name"], "misses its edge", res)
    literal(c, res, recs)
    return res, recs, ds


def literal(c, res, recs):
    """the named outcomes, whoever computed res and recs"""
    for k, v in c["expect"].items():
        assert int(res[k]) == v, (c["name"], k, int(res[k]), v)
    if "shift" in c:
        assert [int(r["shift"]) for r in recs] == [c["shift"]], (c["name"], recs)
    if c["flags"] is not None:
        assert [int(r["flag"]) for r in recs] == list(c["flags"]), (c["name"], [int(r["flag"]) for r in recs])


def _case(name, k, req, pred, expect=None, flags=None, rate=SR):
    return dict(name=name, x=planar(k), rate=rate, req=req, pred=pred, expect=dict(expect or {}), flags=flags)


# ---- the pick kernel's decisions ------------------------------------------------------------------------------------------------------
def _threshold_equality():
    """an impulse train of period P with W a multiple of P: d is flat off the multiples of P, so d[t] t 1024 == 1024 C[t] for every
    t < P: equality is not below, and the lag is P"""
    P, W, tmax = 64, 512, 255
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, threshold=1024, max_frames=1)

    def pred(res, recs, ds):
        d, C = ds[0], cum(ds[0])
        return all(d[t - 1] * t * 1024 == 1024 * C[t] and d[t - 1] > 0 for t in range(1, P)) and 24 < P and d[P - 1] == 0 and recs[0]["lag"] == P
    return [_case("threshold at equality", train(W + tmax + 1, P), req, pred, dict(lag=P, voiced=1), [pr.VOICED])]


def _plateau():
    """a train whose gaps alternate P, P + 1: half the impulses meet at lag P and the other half at P + 1.  Searched for a frame whose
    picked lag has d[lag + 1] == d[lag] > 0 (at most 2 * 28 * 81 frames of 512 samples)"""
    tmax = 255
    for W in (256, 320):
        for P in range(12, 40):
            for phase in range(2 * P + 1):
                k = np.zeros(W + tmax + 1, np.int64)
                pos, i = phase, 0
                while pos < len(k):
                    k[pos] = 1000
                    pos += P + (i & 1)
                    i += 1
                req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, threshold=1024, max_frames=1)
                res, recs, ds = pr.pitch(planar(k), SR, **req, want_d=True)
                lag = recs[0]["lag"]
                if lag > 0 and lag < tmax and ds[0][lag] == ds[0][lag - 1] > 0:
                    def pred(res, recs, ds, lag=lag):
                        return recs[0]["lag"] == lag and ds[0][lag] == ds[0][lag - 1] > 0
                    return [_case("plateau under the descent (W %d, P %d, phase %d)" % (W, P, phase), k, req, pred, dict(lag=lag), [pr.VOICED])]
    raise AssertionError("no plateau found")


def _descent_to_tmax():
    """a sine of period t_max + 4: d still falls at t_max, where the descent has to stop"""
    tmax, W = 300, 512
    out = []
    for thr in (154, 1024):
        req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, threshold=thr, max_frames=1)

        def pred(res, recs, ds):
            return recs[0]["lag"] == tmax and ds[0][tmax] < ds[0][tmax - 1]
        out.append(_case("descent ends at t_max (threshold %d)" % thr, sine(W + tmax + 1, tmax + 4), req, pred, dict(lag=tmax), [pr.VOICED]))
    return out


def _t0_at_tmin():
    """a sine of period P with t_min = P - 1 and threshold 1024: t0 = t_min (d is far below its mean there) and the descent stops one
    lag later, at d[P] = 0.  A lane of the pick kernel owns the lags 8 i + 1 .. 8 i + 8 and a wave 512 of them"""
    out = []
    for where, P, W, tmax in (("neighbouring lanes", 97, 256, 255), ("neighbouring waves", 513, 576, 520), ("one lane", 98, 256, 255)):
        tmin = P - 1
        req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=fmax_for(SR, tmin), threshold=1024, max_frames=1)
        lane = lambda t: (t - 1) // 8
        assert {"neighbouring lanes": lane(tmin) + 1 == lane(P) and lane(tmin) // 64 == lane(P) // 64, "neighbouring waves": lane(tmin) == 63 and lane(P) == 64,
                "one lane": lane(tmin) == lane(P)}[where]

        def pred(res, recs, ds, tmin=tmin, P=P):
            d, C = ds[0], cum(ds[0])
            return d[tmin - 1] * tmin * 1024 < 1024 * C[tmin] and d[tmin] < d[tmin - 1] and d[P] >= d[P - 1] and recs[0]["lag"] == P
        out.append(_case("t0 == t_min, t0 and the stop in %s" % where, sine(W + tmax + 1, P), req, pred, dict(lag=P), [pr.VOICED]))
    return out


def _unvoiced():
    W, tmax = 256, 255
    L = W + tmax + 1
    out = []
    for thr in (154, 1024):
        req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, threshold=thr, max_frames=1)

        def pred(res, recs, ds):
            d = ds[0]
            return d[tmax] == 0 and min(d[:tmax]) > 0 and recs[0]["flag"] == pr.UNVOICED
        out.append(_case("unvoiced: the only zero of d is at t_max + 1 (threshold %d)" % thr, train(L, tmax + 1), req, pred, dict(lag=0, voiced=0), [pr.UNVOICED]))
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=fmax_for(SR, 129), threshold=1024, max_frames=1)

    def pred(res, recs, ds):
        d = ds[0]
        return d[127] == 0 and min(d[128:tmax]) > 0 and d[tmax] == 0 and recs[0]["flag"] == pr.UNVOICED
    out.append(_case("unvoiced: the valley is at t_min - 1 and its multiple at t_max + 1", train(L, 128), req, pred, dict(lag=0, voiced=0), [pr.UNVOICED]))
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, max_frames=1)
    out.append(_case("unvoiced: DC", np.full(L, 1000), req, lambda res, recs, ds: not any(ds[0]) and recs[0]["flag"] == pr.UNVOICED, dict(lag=0, voiced=0), [pr.UNVOICED]))
    for c in out:                                                  # not silent: the energy is above the floor
        assert energies(c)[0] >= W * 8 * 8, c["name"]
    return out


def _gate():
    """the energy exactly at W channels gate^2 is not silent; one unit less is"""
    W, tmax, g = 256, 255, 8
    L = W + tmax + 1
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, gate=g, max_frames=1)
    sq = np.where(np.arange(L) % 64 < 32, g, -g)
    st = np.stack([np.full(L, g), sq])                             # half the frames (g, g), half (g, -g)
    out = []
    for name, k, ch in (("mono", sq, 1), ("stereo", st, 2)):
        floor = W * ch * g * g
        c = _case("gate at equality, " + name, k, req, lambda res, recs, ds: recs[0]["flag"] == pr.VOICED, dict(lag=64, voiced=1), [pr.VOICED])
        assert energies(c) == [floor], (name, energies(c))
        out.append(c)
        k = np.atleast_2d(k).copy()
        k[0, 5] = g - 1
        c = _case("gate one below, " + name, k, req, lambda res, recs, ds: recs[0]["flag"] == pr.SILENT, dict(lag=0, voiced=0), [pr.SILENT])
        assert floor - 4 * g * g <= energies(c)[0] < floor, (name, energies(c))
        out.append(c)
    return out


def _shifts():
    """max |m| at both sides of every limit of the shift, in the window, only in the lagged tail and at the span's last sample; the
    samples around it are a tone with odd negative values, which an arithmetic shift and a division round differently"""
    W, tmax = 256, 255
    L = W + tmax + 1
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, max_frames=1)
    base = sine(L, 50, 1001)
    assert ((base < 0) & (base & 1 == 1)).any()
    out, i = [], 0
    for M in (4095, 4096, 8191, 8192, 16383, 16384, 32767, 32768):
        sh = max(0, M.bit_length() - 12)
        for where, pos in (("in the window", 100), ("in the lagged tail", W + 100), ("at the last sample", L - 1)):
            for sign in ((1, -1) if where == "at the last sample" or M >= 32767 else (1,)):
                ch = 2 if (M == 32768 or i % 2) else 1
                i += 1
                k = np.zeros((ch, L), np.int64)
                k[0] = base
                if ch == 2:
                    k[0, pos], k[1, pos] = sign * (M // 2), sign * (M - M // 2)
                else:
                    k[0, pos] = sign * M

                def pred(res, recs, ds, k=k, sh=sh, M=M, pos=pos):
                    m = k.sum(axis=0)
                    return int(np.abs(m).max()) == M == abs(int(m[pos])) and int(np.abs(np.delete(m, pos)).max()) < 4096 and recs[0]["shift"] == sh
                out.append(_case("shift %d: max |m| = %s%d %s, %s" % (sh, "-" if sign < 0 else "", M, where, ("mono", "stereo")[ch - 1]), k, req, pred, None, None))
                out[-1]["shift"] = sh
    return out


# ---- the vote kernel's decisions ------------------------------------------------------------------------------------------------------
def _framed(contents, W=256, tmax=255, hop=600, **more):
    """disjoint frames: max_frames = K and num_frames chosen so that the hop is `hop` >= L; contents[k] fills frame k's span"""
    K, L = len(contents), W + tmax + 1
    assert hop >= L and K >= 2
    n = L + hop * (K - 1)
    k = np.zeros(n, np.int64)
    for i, c in enumerate(contents):
        k[i * hop:i * hop + len(c)] = c
    req = dict(dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0, max_frames=K, num_frames=n), **more)
    assert pr.frames_of(n, W, tmax, K) == (K, hop)
    return k, req


def _noisy(L, period, seed, noise=40):
    return sine(L, period) + np.random.default_rng(seed).integers(-noise, noise + 1, L)


def _votes():
    L = 512
    out = []

    def add(name, contents, pred, expect, flags=None, **more):
        k, req = _framed(contents, **more)
        out.append(_case(name, k, req, pred, expect, flags))

    lagsof = lambda recs: [r["lag"] for r in recs]
    add("vote: the lower median of an even count, a clarity tie two frames apart", [sine(L, p) for p in (200, 100, 200, 100)],
        lambda res, recs, ds: lagsof(recs) == [200, 100, 200, 100] and recs[1]["clarity"] == recs[3]["clarity"],
        dict(frames=4, voiced=4, consistent=2, frame=1, lag=100))
    add("vote: the edge of the consistent band (med >> 5 == 3)", [sine(L, p) for p in (100, 103, 104, 97, 100)],
        lambda res, recs, ds: lagsof(recs) == [100, 103, 104, 97, 100] and recs[1]["clarity"] > max(recs[k]["clarity"] for k in (0, 3, 4)),
        dict(frames=5, voiced=5, consistent=4, frame=1, lag=103))
    add("vote: silent frames do not vote", [np.zeros(L, np.int64), sine(L, 150), np.zeros(L, np.int64), sine(L, 100)],
        lambda res, recs, ds: lagsof(recs) == [0, 150, 0, 100], dict(frames=4, voiced=2, consistent=1, frame=3, lag=100),
        [pr.SILENT, pr.VOICED, pr.SILENT, pr.VOICED])
    add("vote: 256 frames, a lane each", [sine(L, 100 + (k & 1)) for k in range(256)],
        lambda res, recs, ds: lagsof(recs) == [100, 101] * 128 and len({r["clarity"] for r in recs[0::2]}) == 1 and len({r["clarity"] for r in recs[1::2]}) == 1
        and recs[1]["clarity"] > recs[0]["clarity"], dict(frames=256, voiced=256, consistent=256, frame=1, lag=101))
    contents = [_noisy(L, 100, k) for k in range(201)]
    contents[70] = contents[200] = sine(L, 100)
    add("vote: a clarity tie between frames in different waves", contents,
        lambda res, recs, ds: set(lagsof(recs)) == {100} and recs[70]["clarity"] == recs[200]["clarity"] > max(r["clarity"] for k, r in enumerate(recs) if k not in (70, 200)),
        dict(frames=201, voiced=201, consistent=201, frame=70, lag=100))
    contents = [_noisy(L, 100, 300 + k) for k in range(8)]
    contents[5] = contents[6] = sine(L, 100)
    add("vote: a clarity tie between neighbouring frames", contents,
        lambda res, recs, ds: set(lagsof(recs)) == {100} and recs[5]["clarity"] == recs[6]["clarity"] > max(r["clarity"] for k, r in enumerate(recs) if k not in (5, 6)),
        dict(frames=8, voiced=8, consistent=8, frame=5, lag=100))
    # a lane of the vote kernel scans the bins 8 i .. 8 i + 7 and a wave 512 of them: medians at both sides of a lane's and a wave's edge
    short = dict(f_max=fmax_for(SR, 5))
    for periods, med, cons, rep in (((7, 8, 8), 8, 2, 1), ((7, 7, 8), 7, 2, 0)):
        add("vote: the median in bin %d (the scan's lanes 0 | 1), med >> 5 == 0" % med, [sine(L, p) for p in periods],
            lambda res, recs, ds, periods=periods: lagsof(recs) == list(periods), dict(frames=3, voiced=3, consistent=cons, frame=rep, lag=med), **short)
    # 527 is consistent with a median of 512 (15 <= 512 >> 5) and not with one of 511 (16 > 511 >> 5)
    wide = dict(W=576, tmax=530, hop=1110)
    for periods, med, cons in (((512, 527, 511, 512), 512, 4), ((511, 527, 512, 511), 511, 3)):
        add("vote: the median in bin %d (the scan's waves 0 | 1)" % med, [sine(576 + 531, p) for p in periods],
            lambda res, recs, ds, periods=periods: lagsof(recs) == list(periods) and res["lag"] in periods,
            dict(frames=4, voiced=4, consistent=cons), **wide)
    for periods, med, cons, rep in (((31, 32, 31), 31, 2, 0), ((32, 33, 32), 32, 3, None)):
        add("vote: the band opens at a median of 32 (median %d)" % med, [sine(L, p) for p in periods],
            lambda res, recs, ds, periods=periods: lagsof(recs) == list(periods), dict(dict(frames=3, voiced=3, consistent=cons), **({} if rep is None else dict(frame=rep, lag=med))))
    return out


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def _geometry():
    """mono first frames 2, 6 and 3, stereo 1 and 2; t_max + 1 of 255, 256 and 257 under a window of 320, 256 under a window of 256, 521
    under a window of 576; two frames, the request ending with the second frame's span, so that the span's end falls on every residue
    of a 16-byte group; a full-scale frame in front of the request and one behind it (a float read from there changes the shift)"""
    out, ends = [], {1: set(), 2: set()}
    for ch, firsts in ((1, (2, 6, 3)), (2, (1, 2))):
        for first in firsts:
            for W, nd in ((320, 255), (320, 256), (320, 257), (256, 256), (576, 521)):
                if W != 320 and first != firsts[0]:
                    continue
                L = W + nd
                n = L + W
                k = np.zeros((ch, first + n + 3), np.int64)
                t = np.arange(first + n + 3)
                for c in range(ch):
                    k[c] = np.rint(2000 * np.sin(2 * np.pi * t / 97 + 0.4 * c) + 800 * np.sin(4 * np.pi * t / 97 + 1.0))
                k[:, first - 1] = 28672
                k[:, first + n] = -28672
                ends[ch].add((first + n) * ch % 4)
                req = dict(window=W, f_min=fmin_for(SR, nd - 1), f_max=2000.0, first_frame=first, num_frames=n, max_frames=2)
                out.append(_case("geometry: %s, first frame %d, window %d, t_max + 1 = %d" % (("mono", "stereo")[ch - 1], first, W, nd), k, req,
                                 lambda res, recs, ds: len(recs) == 2 and all(r["shift"] <= 1 for r in recs), dict(frames=2, lag=97, consistent=2)))
    assert ends == {1: {0, 1, 2, 3}, 2: {0, 2}}, ends
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _threshold_equality() + _plateau() + _descent_to_tmax() + _t0_at_tmin() + _unvoiced() + _gate() + _shifts() + _votes() + _geometry()
    assert len({c["name"] for c in out}) == len(out)
    return out


def too_short():
    """requests without a frame: one sample less than a span, a mono and a stereo clip"""
    W, tmax = 256, 255
    req = dict(window=W, f_min=fmin_for(SR, tmax), f_max=2000.0)
    return [dict(name="too short, mono", x=planar(sine(W + tmax, 100)), rate=SR, req=req),
            dict(name="too short, stereo", x=planar(np.stack([sine(300, 64), sine(300, 64)])), rate=SR, req=dict(req, first_frame=1, num_frames=298))]
