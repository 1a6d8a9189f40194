"""numpy / Python-integer restatement of the loop finder (include/zlhip.h, zlhip_sound_loop), written from the
definition and not from libzl_amd/csrc/zl_loop.h:

    request     (s0, e0, Rs, Re, W, min_length) over `length` frames, 0 <= s0 < e0 <= length; H = W / 2
    defaults    Rs, Re 0: min(2047, rint(0.010 rate)), -1: the nominal point alone; W 0: 256; min_length 0: W
    candidates  s in [max(s0 - Rs, H), min(s0 + Rs, length - H)], e likewise around e0; admissible: e - s >= min_length
    mix         m[f] = sum over the channels of clamp(rint(4096 v), +-32767), NaN -> 0
    shift       sh = max(0, bitlength(max |m| over [smin - H, smax + H) and [emin - H, emax + H)) - 10); x = m >> sh (arithmetic)
    cost        cost(s, e) = sum over j in [-H, H) of (x[s + j] - x[e + j])^2;  E(p) = sum of x[p + j]^2;  den = E(s) + E(e) + 1
    order       a before b: cost_a den_b < cost_b den_a; then the smaller |s - s0| + |e - e0|; then the smaller s; then the smaller e
    result      found, start_frame, stop_frame, shift, starts, ends, pairs, cost, den, nominal_valid, nominal_cost, nominal_den;
                nothing found: every field 0
    finish      db(c, d) = -120 where c == 0, else max(-120, 10 log10(c / d)); seam_db, nominal_db, improvement_db = nominal - seam
    items       tiles of 64 starts x 64 ends, the end tiles of one start tile neighbours: the tile's best pair and its admissible pairs
"""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

RESULT_INTS = ("found", "start_frame", "stop_frame", "shift", "starts", "ends", "nominal_valid", "pairs", "cost", "den", "nominal_cost", "nominal_den")
RESULT_DBS = ("seam_db", "nominal_db", "improvement_db")
ITEM_INTS = ("start", "stop", "cost", "den", "pairs")
TILE = 64


def resolve(rate, start_search=0, stop_search=0, window=0, min_length=0, start_frame=0, stop_frame=1):
    """the fields given as 0 filled with their defaults; None where a limit that needs no sound is broken"""
    if not (0.0 < rate < 1e9) or start_frame < 0 or stop_frame <= start_frame:
        return None
    default = int(min(2047.0, max(1.0, float(np.rint(0.010 * rate)))))
    rs = start_search or default
    re = stop_search or default
    window = window or 256
    if not (-1 <= rs <= 2047 and -1 <= re <= 2047) or window % 16 or not 16 <= window <= 1024:
        return None
    min_length = min_length or window
    if min_length < 1:
        return None
    return dict(start_search=int(rs), stop_search=int(re), window=int(window), min_length=int(min_length))


def candidates(p0, r, H, length):
    """(first candidate, how many)"""
    r = max(r, 0)
    lo, hi = max(p0 - r, H), min(p0 + r, length - H)
    return lo, max(0, hi - lo + 1)


def quantise(x):
    """clamp(rint(4096 v), +-32767) in float32 as the device does, NaN -> 0; x: float32 [channels][frames] -> int64 mono mix [frames]"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.rint(x * np.float32(4096.0))
    t = np.where(np.isnan(x), np.float32(0.0), np.clip(t, np.float32(-32767.0), np.float32(32767.0)))
    return t.astype(np.int64).sum(axis=0)


def better(a, b, s0, e0):
    """a, b: (s, e, cost, den) in Python integers, or None"""
    if a is None:
        return False
    if b is None:
        return True
    l, r = a[2] * b[3], b[2] * a[3]
    if l != r:
        return l < r
    da, db = abs(a[0] - s0) + abs(a[1] - e0), abs(b[0] - s0) + abs(b[1] - e0)
    if da != db:
        return da < db
    return (a[0], a[1]) < (b[0], b[1])


def db(cost, den):
    return -120.0 if cost == 0 else max(-120.0, 10.0 * math.log10(float(cost) / float(den)))


def cost_matrix(xs, xe, W):
    """every candidate pair's cost, int64 [ns][ne], and E per candidate.  E(s) + E(e) - 2 X with X as a float64 product of integers
    whose sums stay below 2^31, and are therefore exact"""
    A = sliding_window_view(xs, W).astype(np.float64)
    B = sliding_window_view(xe, W).astype(np.float64)
    Es, Ee = (A * A).sum(axis=1).astype(np.int64), (B * B).sum(axis=1).astype(np.int64)
    X = (A @ B.T).astype(np.int64)
    return Es[:, None] + Ee[None, :] - 2 * X, Es, Ee


def cost_direct(xs, xe, cs, ce, W):
    return int(((xs[cs:cs + W] - xe[ce:ce + W]) ** 2).sum())


def best_of(cost, den, adm, svals, evals, s0, e0):
    """the best admissible pair of a block as (s, e, cost, den) or None, and the number of admissible pairs.  The float ratio only
    prunes (its error is far below the 1e-9 kept); the order itself is decided in Python integers"""
    n = int(adm.sum())
    if n == 0:
        return None, 0
    ratio = np.where(adm, cost / den, np.inf)
    rmin = ratio.min()
    best = None
    for i, k in np.argwhere(ratio <= rmin * (1.0 + 1e-9)):
        p = (int(svals[i]), int(evals[k]), int(cost[i, k]), int(den[i, k]))
        if better(p, best, s0, e0):
            best = p
    return best, n


def loop(x, rate, s0, e0, start_search=0, stop_search=0, window=0, min_length=0, want=False):
    """the whole request over x: float32 [channels][frames] -> result dict[, item records, cost matrix]"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    length = x.shape[1]
    q = resolve(rate, start_search, stop_search, window, min_length, s0, e0)
    assert q is not None and e0 <= length
    W, H, ml = q["window"], q["window"] // 2, q["min_length"]
    smin, ns = candidates(s0, q["start_search"], H, length)
    emin, ne = candidates(e0, q["stop_search"], H, length)
    res = dict({k: 0 for k in RESULT_INTS}, **{k: 0.0 for k in RESULT_DBS})
    if ns == 0 or ne == 0:
        return (res, [], np.zeros((0, 0), np.int64)) if want else res
    ms, me = quantise(x[:, smin - H:smin + ns - 1 + H]), quantise(x[:, emin - H:emin + ne - 1 + H])
    shift = max(0, int(max(np.abs(ms).max(), np.abs(me).max())).bit_length() - 10)
    xs, xe = ms >> shift, me >> shift
    assert int(max(np.abs(xs).max(), np.abs(xe).max())) <= 1024
    cost, Es, Ee = cost_matrix(xs, xe, W)
    assert cost.min() >= 0 and cost.max() < 2 ** 32
    den = Es[:, None] + Ee[None, :] + 1
    svals, evals = smin + np.arange(ns), emin + np.arange(ne)
    adm = (evals[None, :] - svals[:, None]) >= ml
    items, best, pairs = [], None, 0
    for ts in range(0, ns, TILE):
        for te in range(0, ne, TILE):
            sl = (slice(ts, ts + TILE), slice(te, te + TILE))
            b, n = best_of(cost[sl], den[sl], adm[sl], svals[sl[0]], evals[sl[1]], s0, e0)
            items.append(dict(start=-1, stop=-1, cost=0, den=0, pairs=0) if b is None else dict(start=b[0], stop=b[1], cost=b[2], den=b[3], pairs=n))
            pairs += n
            if better(b, best, s0, e0):
                best = b
    if best is not None:
        res.update(found=1, start_frame=best[0], stop_frame=best[1], shift=shift, starts=ns, ends=ne, pairs=pairs, cost=best[2], den=best[3])
        res["seam_db"] = db(best[2], best[3])
        if smin <= s0 < smin + ns and emin <= e0 < emin + ne and e0 - s0 >= ml:
            nc = cost_direct(xs, xe, s0 - smin, e0 - emin, W)
            assert nc == int(cost[s0 - smin, e0 - emin])
            nd = int(den[s0 - smin, e0 - emin])
            res.update(nominal_valid=1, nominal_cost=nc, nominal_den=nd, nominal_db=db(nc, nd))
            res["improvement_db"] = res["nominal_db"] - res["seam_db"]
    return (res, items, cost) if want else res


# ---- the voice's two formulas (zl_plan.h: zl_clip_start / zl_clip_stop and K1's casts) ------------------------------------------------
def frame_of(start_s, rate):
    return int(float(np.float32(start_s)) * rate)


def stop_of(start_s, length_s, rate):
    return int(float(np.float32(start_s) + np.float32(length_s)) * rate)


# ---- the signals of the cases ------------------------------------------------------------------------------------------------------
def tone(period, channels=1, frames=96000, level=0.3, noise=0.0005, seed=0):
    """a three-harmonic tone of `period` frames under the envelope e^(-t / 4e6), float32 [channels][frames]"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    w = 2.0 * np.pi * t / period
    out = []
    for c in range(channels):
        y = np.sin(w + 0.3 * c) + 0.5 * np.sin(2.0 * w + 1.0) + 0.25 * np.sin(3.0 * w + 2.0 + 0.2 * c)
        y = level * (y / 1.75) * np.exp(-t / 4e6) + noise * rng.standard_normal(frames)
        out.append(y)
    return np.asarray(out, np.float32)


def square(period, frames, channels=1, level=1000):
    """an integer-valued signal of exact period `period` (in units of 1/4096, so the mix is the integers themselves)"""
    base = np.random.default_rng(period).integers(-11, 12, period) * (level // 11)
    y = np.tile(base, frames // period + 1)[:frames].astype(np.float64) / 4096.0
    return np.repeat(y[None, :], channels, 0).astype(np.float32)


# ---- the grid both tiers hold to this restatement (tests/test_loop_cpu.py: the host harness; tests/test_loop_gpu.py: the kernels) -----
SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                    0x39000000, 0x38FFFFFF, 0x39C00000, 0xB9C00000, 0x3A200000], np.uint32)
KEYS = ("start_frame", "stop_frame", "start_search", "stop_search", "window", "min_length")


def grid():
    """[(what, x float32 [channels][frames], request dict)]: candidate counts 1, 63, 64, 65 and 129 on either side, windows 16, 256 and
    1024, strips that begin at frames 1, 3 and 5, mono and stereo, full scale in both channels (shift 6), min_length cutting diagonally
    through a tile, overlapping start and end ranges, ranges clipped at both data edges, no candidates, no admissible pair, a nominal
    outside the candidates, a kept point, special float values.  Clips of at most 24000 frames"""
    cases = []
    radii = ((-1, 31), (31, 32), (32, 64), (64, -1))               # 1 x 63, 63 x 65, 65 x 129, 129 x 1 candidates
    n = 0
    for W in (16, 256, 1024):
        H = W // 2
        for k, (rs, re) in enumerate(radii):
            ch, off = 1 + (n % 2), (1, 3, 5)[n % 3]
            s0 = H + off + max(rs, 0)                              # the start strip begins at frame `off`
            e0 = s0 + 2500 + 7 * k
            x = tone(97.3 + 11.0 * k, ch, e0 + max(re, 0) + H + 3 + (n % 4), seed=n)
            cases.append((f"W{W} r{rs},{re} ch{ch} first{off}", x, dict(start_frame=s0, stop_frame=e0, start_search=rs, stop_search=re, window=W)))
            n += 1
    # 64 candidates on either side: both ranges clipped, at the data's two edges (a nominal start that is no candidate: no nominal)
    for ch in (1, 2):
        x = tone(133.7, ch, 3000 + ch, seed=20 + ch)
        L = x.shape[1]
        cases.append((f"64x64 ch{ch}", x, dict(start_frame=128 + 31, stop_frame=L - 128 - 31, start_search=32, stop_search=32, window=256)))
        cases.append((f"edges ch{ch}", x, dict(start_frame=3, stop_frame=L - 2, start_search=200, stop_search=201, window=256)))
    # full scale in both channels: |m| = 65534, sixteen bits, shift 6
    x = tone(80.0, 2, 4000, level=9.0, seed=30)
    cases.append(("full scale", x, dict(start_frame=1000, stop_frame=3000, start_search=40, stop_search=40, window=256)))
    # overlapping ranges and min_length cutting diagonally through the tiles
    x = tone(61.0, 2, 9000, seed=31)
    cases.append(("diagonal", x, dict(start_frame=5000, stop_frame=5040, start_search=64, stop_search=64, window=16, min_length=40)))
    cases.append(("diagonal default", x, dict(start_frame=5001, stop_frame=5100, start_search=70, stop_search=70, window=32)))
    # nothing to find: a clip shorter than the window, and one pair that is too short
    cases.append(("short clip", tone(50.0, 1, 200, seed=32), dict(start_frame=0, stop_frame=200, window=256)))
    cases.append(("one short pair", x, dict(start_frame=1000, stop_frame=1010, start_search=-1, stop_search=-1, window=256)))
    cases.append(("both kept", x, dict(start_frame=1001, stop_frame=4000, start_search=-1, stop_search=-1, window=1024)))
    # special float values, alone and inside a tone
    for ch in (1, 2):
        rng = np.random.default_rng(40 + ch)
        s = rng.permutation(np.tile(SPECIAL, 600))[:6000 * ch].reshape(ch, -1).view(np.float32).copy()
        s[:, 3000:] = np.where(np.arange(3000) % 3 == 0, s[:, 3000:], tone(99.0, ch, 3000, seed=41))
        cases.append((f"special ch{ch}", s, dict(start_frame=701, stop_frame=2203, start_search=33, stop_search=33, window=256)))
        cases.append((f"special tone ch{ch}", s, dict(start_frame=3501, stop_frame=5503, start_search=40, stop_search=64, window=64)))
    return cases


# ---- exact ties: the order's later rules, for both tiers -------------------------------------------------------------------------------
def tie_nominals(period):
    """the four nominal loops of the CPU tier's tie test: a whole number of periods, half a period too long, 3 too long, 5 too short"""
    return ((4000, 4000 + 50 * period), (4003, 4003 + 50 * period + period // 2), (4001, 4001 + 30 * period + 3), (4002, 4002 + 30 * period - 5))


def ties():
    """[(what, x float32 [channels][frames], request dict)] in grid()'s form: clips of 12000 frames, W = 64, in which the cost ratio
    decides nothing among hundreds of pairs, so that the result hangs on the order's later rules and on every step of the reduction
    (lane tile, wave, workgroup, items) applying them.  Integer-valued signals of exact period 16 and 100 (every pair a whole number of
    periods long costs 0), mono at shift 0 and stereo at level 11000 (shift 5); digital silence (every cost 0, den 1: the distance alone
    decides everywhere) and a constant 0.1 (cost 0 under a large den); a nominal too short for min_length (the winner is not the
    nominal); unequal radii, a start range clipped at the data's first frame and an end range clipped at its last one, which move the
    winner off the centre item.

    What the restatement gives (tests/test_loop_cpu.py asserts the conditions): zero = admissible pairs of cost 0, in = the items that
    hold one / the request's items, item and wave = where the winner lies (wave = ((stop_frame - emin) mod 64) // 16, the end tile's
    quarter a wave of the pairs workgroup owns), rule = the first rule that tells the winner from the runner-up

        case                        zero   in    item wave  rule
        square 16 n0 r70            1245   9/9     4    0   distance
        square 16 n1 r70            1242   9/9     1    0   start
        square 16 n2 r70            1242   9/9     4    0   start
        square 16 n3 r70            1242   9/9     4    0   start
        square 16 r100,104          2626  16/16    5    2   start
        square 16 r33,120           1010   8/8     1    3   start
        square 16 r140,84           2965  15/15    7    1   distance
        square 16 first frame       2475  15/15    2    0   end
        square 100 n0 r70            223   7/9     4    0   distance
        square 100 n1 r70            182   6/9     1    0   start
        square 100 n2 r70            220   8/9     4    0   start
        square 100 n3 r70            218   8/9     4    0   start
        square 100 r100,104          420  13/16    1    2   start
        square 100 r33,120           142   7/8     2    0   start
        square 100 r140,84           469  14/15    7    1   distance
        square 100 first frame       394  13/15    1    1   end
        square 16 stereo shift 5    1488   9/9     1    1   start
        silence                    19881   9/9     4    0   distance
        silence r140,84            47489  15/15    7    1   distance
        silence too short          11421   6/12    1    2   start
        silence last frame         23829   9/9     5    2   distance
        constant 0.1               28341  12/12    5    2   distance"""
    cases = []
    for period in (16, 100):
        x = square(period, 12000)
        for k, (s0, e0) in enumerate(tie_nominals(period)):
            cases.append((f"square {period} n{k} r70", x, dict(start_frame=s0, stop_frame=e0, start_search=70, stop_search=70, window=64)))
        s0, e0 = tie_nominals(period)[1]
        # unequal radii: the nominal pair lies in other tiles and other waves of them
        cases.append((f"square {period} r100,104", x, dict(start_frame=s0, stop_frame=e0, start_search=100, stop_search=104, window=64)))
        cases.append((f"square {period} r33,120", x, dict(start_frame=s0 + 1, stop_frame=e0 + 1, start_search=33, stop_search=120, window=64)))
        cases.append((f"square {period} r140,84", x, dict(start_frame=s0, stop_frame=e0 - period // 2, start_search=140, stop_search=84, window=64)))
        # the start range clipped at the data's first frame, the nominal half a period too long: the start cannot move down, and the
        # same start with the end half a period down or up is a draw down to the last rule
        cases.append((f"square {period} first frame", x, dict(start_frame=32, stop_frame=32 + 50 * period + period // 2, start_search=140, stop_search=140, window=64)))
    x = square(16, 12000, channels=2, level=11000)
    cases.append(("square 16 stereo shift 5", x, dict(start_frame=4003, stop_frame=4003 + 50 * 16 + 8, start_search=70, stop_search=84, window=64)))
    z = np.zeros((2, 12000), np.float32)
    cases.append(("silence", z, dict(start_frame=5000, stop_frame=9000, start_search=70, stop_search=70, window=64)))
    cases.append(("silence r140,84", z, dict(start_frame=5000, stop_frame=9000, start_search=140, stop_search=84, window=64)))
    cases.append(("silence too short", z, dict(start_frame=5000, stop_frame=5100, start_search=70, stop_search=110, window=64, min_length=130)))
    cases.append(("silence last frame", z, dict(start_frame=5000, stop_frame=12000, start_search=70, stop_search=200, window=64)))
    cases.append(("constant 0.1", np.full((1, 12000), 0.1, np.float32), dict(start_frame=5001, stop_frame=9003, start_search=70, stop_search=100, window=64)))
    return cases


def first_rule(a, b, s0, e0):
    """the first rule of the order that tells pair a from pair b ((s, e, cost, den) each): "cost", "distance", "start" or "end" """
    if a[2] * b[3] != b[2] * a[3]:
        return "cost"
    if abs(a[0] - s0) + abs(a[1] - e0) != abs(b[0] - s0) + abs(b[1] - e0):
        return "distance"
    return "start" if a[0] != b[0] else "end"


def tie_facts(x, rate, q):
    """what ties()'s docstring tabulates about one case, from the definition over the request's whole matrix: zero (admissible pairs of
    cost 0), zero_items (the items that hold one), items, winner and runner_up as (s, e, cost, den) -- the best admissible pair and the
    best but that one, both by better() --, item and wave (where the winner lies) and rule (what tells the two apart)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    length = x.shape[1]
    s0, e0 = q["start_frame"], q["stop_frame"]
    f = resolve(rate, *(q.get(k, 0) for k in KEYS[2:]), s0, e0)
    W, H = f["window"], f["window"] // 2
    smin, ns = candidates(s0, f["start_search"], H, length)
    emin, ne = candidates(e0, f["stop_search"], H, length)
    ms, me = quantise(x[:, smin - H:smin + ns - 1 + H]), quantise(x[:, emin - H:emin + ne - 1 + H])
    shift = max(0, int(max(np.abs(ms).max(), np.abs(me).max())).bit_length() - 10)
    cost, Es, Ee = cost_matrix(ms >> shift, me >> shift, W)
    den = Es[:, None] + Ee[None, :] + 1
    svals, evals = smin + np.arange(ns), emin + np.arange(ne)
    adm = (evals[None, :] - svals[:, None]) >= f["min_length"]
    tiles = -(-ne // TILE)
    zero = np.argwhere(adm & (cost == 0))
    win, _ = best_of(cost, den, adm, svals, evals, s0, e0)
    rest = adm.copy()
    rest[win[0] - smin, win[1] - emin] = False
    second, _ = best_of(cost, den, rest, svals, evals, s0, e0)
    return dict(zero=len(zero), zero_items=len({(i // TILE) * tiles + k // TILE for i, k in zero}), items=-(-ns // TILE) * tiles, winner=win, runner_up=second,
                item=((win[0] - smin) // TILE) * tiles + (win[1] - emin) // TILE, wave=((win[1] - emin) % TILE) // 16, rule=first_rule(win, second, s0, e0))
