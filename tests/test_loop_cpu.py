"""Loop finder, CPU tier: what the definition does to sound and how it breaks ties, with the numpy / Python-integer restatement
(tests/loop_ref.py) alone; the host build of libzl_amd/csrc/zl_loop.h (tests/cpu_harness/loop_host.cpp walks a call the way the kernels
do, item by item and lane tile by lane tile, with the header's own arithmetic) against the restatement on every cost of the matrix,
every item record and every integer of the result, the three dB fields within 1e-9 (two log10 implementations, each good to an ulp of a
value below 12, times 10: six orders below that); the defaults, the limits and the struct layouts; the frames-to-seconds inverse; the new
kernels' resources; the walk under the sanitizers (tests/cpp/loop_check.cpp).  tests/test_loop_gpu.py holds the kernels themselves to the
restatement on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_ref as lr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
FORMS = {"diff": 0, "dot": 1}

_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_loop_harness())
        l.zllp_resolve.restype = C.c_int32
        l.zllp_resolve.argtypes = [C.c_double] + [C.POINTER(C.c_int32)] * 4
        l.zllp_sizes.argtypes = [C.c_void_p]
        l.zllp_seconds.restype = C.c_int32
        l.zllp_seconds.argtypes = [C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        l.zllp_better.restype = C.c_int32
        l.zllp_better.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        l.zllp_call.restype = C.c_int64
        l.zllp_call.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int32]
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


# ---- (a) what the definition does to sound (the restatement alone) ------------------------------------------------------------------
PERIODS = (218.4, 100.0, 733.3)
NOMINALS = ((24000, 72057), (30011, 80000))
_measured = {}


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("period", PERIODS)
def test_tones_loop_on_a_whole_number_of_periods(period, channels):
    """Three-harmonic tones under a slow decay with a little noise: wherever the two search ranges together reach over a period
    (4 R >= period) the found loop is a whole number of periods long within 0.02 period and its seam lies at least 20 dB below the
    nominal loop's.  Measured with this restatement over all the cases: 0.0019 period at worst, seam_db -37.6 .. -44.3 against nominal_db
    -12.0 .. +2.2, the smallest improvement 28.8 dB (the bars leave room for other noise draws).  Where the ranges are shorter than that
    (period 733.3 at R = 64) only a valid pair is asked for."""
    x = lr.tone(period, channels, seed=int(period) + channels)
    for s0, e0 in NOMINALS:
        for R in (64, 480):
            r = lr.loop(x, SR, s0, e0, R, R, 256)
            assert r["found"] == 1 and abs(r["start_frame"] - s0) <= R and abs(r["stop_frame"] - e0) <= R and r["stop_frame"] - r["start_frame"] >= 256
            assert r["starts"] == r["ends"] == 2 * R + 1 and r["pairs"] == (2 * R + 1) ** 2 and r["nominal_valid"] == 1
            n = (r["stop_frame"] - r["start_frame"]) / period
            print(f"period {period} ch {channels} nominal ({s0}, {e0}) R {R}: length {n:.4f} periods, seam {r['seam_db']:.1f} dB, nominal {r['nominal_db']:.1f} dB, "
                  f"improvement {r['improvement_db']:.1f} dB")
            if 4 * R < period:
                continue
            _measured[(period, channels, s0, R)] = (abs(n - round(n)), r["improvement_db"])
            assert abs(n - round(n)) <= 0.02, (period, channels, s0, R, n)
            assert r["improvement_db"] >= 20.0, (period, channels, s0, R, r)
    print("worst so far: %.4f period, %.1f dB" % (max(v[0] for v in _measured.values()), min(v[1] for v in _measured.values())))


# ---- (b) exact ties -----------------------------------------------------------------------------------------------------------------
def nearest_zero(period, s0, e0):
    """where the order sends a nominal loop on a signal of exact period with both ranges reaching a period either way: the nearest
    zero -- shorten by off or lengthen by period - off, whichever is less; among the ways to spread that over the two points the smallest
    s wins: the start moves down as far as the distance lets it, or the stop moves down while the start stays"""
    off = (e0 - s0) % period                                       # the nominal loop is `off` frames longer than a whole number of periods
    down, up = off, period - off
    if off == 0:
        return (s0, e0)
    if down < up:
        return (s0, e0 - down)                                     # s stays (moving it up would be a larger s), e comes down
    return (s0 - up, e0)                                           # lengthen (or a draw between the two): the smallest s is s0 - up with e at e0


@pytest.mark.parametrize("period", [16, 100])
def test_exact_ties_go_to_the_nearest_pair_then_the_smaller_start_then_the_smaller_end(period):
    """An integer-valued signal of exact period: every pair whose length is a whole number of periods costs 0, so the order's later rules
    decide -- the smallest |s - s0| + |e - e0|, then the smallest s, then the smallest e"""
    x = lr.square(period, 12000)
    for s0, e0, R in [(s0, e0, 70) for s0, e0 in lr.tie_nominals(period)] + [(4000, 4000 + 50 * period + 1, -1)]:
        r, items, cost = lr.loop(x, SR, s0, e0, R, R, 64, want=True)
        off = (e0 - s0) % period                                   # the nominal loop is `off` frames longer than a whole number of periods
        assert r["found"] == 1 and r["shift"] == 0
        if R < 0:
            assert (r["start_frame"], r["stop_frame"]) == (s0, e0) and (r["cost"] == 0) == (off == 0)
            continue
        assert r["cost"] == 0 and r["seam_db"] == -120.0 and (r["stop_frame"] - r["start_frame"]) % period == 0
        want = nearest_zero(period, s0, e0)
        assert (r["start_frame"], r["stop_frame"]) == want, (period, s0, e0, r)
        zeros = int((cost == 0).sum())
        assert zeros >= (2 * R + 1) ** 2 // period - 2 * R - 1     # (ties everywhere: a rule that looked at the cost alone would not get here)
    # the order itself, against the header's: cross-multiplied costs beyond 2^53, then distance, then s, then e
    rng = np.random.default_rng(period)
    pool = [(100 + int(rng.integers(0, 5)), 300 + int(rng.integers(0, 5)), int(rng.integers(0, 3)) * (2 ** 31 - 1) + int(rng.integers(0, 2)), int(rng.integers(1, 3)) * 2 ** 30 + 1)
            for _ in range(60)]
    for a in pool:
        for b in pool:
            pa, pb = np.array(a, np.int64), np.array(b, np.int64)
            assert bool(lib().zllp_better(pa.ctypes.data, pb.ctypes.data, 102, 302)) == lr.better(a, b, 102, 302), (a, b)
            assert a[:2] == b[:2] or lr.better(a, b, 102, 302) != lr.better(b, a, 102, 302)       # total over different pairs


# ---- (c) the harness against the restatement ----------------------------------------------------------------------------------------
def arena(x):
    """float32 [channels][frames] -> the arena's layout, padded with zeros to a whole 16-byte group"""
    flat = np.ascontiguousarray(np.asarray(x, np.float32).T).reshape(-1)
    return np.concatenate([flat, np.zeros(-len(flat) % 4, np.float32)])


def same_result(got, want, what):
    assert {k: int(getattr(got, k)) for k in lr.RESULT_INTS} == {k: int(want[k]) for k in lr.RESULT_INTS}, (what, want)
    for k in lr.RESULT_DBS:
        assert abs(float(getattr(got, k)) - float(want[k])) <= 1e-9, (what, k, getattr(got, k), want[k])


def call(requests, form):
    """requests: (x float32 [channels][frames], rate, dict of zlhip_loop_request's fields but id).  Runs the harness walk over the whole call
    and holds every cost, every item record and every result to the restatement; returns (result, items, geometry) per request"""
    n = len(requests)
    reqs = (_abi.LoopRequest * n)()
    datas, refs = [], []
    for i, (x, rate, f) in enumerate(requests):
        x = np.atleast_2d(np.asarray(x, np.float32))
        reqs[i] = _abi.LoopRequest(0, *(f.get(k, 0) for k in lr.KEYS))
        datas.append(arena(x))
        refs.append(lr.loop(x, rate, *(f.get(k, 0) for k in lr.KEYS), want=True))
    data = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    length = np.array([np.atleast_2d(r[0]).shape[1] for r in requests], np.int32)
    channels = np.array([np.atleast_2d(r[0]).shape[0] for r in requests], np.int32)
    rate = np.array([r[1] for r in requests], np.float64)
    words = sum(c.size for _, _, c in refs)
    nitems = sum(len(it) for _, it, _ in refs)
    costs = np.full(words + 1, 0xDEADBEEF, np.uint32)
    items = (_abi.LoopItem * (nitems + 1))()
    C.memset(items, 0x5A, C.sizeof(items))
    geom = np.zeros((n, 8), np.int32)
    cbase = np.zeros(n, np.int64)
    out = (_abi.Loop * n)()
    sizes = np.zeros(3, np.int32)
    lib().zllp_sizes(sizes.ctypes.data)
    assert list(sizes) == [C.sizeof(_abi.Loop), C.sizeof(_abi.LoopItem), 72] and C.sizeof(_abi.Loop) == 80 and C.sizeof(_abi.LoopItem) == 24
    touched = [np.zeros(len(d), np.uint8) for d in datas]
    tptr = (C.c_void_p * n)(*[t.ctypes.data for t in touched])
    walk = np.zeros(4, np.int64)
    used = lib().zllp_call(n, C.addressof(reqs), C.addressof(data), length.ctypes.data, channels.ctypes.data, rate.ctypes.data, costs.ctypes.data, words,
                           C.addressof(items), nitems, geom.ctypes.data, cbase.ctypes.data, C.addressof(out), C.addressof(tptr), walk.ctypes.data, form)
    assert used == words and int(costs[words]) == 0xDEADBEEF and bytes(items[nitems]) == b"\x5a" * 24
    terms, results, ib = 0, [], 0
    for i, (res, its, cost) in enumerate(refs):
        smin, ns, emin, ne, W, ml, nit, item_base = (int(v) for v in geom[i])
        f = requests[i][2]
        q = lr.resolve(float(rate[i]), *(f.get(k, 0) for k in lr.KEYS[2:]))
        assert W == q["window"] and ml == q["min_length"] and (ns, ne) == cost.shape and nit == len(its) == -(-ns // 64) * -(-ne // 64) and item_base == ib
        if ns:
            assert (smin, ns) == lr.candidates(f["start_frame"], q["start_search"], W // 2, int(length[i])) and (emin, ne) == lr.candidates(f["stop_frame"], q["stop_search"], W // 2, int(length[i]))
        got = costs[cbase[i]:cbase[i] + ns * ne].reshape(ns, ne).astype(np.int64)
        assert np.array_equal(got, cost), (i, "cost", np.argwhere(got != cost)[:4])
        for k in range(nit):
            assert {name: int(getattr(items[ib + k], name)) for name in lr.ITEM_INTS} == its[k], (i, k, its[k])
        same_result(out[i], res, (i, f))
        # every float of the two strips is used (by the strip that holds it), and nothing else of the sound is
        want = np.zeros(len(datas[i]), np.uint8)
        ch, H = int(channels[i]), W // 2
        if ns:
            want[(smin - H) * ch:(smin + ns - 1 + H) * ch] |= 1
            want[(emin - H) * ch:(emin + ne - 1 + H) * ch] |= 2
        assert np.array_equal(touched[i], want), (i, "a float of a strip is not read, or one outside is")
        terms += ns * ne * W
        results.append((res, its, dict(smin=smin, ns=ns, emin=emin, ne=ne, window=W, items=nit)))
        ib += nit
    assert [int(v) for v in walk] == [terms, 0, 0, 0], walk
    return results


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_grid_equals_the_restatement(form):
    cases = lr.grid()
    out = call([(x, SR, q) for _, x, q in cases], FORMS[form])
    by = {what: (res, g) for (what, _, _), (res, _, g) in zip(cases, out)}
    counts = {(g["ns"], g["ne"]) for _, g in by.values()}
    assert {(1, 63), (63, 65), (65, 129), (129, 1), (64, 64), (1, 1), (0, 0)} <= counts, counts
    assert by["full scale"][0]["shift"] == 6 and by["special ch2"][0]["shift"] == 6 and by["W256 r-1,31 ch1 first3"][0]["shift"] <= 1
    assert by["short clip"][0]["found"] == 0 and by["one short pair"][0]["found"] == 0 and by["one short pair"][1]["ns"] == 1
    assert by["edges ch1"][0]["found"] == 1 and by["edges ch1"][0]["nominal_valid"] == 0 and by["edges ch1"][0]["improvement_db"] == 0.0
    assert by["edges ch2"][1]["smin"] == 128 and by["edges ch2"][1]["emin"] + by["edges ch2"][1]["ne"] - 1 == 3002 - 128       # clipped at both edges
    d = by["diagonal"][0]
    assert 0 < d["pairs"] < d["starts"] * d["ends"] and d["stop_frame"] - d["start_frame"] >= 40       # min_length cuts the tiles
    assert by["both kept"][0]["pairs"] == 1 and by["both kept"][0]["improvement_db"] == 0.0
    assert all(res["nominal_valid"] == 1 for what, (res, _) in by.items() if what.startswith("W"))


def test_the_tie_cases_tie_where_they_are_meant_to():
    """lr.ties() from the restatement alone, before anything runs on a device: every square and silence case has at least 100
    admissible pairs of cost 0 in at least 6 of its items; over the list the winner lies in at least 4 different item indices and in
    all four waves of the pairs workgroup; each later rule -- distance, smaller start, smaller end -- decides at least one result"""
    cases = lr.ties()
    facts = {what: lr.tie_facts(x, SR, q) for what, x, q in cases}
    assert len(facts) == len(cases)
    for what, x, q in cases:
        f = facts[what]
        print(f"{what:26s} zero {f['zero']:5d} in {f['zero_items']:2d}/{f['items']:<2d} item {f['item']:2d} wave {f['wave']} rule {f['rule']}")
        assert x.shape[1] <= 12000 and q["window"] == 64
        res = lr.loop(x, SR, *(q.get(k, 0) for k in lr.KEYS))
        assert (res["start_frame"], res["stop_frame"], res["cost"], res["den"]) == f["winner"] and res["cost"] == 0
        assert lr.better(f["winner"], f["runner_up"], q["start_frame"], q["stop_frame"]) and f["runner_up"][2] == 0 and f["rule"] != "cost"
        if what.startswith(("square", "silence")):
            assert f["zero"] >= 100 and f["zero_items"] >= 6, (what, f)
    assert len({f["item"] for f in facts.values()}) >= 4, sorted({f["item"] for f in facts.values()})
    assert {f["wave"] for f in facts.values()} == {0, 1, 2, 3}
    assert {f["rule"] for f in facts.values()} == {"distance", "start", "end"}
    assert facts["silence too short"]["winner"][:2] != (5000, 5100) and facts["square 16 stereo shift 5"]["winner"][3] < facts["square 16 n1 r70"]["winner"][3]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_ties_equal_the_restatement(form):
    """lr.ties() through the harness walk in one call: every cost, every item record and every result, as for the grid; the four
    symmetric nominals of either period land where the closed form says"""
    cases = lr.ties()
    out = call([(x, SR, q) for _, x, q in cases], FORMS[form])
    by = {what: res for (what, _, _), (res, _, _) in zip(cases, out)}
    for period in (16, 100):
        for k, (s0, e0) in enumerate(lr.tie_nominals(period)):
            res = by[f"square {period} n{k} r70"]
            assert (res["start_frame"], res["stop_frame"]) == nearest_zero(period, s0, e0) and res["pairs"] == 141 * 141 and res["shift"] == 0
    assert by["square 16 stereo shift 5"]["shift"] == 5 and by["silence"]["den"] == 1 and by["constant 0.1"]["den"] > 1 << 20
    assert all(res["found"] == 1 and res["cost"] == 0 and res["seam_db"] == -120.0 for res in by.values())
    assert by["silence too short"]["nominal_valid"] == 0 and by["silence last frame"]["nominal_valid"] == 0


def test_a_call_with_empty_requests_between_the_others():
    x = lr.tone(77.0, 2, 5000, seed=3)
    short = lr.tone(50.0, 1, 100, seed=4)
    f = dict(start_frame=1000, stop_frame=3001, start_search=40, stop_search=33, window=64)
    out = call([(short, SR, dict(start_frame=0, stop_frame=100)), (x, SR, f), (short, 44100.0, dict(start_frame=3, stop_frame=90, window=128)), (x, 44100.0, dict(f, window=32)),
                (short, SR, dict(start_frame=10, stop_frame=20, window=16, start_search=-1, stop_search=-1))], FORMS["dot"])
    assert [res["found"] for res, _, _ in out] == [0, 1, 0, 1, 0] and [g["items"] for _, _, g in out] == [0, 4, 0, 4, 1]


# ---- (d) defaults, limits, layouts --------------------------------------------------------------------------------------------------
def resolve(sr, start_frame=100, stop_frame=5000, **f):
    """zlhip_loop_resolve and the harness's zl_lp_resolve, held to each other and to the restatement; the resolved fields or None"""
    r = _abi.LoopRequest(0, start_frame, stop_frame, *(f.get(k, 0) for k in lr.KEYS[2:]))
    before = bytes(r)
    rc = zlhip().zlhip_loop_resolve(sr, C.byref(r))
    v = [C.c_int32(f.get(k, 0)) for k in lr.KEYS[2:]]
    hrc = lib().zllp_resolve(sr, *(C.byref(x) for x in v))
    want = lr.resolve(sr, *(f.get(k, 0) for k in lr.KEYS[2:]), start_frame, stop_frame)
    if want is None:
        assert rc == _abi.ZLHIP_ERR_INVALID and bytes(r) == before, f
        return None
    got = {k: getattr(r, k) for k in lr.KEYS[2:]}
    assert rc == 0 and hrc == 0 and got == want == {k: x.value for k, x in zip(lr.KEYS[2:], v)}, (f, got, want)
    return got


def test_defaults():
    assert resolve(48000.0) == dict(start_search=480, stop_search=480, window=256, min_length=256)
    assert resolve(44100.0) == dict(start_search=441, stop_search=441, window=256, min_length=256)
    assert resolve(22050.0)["start_search"] == 220 and resolve(96000.0)["start_search"] == 960          # rint: 220.5 to even
    assert resolve(384000.0)["start_search"] == 2047                                                   # the default stays inside the limit
    assert resolve(48000.0, window=64) == dict(start_search=480, stop_search=480, window=64, min_length=64)
    assert resolve(48000.0, start_search=-1, stop_search=7, min_length=1) == dict(start_search=-1, stop_search=7, window=256, min_length=1)


def test_every_limit_either_side():
    ok = dict(start_search=2047, stop_search=2047, window=1024, min_length=1)
    assert resolve(48000.0, **ok) == ok
    assert resolve(48000.0, **dict(ok, window=16)) is not None
    for bad in (dict(start_search=2048), dict(stop_search=2048), dict(start_search=-2), dict(stop_search=-2), dict(window=1040), dict(window=8), dict(window=24),
                dict(window=-16), dict(min_length=-1)):
        assert resolve(48000.0, **dict(ok, **bad)) is None, bad
    assert resolve(0.0, **ok) is None and resolve(float("nan"), **ok) is None and resolve(1e9, **ok) is None
    assert resolve(48000.0, start_frame=-1, **ok) is None and resolve(48000.0, start_frame=5000, stop_frame=5000, **ok) is None
    assert resolve(48000.0, start_frame=4999, stop_frame=5000, **ok) == ok
    assert zlhip().zlhip_loop_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = _abi.LoopRequest(0, 100, 5000, 0, 0, 0, 0)
    out = (_abi.Loop * 1)()
    C.memset(out, 0x5A, C.sizeof(out))
    n = C.c_int32(-7)
    assert z.zlhip_sound_loop(None, C.byref(r), out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_loop_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_loop_items(None, 0, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_loop_costs(None, 0, None, 0, C.byref(n), C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_loop_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_loop_batch(None, C.byref(r), 1, out) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * 80 and n.value == -7
    lz = C.CDLL(build.build_engine())
    for name, args in (("libzl_hotpath_clip_find_loop", [C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 4), ("libzl_hotpath_clip_snap_loop", [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
                       ("libzl_hotpath_clips_snap_loops", [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p])):
        getattr(lz, name).restype = C.c_int
        getattr(lz, name).argtypes = args
    assert lz.libzl_hotpath_clip_find_loop(None, 0.0, 0, C.byref(n), None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clip_snap_loop(None, 0.0, 0.0, C.byref(n), None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clips_snap_loops(None, 2, 0.0, 0.0, None) == _abi.ZLHIP_ERR_INVALID and n.value == -7


def test_loop_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_loop_request", _abi.LoopRequest), ("zlhip_loop", _abi.Loop), ("zlhip_loop_item", _abi.LoopItem))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:3] == [28, 80, 24]
    assert got[3:] == list(range(0, 28, 4)) + list(range(0, 32, 4)) + [32, 40, 44, 48, 52, 56, 64, 72] + [0, 4, 8, 12, 16]


# ---- (e) frames to seconds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [22050.0, 44100.0, 48000.0, 96000.0])
def test_seconds_round_trip_through_the_voices_formulas(rate):
    """random (start, stop) up to 2^22 frames: the float seconds map back to exactly these frames through the voice's two formulas,
    restated here in numpy float32 / Python float"""
    rng = np.random.default_rng(int(rate))
    z = zlhip()
    a, l = C.c_float(0.0), C.c_float(0.0)
    for top in (1 << 12, 1 << 17, 1 << 22):
        for _ in range(700):
            start = int(rng.integers(0, top - 1))
            stop = int(rng.integers(start + 1, top + 1))
            assert lib().zllp_seconds(rate, start, stop, C.byref(a), C.byref(l)) == 0, (rate, start, stop)
            assert lr.frame_of(a.value, rate) == start and lr.stop_of(a.value, l.value, rate) == stop, (rate, start, stop, a.value, l.value)
    assert z.zlhip_loop_seconds(rate, 30011, 80000, C.byref(a), C.byref(l)) == 0 and lr.frame_of(a.value, rate) == 30011 and lr.stop_of(a.value, l.value, rate) == 80000


def test_seconds_beyond_a_floats_reach_are_refused():
    z = zlhip()
    a, l = C.c_float(-1.0), C.c_float(-2.0)
    rng = np.random.default_rng(5)
    fails = 0
    for _ in range(400):                                           # around 2^30 frames a float of seconds steps over thousands of frames
        start = int(rng.integers(1 << 29, 1 << 30))
        rc = lib().zllp_seconds(48000.0, start, start + 48000, C.byref(a), C.byref(l))
        assert rc in (0, -1)
        if rc == 0:
            assert lr.frame_of(a.value, 48000.0) == start and lr.stop_of(a.value, l.value, 48000.0) == start + 48000
        fails += rc != 0
    assert fails >= 300, fails                                     # (a frame is hit by chance about once in 47 / 8)
    a, l = C.c_float(-1.0), C.c_float(-2.0)
    assert z.zlhip_loop_seconds(48000.0, (1 << 30) + 1, (1 << 30) + 48001, C.byref(a), C.byref(l)) == _abi.ZLHIP_ERR_INVALID and (a.value, l.value) == (-1.0, -2.0)
    for bad in ((0.0, 0, 10), (48000.0, -1, 10), (48000.0, 10, 10), (float("nan"), 0, 10)):
        assert z.zlhip_loop_seconds(*bad, C.byref(a), C.byref(l)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_loop_seconds(48000.0, 0, 10, None, C.byref(l)) == _abi.ZLHIP_ERR_INVALID


# ---- (f) the kernels' resources -----------------------------------------------------------------------------------------------------
def test_loop_kernels_resources(built):
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_loop_kernel_resources.txt")
    assert os.path.exists(path), "no zl_loop kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    prep = [r for n, r in rows.items() if "zl_k_loop_prep" in n]
    pairs = [r for n, r in rows.items() if "zl_k_loop_pairs" in n]
    pick = [r for n, r in rows.items() if "zl_k_loop_pick" in n]
    assert len(prep) == 1 and len(pairs) == 1 and len(pick) == 1 and len(rows) == 3, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    # two staged strip tiles of 64 + 1024 int16, four pairs and four words for the reductions
    for r in pairs:
        assert r["lds"] == 2 * 2 * (64 + 1024) + 4 * 16 + 4 * 8, rows
        assert r["vgprs"] <= 64 and r["waves"] >= 8, rows
    assert prep[0]["lds"] == 32 and pick[0]["lds"] == 4 * 16 + 4 * 8, rows


# ---- (g) the walk under the sanitizers ----------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/loop_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with AddressSanitizer
    and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment loads
    in front of it."""
    exe = str(tmp_path / "loop_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_check.cpp"), "-o", exe])
    for args in (["1", "12"], ["2", "12"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "loop check ok" in rc.stdout
