"""Warp, CPU tier: the host build of libzl_amd/csrc/zl_warp.h (tests/cpu_harness/warp_host.cpp walks a call the way the kernels do, the
seek region by region and the synthesis workgroup by workgroup, with the header's own arithmetic) against the numpy / Python-integer
restatement (tests/warp_ref.py) with == on every float of every extent, every seek offset and every result field, every float of an
extent written exactly once and no read outside the buffer the harness was given; the resolve at every limit from both sides; the plan
against its restatement; what the definition does to sound, on the restatement alone; the library's host-only calls, the struct
layouts, the new kernels' resources; the walk under the sanitizers (tests/cpp/warp_check.cpp).  tests/test_warp_gpu.py holds the
kernels themselves to the restatement on the GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import warp_cases as wc
import warp_ref as wr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
PA = C.POINTER(_abi.WarpAnchor)

_h = None
_z = None


def harness():
    global _h
    if _h is None:
        l = C.CDLL(build.build_warp_harness())
        l.zlwp_resolve.restype = C.c_int
        l.zlwp_resolve.argtypes = [C.c_double, C.c_int32, PA, C.c_int32, C.POINTER(_abi.Warp)]
        l.zlwp_plan.restype = C.c_int
        l.zlwp_plan.argtypes = [C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                PA, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.zlwp_map.restype = C.c_int64
        l.zlwp_map.argtypes = [PA, C.c_int32, C.c_int64]
        l.zlwp_extent_floats.restype = C.c_int64
        l.zlwp_extent_floats.argtypes = [C.c_int64, C.c_int32]
        l.zlwp_call.restype = C.c_int32
        l.zlwp_call.argtypes = [C.c_int32] + [C.c_void_p] * 13
        _h = l
    return _h


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def anchor_array(anchors):
    a = np.ascontiguousarray(np.asarray(anchors, np.int32).reshape(-1, 2))
    return a, C.cast(a.ctypes.data, PA)


def run_call(cases, short=None, lacking=()):
    """one harness call over the cases.  short: {case index: floats the accessor is told the source holds}; lacking: the cases whose
    original lacks ZL_SOUND_FINITE.  Returns (status, results, extents, writes, offsets, verdicts, walk)"""
    n = len(cases)
    want = [wr.resolve(c["rate"], c["x"].shape[1], c["anchors"]) for c in cases]
    arrs = [anchor_array(c["anchors"])[0] for c in cases]
    srcs = [np.ascontiguousarray(c["x"].T.reshape(-1)) for c in cases]
    floats = [int(harness().zlwp_extent_floats(w[0]["length"], c["x"].shape[0])) if w else 4 for c, w in zip(cases, want)]
    dst = [np.full(k, np.nan, f32) for k in floats]
    writes = [np.zeros(k, np.int32) for k in floats]
    offsets = [np.full(max(1, w[0]["segments"] if w else 1), -1, np.int32) for w in want]
    ptrs = lambda a: (C.c_void_p * n)(*[v.ctypes.data for v in a])
    counts = (C.c_int32 * n)(*[a.shape[0] for a in arrs])
    nsrc = (C.c_int64 * n)(*[(short or {}).get(i, s.size) for i, s in enumerate(srcs)])
    length = (C.c_int32 * n)(*[c["x"].shape[1] for c in cases])
    chans = (C.c_int32 * n)(*[c["x"].shape[0] for c in cases])
    rates = (C.c_double * n)(*[c["rate"] for c in cases])
    out = (_abi.Warp * n)()
    verdicts = (C.c_uint32 * n)(*[1 if i in lacking else 0 for i in range(n)])
    walk = (C.c_int64 * 4)()
    pA, pSrc, pDst, pWrites, pOffs = ptrs(arrs), ptrs(srcs), ptrs(dst), ptrs(writes), ptrs(offsets)
    rc = harness().zlwp_call(n, C.addressof(counts), C.addressof(pA), C.addressof(pSrc), C.addressof(nsrc), C.addressof(length), C.addressof(chans),
                             C.addressof(rates), C.addressof(pDst), C.addressof(pWrites), C.addressof(out), C.addressof(pOffs), C.addressof(verdicts),
                             C.addressof(walk))
    res = [{k: getattr(out[i], k) for k, _ in _abi.Warp._fields_} for i in range(n)]
    return rc, res, dst, writes, offsets, list(verdicts), tuple(walk)


# ---- the header against the restatement ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return wc.grid()


def test_the_grid_covers_what_it_is_meant_to(grid):
    f = wc.facts(grid)
    assert {6, 34, 160} <= f["W"] and max(f["W"]) > 512
    assert f["mono_res"] == {0, 1, 2, 3} and f["stereo_res"] == {0, 1}
    assert {256, 257, 512, 513} <= f["n8"] and f["taus"] == {0.25, 4.0}
    assert {"D<O", "D=O", "D=L", "D=L+1"} <= f["nseg1"]
    assert f["room0"] >= 2 and f["clamp_last"] >= 2 and f["copy_between"] >= 2 and f["edge"] >= 2 and f["one_region"] >= 2
    applied = [wr.resolve(c["rate"], c["x"].shape[1], c["anchors"])[0]["applied"] for c in grid]
    half = applied.index(0, 1)
    assert not applied[0] and not applied[-1] and not applied[half] and not applied[half + 1] and applied.count(0) == 4
    assert {c["x"].shape[0] for c in grid} == {1, 2}
    for c in grid:
        if "expect_off2" in c:
            assert int(wc.want(c)[2][2]) == c["expect_off2"] > 0, c["tag"]


def test_harness_matches_the_restatement_on_every_bit(grid):
    rc, res, dst, writes, offsets, verdicts, walk = run_call(grid)
    assert rc == len(grid) - 4
    assert walk[3] == 0, "a read outside a clip's own floats"
    segs = 0
    for i, c in enumerate(grid):
        summary, y, offs, ext = wc.want(c)
        assert res[i] == summary, (c["tag"], res[i], summary)
        if not summary["applied"]:
            assert not writes[i].any() and np.isnan(dst[i]).all()
            continue
        assert np.array_equal(offsets[i], offs), (c["tag"], offsets[i], offs)
        assert np.all(writes[i] == 1), (c["tag"], np.flatnonzero(writes[i] != 1)[:8])
        assert dst[i].size == ext.size and np.array_equal(dst[i].view(u32), ext.view(u32)), (c["tag"], np.flatnonzero(dst[i].view(u32) != ext.view(u32))[:8])
        assert verdicts[i] == 0
        segs += sum(r["nseg"] - 1 for r in wr.resolve(c["rate"], c["x"].shape[1], c["anchors"])[1])
    assert walk[2] == segs and walk[0] > rc and walk[1] >= rc


def test_a_join_is_the_previous_slices_continuation_faded_into_the_next(grid):
    """the first O frames behind every anchor, written out by hand for the joins of one case: behind a stretched region, behind a copy
    region and inside a region -- the frames the segment in front would have played next, faded into the new segment's own"""
    c = next(k for k in grid if k["tag"] == "copy-between")
    x = c["x"]
    summary, regs = wr.resolve(c["rate"], x.shape[1], c["anchors"])
    _, y, offs, _ = wc.want(c)
    O, k0 = summary["overlap"], 0
    prev = None
    joins = 0
    for r in regs:
        for k in range(r["nseg"]):
            b = r["a"] if k == 0 else r["a"] + min(int(math.floor(k * r["step"])), r["room"]) + int(offs[k0 + k])
            frames = min(r["L"], r["D"] - k * r["L"])
            n0 = r["d"] + k * r["L"]
            if prev is not None:
                pb, plen = prev
                for j in range(min(O, frames)):
                    w = f32(j) / f32(O)
                    for ch in range(x.shape[0]):
                        want = x[ch, pb + plen + j] * (f32(1.0) - w) + x[ch, b + j] * w
                        assert y[ch, n0 + j] == want, (r["d"], k, j)
                assert np.array_equal(y[:, n0], x[:, pb + plen]) and not np.array_equal(y[:, n0:n0 + O], x[:, b:b + O])
                joins += 1
            assert np.array_equal(y[:, n0 + min(O, frames):n0 + frames], x[:, b + min(O, frames):b + frames])
            prev = (b, frames)
        k0 += r["nseg"]
    assert joins == summary["segments"] - 1 >= 4 and np.array_equal(y[:, :O], x[:, :O])


def test_a_call_of_identities_touches_nothing(grid):
    cases = [c for c in grid if not wc.want(c)[0]["applied"]]
    rc, res, dst, writes, _, _, walk = run_call(cases)
    assert rc == 0 and walk == (0, 0, 0, 0) and all(not w.any() for w in writes)
    for c, r in zip(cases, res):
        assert r == dict(applied=0, regions=len(c["anchors"]) - 1, stretched_regions=0, segments=len(c["anchors"]) - 1, length=c["x"].shape[1], overlap=wr.overlap(c["rate"]))


def test_the_harness_refuses_a_read_outside_the_buffer_it_was_given():
    """the refusal is the accessor's: told that the buffer is one float shorter than the clip, the same walk is refused the reads of
    that float -- the seek's and the synthesis' -- and the NaN shows in the output"""
    c = wc.case("short", 1000, 1, [(100, 150), (100, 100)])
    rc, _, dst, writes, _, verdicts, walk = run_call([c])
    assert rc == 1 and walk[3] == 0 and verdicts == [0]
    rc, _, dst, writes, _, verdicts, walk = run_call([c], short={0: 199})
    assert rc == 1 and walk[3] >= 1 and np.all(writes[0] == 1)
    assert np.isnan(dst[0][249]) and verdicts == [1] and np.isnan(dst[0]).sum() == 1


def test_the_verdict():
    """an inf the warp plays, a NaN it plays, two samples near FLT_MAX that are finite and stay so under the fade's weights (they sum to
    1); a clip whose original lacks the flag keeps its word; the restatement says the same"""
    base = wc.clip(6, 2, 300)
    cases = []
    for k in range(5):
        x = base.copy()
        if k == 1:
            x[1, 10] = np.inf
        if k == 2:
            x[0, 290] = np.nan
        if k == 3:
            x[0, 5] = x[1, 200] = 3e38
        cases.append(dict(tag="verdict%d" % k, rate=1000.0, x=x, anchors=[(0, 0), (150, 200), (300, 330)]))
    rc, res, dst, _, _, verdicts, walk = run_call(cases + [dict(cases[0], tag="verdict-lacking")], lacking=(5,))
    assert rc == 6 and walk[3] == 0
    assert verdicts == [0, 1, 1, 0, 0, 1]
    for i, c in enumerate(cases):
        summary, y, offs, _ = wr.warp(c["x"], c["rate"], c["anchors"])
        assert wr.all_finite(y) == (verdicts[i] == 0)
        assert wc.same_bits(dst[i], wr.extent(y))


# ---- resolve --------------------------------------------------------------------------------------------------------------------------
def resolve_all(rate, length, anchors):
    """the header's, the library's and the restatement's answer; they agree"""
    outs = []
    arr, p = anchor_array(anchors)
    for fn in (harness().zlwp_resolve, zlhip().zlhip_warp_resolve):
        out = _abi.Warp()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = fn(rate, length, p, arr.shape[0], C.byref(out))
        if rc != 0:
            assert bytes(out) == b"\x5a" * C.sizeof(out)
        outs.append({k: getattr(out, k) for k, _ in _abi.Warp._fields_} if rc == 0 else None)
    ref = wr.resolve(rate, length, anchors)
    ref = ref[0] if ref else None
    assert outs[0] == outs[1] == ref, (outs, ref)
    return ref


def test_resolve_at_every_limit(built):
    R = 1000.0                                                     # O = 16; tau >= 2: L = 24, W = 15; tau <= 0.5: L = 74, W = 20
    assert resolve_all(R, 400, [(0, 0), (400, 100)])["applied"] == 1 and resolve_all(R, 401, [(0, 0), (401, 100)]) is None          # A = 4 D | 4 D + 1
    assert resolve_all(R, 100, [(0, 0), (100, 400)])["applied"] == 1 and resolve_all(R, 100, [(0, 0), (100, 401)]) is None          # D = 4 A | 4 A + 1
    r = resolve_all(R, 93, [(0, 0), (93, 200)])                                                                                     # room = 0 | -1
    assert r == dict(applied=1, regions=1, stretched_regions=1, segments=3, length=200, overlap=16)
    assert resolve_all(R, 92, [(0, 0), (92, 200)]) is None
    assert resolve_all(R, 38, [(0, 0), (38, 10)])["segments"] == 1 and resolve_all(R, 37, [(0, 0), (37, 10)]) is None
    # W + O = 4608, the seek's staging: 204800 Hz at tau <= 0.5 gives W = 4096, O = 512; a little faster and W = 4097
    n = 40000
    assert wr.seq_seek(204800.0, 0.5)[1] + wr.overlap(204800.0) == 4608
    assert resolve_all(204800.0, n, [(0, 0), (n, 2 * n)])["applied"] == 1
    assert wr.seq_seek(204850.0, 0.5)[1] == 4097 and resolve_all(204850.0, n, [(0, 0), (n, 2 * n)]) is None
    # 4096 anchors, 4097
    many = [(i * 100, i * 100 + (0 if i == 0 else 1)) for i in range(4096)]
    assert resolve_all(R, many[-1][0], many) == dict(applied=1, regions=4095, stretched_regions=1, segments=4096, length=many[-1][1], overlap=16)
    more = many + [(many[-1][0] + 100, many[-1][1] + 100)]
    assert resolve_all(R, more[-1][0], more) is None
    assert resolve_all(R, 100, [(0, 0)]) is None
    # first or last anchor wrong
    assert resolve_all(R, 200, [(1, 0), (200, 300)]) is None and resolve_all(R, 200, [(0, 1), (200, 300)]) is None
    assert resolve_all(R, 200, [(0, 0), (199, 300)]) is None and resolve_all(R, 200, [(0, 0), (201, 300)]) is None
    # a repeated a or d, a step back
    assert resolve_all(R, 300, [(0, 0), (100, 150), (100, 160), (300, 400)]) is None
    assert resolve_all(R, 300, [(0, 0), (100, 150), (110, 150), (300, 400)]) is None
    assert resolve_all(R, 300, [(0, 0), (100, 150), (90, 160), (300, 400)]) is None
    # the identity: resolves, not applied
    assert resolve_all(R, 300, [(0, 0), (100, 100), (300, 300)]) == dict(applied=0, regions=2, stretched_regions=0, segments=2, length=300, overlap=16)
    assert resolve_all(R, 1, [(0, 0), (1, 1)])["applied"] == 0
    # N + 8 <= INT32_MAX (a copy region of that size is arithmetic only)
    big = 2 ** 31 - 1 - 8
    assert resolve_all(R, big, [(0, 0), (big, big)])["applied"] == 0 and resolve_all(R, big, [(0, 0), (big, big + 1)]) is None
    assert resolve_all(0.0, 300, [(0, 0), (300, 400)]) is None and resolve_all(float("nan"), 300, [(0, 0), (300, 400)]) is None
    z = zlhip()
    assert z.zlhip_warp_resolve(R, 300, None, 2, C.byref(_abi.Warp())) == _abi.ZLHIP_ERR_INVALID


def test_map(built):
    anchors = [(0, 0), (100, 150), (150, 200), (300, 260)]
    arr, p = anchor_array(anchors)
    for src in list(range(-3, 305)) + [10 ** 12, -10 ** 12]:
        ref = wr.warp_map(anchors, src)
        assert harness().zlwp_map(p, 4, src) == zlhip().zlhip_warp_map(p, 4, src) == ref, src
    assert [wr.warp_map(anchors, s) for s in (0, 1, 2, 99, 100, 101, 299, 300)] == [0, 1, 3, 148, 150, 151, 259, 260]
    assert zlhip().zlhip_warp_map(None, 4, 5) == -1 and zlhip().zlhip_warp_map(p, 1, 5) == -1


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def plan_all(rate, length, onsets, src_bpm, dst_bpm, steps, strength, origin, preroll=-1, capacity=None):
    on = np.ascontiguousarray(np.asarray(onsets, np.int32))
    cap = len(onsets) + 2 if capacity is None else capacity
    outs = []
    for fn in (harness().zlwp_plan, zlhip().zlhip_warp_plan):
        buf = np.full((max(cap, 1), 2), -77, np.int32)
        n, dropped = C.c_int32(-5), C.c_int32(-5)
        rc = fn(rate, length, on.ctypes.data, on.size, src_bpm, dst_bpm, steps, strength, origin, preroll, C.cast(buf.ctypes.data, PA), cap, C.byref(n), C.byref(dropped))
        outs.append((rc, [tuple(int(v) for v in row) for row in buf[:n.value]] if rc == 0 else None, dropped.value if rc == 0 else None))
    assert outs[0][1:] == outs[1][1:] and (outs[0][0] == 0) == (outs[1][0] == 0), outs
    return outs[1]


def test_plan_matches_its_restatement_and_always_resolves(built):
    rng = np.random.default_rng(11)
    checked = 0
    for trial in range(120):
        rate = float(rng.choice([1000.0, 4000.0, 8000.0, 44100.0]))
        length = int(rate * rng.uniform(1.0, 4.0))
        src_bpm = float(rng.uniform(70.0, 170.0))
        dst_bpm = float(src_bpm * rng.uniform(0.45, 2.2))
        steps = int(rng.choice([1, 2, 4, 8]))
        strength = float(rng.choice([0.0, 0.5, 1.0, rng.uniform(0.0, 1.0)]))
        origin = int(rng.integers(0, length // 4))
        g = rate * 60.0 / (src_bpm * steps)
        grid = np.arange(origin, length, g)
        onsets = np.unique(np.clip(np.rint(grid + rng.uniform(-0.3, 0.3, grid.size) * g), 0, length).astype(np.int64))
        if trial % 5 == 0:
            onsets = np.unique(np.concatenate([onsets, onsets[:3] + 2, [length]]).clip(0, length))
        preroll = int(rng.choice([-1, 0, 5]))
        ref = wr.plan(rate, length, onsets, src_bpm, dst_bpm, steps, strength, origin, preroll)
        rc, anchors, dropped = plan_all(rate, length, onsets, src_bpm, dst_bpm, steps, strength, origin, preroll)
        if ref is None:
            assert rc == _abi.ZLHIP_ERR_INVALID
            continue
        assert rc == 0 and anchors == ref[0] and dropped == ref[1], (trial, anchors, ref)
        assert wr.resolve(rate, length, anchors) is not None, trial
        assert resolve_all(rate, length, anchors) is not None
        checked += 1
    assert checked >= 80


def test_plan_strength_zero_at_equal_bpm_is_the_identity(built):
    onsets = [500, 1010, 1490, 2003, 2600, 3100]
    rc, anchors, dropped = plan_all(4000.0, 4000, onsets, 120.0, 120.0, 4, 0.0, 0)
    assert rc == 0 and dropped == 0 and anchors == [(0, 0)] + [(t - 32, t - 32) for t in onsets] + [(4000, 4000)]
    assert wr.resolve(4000.0, 4000, anchors)[0]["applied"] == 0


def test_plan_strength_one_puts_every_kept_hit_on_the_grid(built):
    rate, length, bpm, steps = 4000.0, 16000, 120.0, 2
    g = rate * 60.0 / (bpm * steps)                                # 1000 frames
    rng = np.random.default_rng(3)
    onsets = [int(round(k * g + rng.integers(-60, 61))) for k in range(1, 15)]
    for dst_bpm in (120.0, 100.0, 137.0):
        rc, anchors, dropped = plan_all(rate, length, onsets, bpm, dst_bpm, steps, 1.0, 0)
        assert rc == 0 and dropped == 0 and len(anchors) == len(onsets) + 2
        P, scale = wr.overlap(rate), bpm / dst_bpm
        for (a, d), t in zip(anchors[1:-1], onsets):
            k = round(t / g)
            assert a == t - P and d + P == int(wr.rint((k * g) * scale)), (a, d, t)
        assert anchors[-1] == (length, int(wr.rint(length * scale)))


def test_plan_drops_hits_closer_than_a_region_may_be(built):
    """at 4000 Hz a stretched region needs A >= L + W - 1 >= 187 frames and a ratio inside 2: a flam 40 frames behind a hit that is moved
    by 30 cannot be a region of its own, and a hit moved by more than its distance to the one before is dropped too"""
    rate, length = 4000.0, 8000
    onsets = [1030, 1070, 2000, 2950, 3990, 4010, 6020]
    rc, anchors, dropped = plan_all(rate, length, onsets, 120.0, 120.0, 4, 1.0, 0)
    ref = wr.plan(rate, length, onsets, 120.0, 120.0, 4, 1.0, 0)
    assert rc == 0 and (anchors, dropped) == ref
    kept = [a + 32 for a, _ in anchors[1:-1]]
    assert 1030 in kept and 1070 not in kept and dropped >= 1 and dropped == len(onsets) - len(kept)
    assert wr.resolve(rate, length, anchors)[0]["applied"] == 1


def test_plan_parameter_ranges(built):
    ok = dict(rate=4000.0, length=8000, onsets=[1030, 2000], src_bpm=120.0, dst_bpm=100.0, steps=4, strength=1.0, origin=0)
    assert plan_all(**ok)[0] == 0
    for k, v in (("strength", -0.01), ("strength", 1.01), ("strength", float("nan")), ("steps", 0), ("steps", 65), ("src_bpm", 0.0), ("dst_bpm", -1.0),
                 ("src_bpm", float("inf")), ("dst_bpm", float("nan")), ("origin", -1), ("origin", 8000), ("dst_bpm", 500.0), ("dst_bpm", 50.0),
                 ("onsets", [2000, 1030]), ("onsets", [-1]), ("onsets", [8001])):
        bad = dict(ok); bad[k] = v
        assert plan_all(**bad)[0] == _abi.ZLHIP_ERR_INVALID, (k, v)
        assert wr.plan(bad["rate"], bad["length"], bad["onsets"], bad["src_bpm"], bad["dst_bpm"], bad["steps"], bad["strength"], bad["origin"]) is None, (k, v)
    assert plan_all(**ok, capacity=3)[0] == _abi.ZLHIP_ERR_CAPACITY and plan_all(**ok, capacity=4)[0] == 0 and plan_all(**ok, capacity=1)[0] == _abi.ZLHIP_ERR_CAPACITY


# ---- what it does to sound (the restatement alone) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_bpm", [120.0, 110.0, 131.0])
def test_click_track_every_hit_is_heard_once_and_on_the_grid(dst_bpm):
    """single-sample impulses over low noise, jittered around a grid, planned at strength 1 (tau on both sides of 1 inside the clip, and
    D > O everywhere): the warped data holds exactly as many frames above half scale as the source, each at its planned dst + P"""
    rate, bpm, steps = 4000.0, 120.0, 2
    g = rate * 60.0 / (bpm * steps)                                # 1000 frames
    rng = np.random.default_rng(21)
    length = 12000
    hits = [int(k * g + j) for k, j in zip(range(1, 11), (-90, 70, -40, 95, -100, 20, 60, -75, 85, -30))]
    x = rng.uniform(-0.01, 0.01, (1, length)).astype(f32)
    x[0, hits] = 1.0
    anchors, dropped = wr.plan(rate, length, hits, bpm, dst_bpm, steps, 1.0, 0)
    assert dropped == 0 and len(anchors) == len(hits) + 2
    summary, regs = wr.resolve(rate, length, anchors)
    assert all(r["D"] > summary["overlap"] for r in regs)
    taus = [r["A"] / r["D"] for r in regs]
    assert min(taus) < 1.0 < max(taus)
    summary, y, offs, _ = wr.warp(x, rate, anchors)
    loud = np.flatnonzero(np.abs(y[0]) > 0.5)
    P = summary["overlap"]
    assert loud.size == len(hits), (loud, hits)
    assert list(loud) == [d + P for _, d in anchors[1:-1]]
    assert np.all(y[0, loud] == f32(1.0))                          # the attack is the source's own sample


def test_steady_sine_keeps_its_steps_small():
    """a sine of period 40 frames at 4000 Hz through alternating regions of tau about 0.9 and 1.1: the largest sample-to-sample step of
    the output against the source's own largest step.  Observed on the restatement: see DESIGN.md section 19; asserted with a margin
    of a quarter over it.  (A seek that fails to line the phases up, or a join without its fade, gives a step near the sine's peak to
    peak: a ratio of about 12.)"""
    rate, n = 4000.0, 16000
    t = np.arange(n)
    x = (0.5 * np.sin(2 * np.pi * t / 40.0))[None, :].astype(f32)
    pairs = [(900, 1000) if k % 2 == 0 else (1100, 1000) for k in range(16)]
    anchors = wc.chain(pairs)
    summary, y, offs, _ = wr.warp(x, rate, anchors)
    own = float(np.max(np.abs(np.diff(x[0].astype(np.float64)))))
    got = float(np.max(np.abs(np.diff(y[0].astype(np.float64)))))
    print("sine: largest step %.5f against the source's %.5f: ratio %.3f" % (got, own, got / own))
    assert got / own <= SINE_STEP_RATIO * 1.25


SINE_STEP_RATIO = 1.781    # observed on the restatement


# ---- the C-ABI without a GPU, the layouts, the kernels' resources ---------------------------------------------------------------------
def test_without_a_gpu_the_calls_answer_invalid(built):
    l = zlhip()
    arr, p = anchor_array([(0, 0), (100, 150)])
    q = _abi.WarpRequest(0, 2, p)
    out = _abi.Warp()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert l.zlhip_sound_warp(None, C.byref(q), C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_warp_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_warp_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_warp_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_warp_offsets(None, 0, None, 0, None) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    lz = C.CDLL(build.build_engine())
    fn = lz.libzl_hotpath_clip_warp_to_grid
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    n = C.c_int(-7)
    assert fn(None, 0.0, 4, 1.0, C.byref(n), None) == _abi.ZLHIP_ERR_INVALID and n.value == -7
    assert l.zlhip_abi_version() == 3


def test_warp_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_warp_anchor", _abi.WarpAnchor), ("zlhip_warp_request", _abi.WarpRequest), ("zlhip_warp", _abi.Warp))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    body += 'printf("%d ",ZLHIP_WARP_MAX_ANCHORS);'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-1] == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:3] == [8, 16, 24] and got[-1] == _abi.WARP_MAX_ANCHORS == wr.MAX_ANCHORS == 4096
    assert got[3:-1] == [0, 4] + [0, 4, 8] + list(range(0, 24, 4))


def test_warp_kernels_have_no_scratch_memory_and_the_seek_keeps_section_8s_lds(built):
    lib = os.path.join(ROOT, "libzl_amd", "lib")

    def rows(path):
        assert os.path.exists(path), "build() writes the kernels' resources"
        out = {}
        for line in open(path):
            name, *kv = line.split()
            out[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
        return out
    mine = rows(os.path.join(lib, "libzlhip_zl_warp_kernel_resources.txt"))
    theirs = rows(os.path.join(lib, "libzlhip_zl_stretch_kernel_resources.txt"))
    seek = [r for n, r in mine.items() if "zl_k_warp_seek" in n]
    synth = [r for n, r in mine.items() if "zl_k_warp_synth" in n]
    st_seek = [r for n, r in theirs.items() if "zl_k_stretch_seek" in n]
    assert len(seek) == 1 and len(synth) == 1 and len(mine) == 2 and len(st_seek) == 1, (mine, theirs)
    for r in mine.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, mine
    assert seek[0]["lds"] == st_seek[0]["lds"] == 2 * 4 * 4608 + 2 * 4 * 512 + 8 * 8 + 8 * 4 + 8, (mine, theirs)
    assert synth[0]["lds"] == 0 and synth[0]["waves"] >= 8, mine


# ---- the walk under the sanitizers ------------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/warp_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with AddressSanitizer
    and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment loads
    in front of it."""
    exe = str(tmp_path / "warp_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "warp_check.cpp"), "-o", exe])
    for args in (["1", "40"], ["2", "40"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "warp check ok" in rc.stdout
