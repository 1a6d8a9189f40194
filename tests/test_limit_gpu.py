"""Peaks and limiter, GPU tier: the kernels of libzl_amd/csrc/zl_limit.hip against the numpy restatement (tests/limit_ref.py), which takes
its filter rows from zlhip_resample_design so that libm does not enter.  Every extent is read back whole (zlhip_debug_sound_extent) from
an arena that held noise and compared == with the restatement; every chunk record of the analysis likewise; then the single call and a
limit of a limited clip, a loud neighbour, a grown arena, the buffers, every refusal, the render an all-identity call does not launch,
the finite flag, the resident kernel, a voice over a limited clip against the oracle's run over the restatement's data, the group."""
import ctypes as C
import os

import numpy as np
import pytest

import limit_cases as lc
import limit_ref as lr
from edit_cases import dirty, same_bits

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SR = 48000.0
_TABLES = {}


def tables():
    if not _TABLES:
        from libzl_amd import _abi
        lib = _abi.load()
        for F, rate in ((4, 48000.0), (2, 96000.0)):
            t = np.zeros(F * 64, f32)
            assert lib.zlhip_resample_design(rate, rate * F, None, None, None, None, t.ctypes.data, t.size) == 0
            _TABLES[F] = t.reshape(F, 64)
    return _TABLES


def make(**kw):
    from libzl_amd import SamplerSynth
    cfg = dict(num_buses=2, voices_per_bus=8, max_frames=256, max_batch_blocks=8, max_sounds=32, sound_arena_bytes=4 << 20)
    cfg.update(kw)
    return SamplerSynth(**cfg)


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u32), np.ascontiguousarray(b).view(u32))


def upload(syn, x, sr=SR):
    return syn.register_clip(x[0].copy(), x[1].copy() if x.shape[0] == 2 else None, float(sr))


def case(x, rate=SR, **q):
    return dict(tag="", x=np.ascontiguousarray(x, f32), rate=float(rate), q=q)


def want(c):
    return lr.limit(c["x"], c["rate"], c["q"], tables())


def mismatch(syn, cid, c, got):
    """what differs between the device's answer for case c (result `got`, the extent clip `cid` holds now) and the restatement, or None"""
    res, ext, finite, _ = want(c)
    for k in lr.RESULT_FIELDS:
        a, b = got[k], res[k]
        if (f32(a).view(u32) != f32(b).view(u32)) if isinstance(b, (float, np.floating)) else (a != b):
            return ("result", k, got, res)
    now = syn.clip_extent(cid)
    if not res["applied"]:                                         # (its upload's extent: untouched)
        return same_bits(now[:c["x"].size], np.ascontiguousarray(c["x"].T).reshape(-1))
    if syn.clip_info(cid)["finite"] != finite:
        return ("finite", syn.clip_info(cid)["finite"], finite)
    return same_bits(now, ext)


def check_call(syn, cases, ids):
    """one clip_limit_batch over the cases (clip ids[i] holds cases[i]["x"]): (the mismatches, the results)"""
    outs = syn.clip_limit_batch([dict(clip=cid, **c["q"]) for cid, c in zip(ids, cases)])
    bad = []
    for i, (cid, c, got) in enumerate(zip(ids, cases, outs)):
        m = mismatch(syn, cid, c, got)
        if m is not None:
            bad.append((i, c["tag"], c["x"].shape, c["q"], m))
    return bad, outs


def noise(rng, ch, n, amp=0.3):
    return rng.uniform(-amp, amp, (ch, n)).astype(f32)


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
def test_the_grid_in_one_call(built):
    """tests/limit_cases.py::grid (tests/test_limit_cpu.py asserts what it covers): every case in ONE call, the identity first and last;
    then that the clips with nothing to change are untouched and that the extents' tails are the kernel's zeros"""
    cases = lc.grid()
    with make(max_sounds=128, sound_arena_bytes=16 << 20) as s:
        dirty(s, 3 << 20)
        ids = [upload(s, c["x"], c["rate"]) for c in cases]
        before = [s.clip_extent(cid) for cid in ids]
        bad, outs = check_call(s, cases, ids)
        assert not bad, (len(bad), bad[:3])
        idle = [i for i, o in enumerate(outs) if not o["applied"]]
        assert len(idle) >= 5 and idle[0] == 0 and idle[-1] == len(cases) - 1
        for i in idle:
            assert same(s.clip_extent(ids[i]), before[i]), (i, cases[i]["tag"])
        for cid, c, o in zip(ids, cases, outs):
            info = s.clip_info(cid)
            assert (info["length"], info["channels"], info["sample_rate"], info["rendered"]) == (c["x"].shape[1], c["x"].shape[0], c["rate"], False), c["tag"]
            if o["applied"]:
                ext = s.clip_extent(cid)
                assert ext.size > c["x"].size and not ext[c["x"].size:].any(), c["tag"]
                assert not (np.abs(ext[np.isfinite(ext)]) > o["ceiling"]).any(), c["tag"]


def test_the_single_call_and_a_limit_of_a_limited_clip(built):
    with make() as s:
        dirty(s, 200000)
        rng = np.random.default_rng(61)
        x = noise(rng, 2, 5000); x[0, 1203] = 1.4; x[1, 3776] = -0.95; x[1, 3790] = 1.0
        cid = upload(s, x)
        got = s.clip_limit(cid, hold_frames=48)
        c = case(x, hold_frames=48)
        assert got["applied"] == 1 and got["frames_reduced"] > 2 * 240 and 0.6 < got["min_gain"] < 0.65 and got["peak_before"] == f32(1.4)
        assert mismatch(s, cid, c, got) is None
        # again: the peak is at the ceiling now, exactly -- the identity
        L, R = s.read_clip(cid)
        y = np.stack([L, R])
        assert np.abs(y).max() <= lr.CEILING
        ext = s.clip_extent(cid)
        again = s.clip_limit(cid, hold_frames=48)
        assert again["applied"] == 0 and again["peak_before"] == np.abs(y).max() and same(s.clip_extent(cid), ext)
        assert s.clip_peak(cid)["sample_peak"] == (np.abs(y[0]).max(), np.abs(y[1]).max())
        # a lower ceiling with a gain, on the limited data
        c2 = case(y, ceiling=0.25, gain=1.5, lookahead_frames=33, flags=lr.TRUE_PEAK)
        got = s.clip_limit(cid, ceiling=0.25, gain=1.5, lookahead_frames=33, flags=lr.TRUE_PEAK)
        assert got["applied"] == 1 and got["oversampling"] == 4 and mismatch(s, cid, c2, got) is None


# ---- the analysis ---------------------------------------------------------------------------------------------------------------------
def test_the_analysis_gives_the_restatements_records(built):
    cases = lc.peak_cases()
    with make(max_sounds=16, sound_arena_bytes=4 << 20) as s:
        dirty(s, 300000)
        ids = {}
        for x, rate, *_ in cases:
            if (id(x), rate) not in ids:
                ids[(id(x), rate)] = upload(s, x, rate)
        reqs = [dict(clip=ids[(id(x), rate)], first_frame=first, num_frames=num, flags=flags) for x, rate, first, num, flags in cases]
        outs = s.clip_peak_batch(reqs)
        for i, ((x, rate, first, num, flags), got) in enumerate(zip(cases, outs)):
            res, rec = lr.peak(x, rate, first, num, flags, tables())
            assert same(s.peak_chunks(i), rec), (i, rate, first, num, flags)
            assert (got["oversampling"], got["chunks"]) == (res["oversampling"], res["chunks"])
            assert same(np.array(got["sample_peak"], f32), np.array(res["sample_peak"], f32)) and same(np.array(got["true_peak"], f32), np.array(res["true_peak"], f32)), i
        # the single call is the batch of one; num_frames 0 reaches to the end
        x, rate, first, num, flags = cases[3]
        assert s.clip_peak(reqs[3]["clip"], first, 0, flags) == outs[3] and first + num == x.shape[1]


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two at +-7.9 in a small arena that held noise, measured from its first frame to its last with the filter's
    taps reaching over both ends, then limited: a neighbour's float in the detector would be a peak, one in the render a hot frame"""
    with make(max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(65)
        dirty(s, 200000)
        for n in (3333, 2 * lr.CHUNK, 131):
            loud = [np.repeat(rng.choice(np.array([-7.9, 7.9], f32), (1, m)), ch, axis=0) for m in (3001, 3003)]
            quiet = noise(rng, ch, n, 0.2)
            ids = [upload(s, x) for x in (loud[0], quiet, loud[1])]
            res, rec = lr.peak(quiet, SR, 0, n, lr.TRUE_PEAK, tables())
            got = s.clip_peak(ids[1], flags=lr.TRUE_PEAK)
            assert same(s.peak_chunks(0), rec) and max(got["true_peak"]) < 0.8
            before = [s.clip_extent(i) for i in ids]
            assert s.clip_limit(ids[1], flags=lr.TRUE_PEAK)["applied"] == 0
            bad, outs = check_call(s, [case(quiet, gain=2.0, flags=lr.TRUE_PEAK, ceiling=0.5, lookahead_frames=512, hold_frames=512)], [ids[1]])
            assert not bad, bad
            assert outs[0]["peak_before"] < 1.6 and same(s.clip_extent(ids[0]), before[0]) and same(s.clip_extent(ids[2]), before[2])
            for cid in ids:
                s.unregister_clip(cid)


def test_a_clip_in_a_grown_arena(built):
    arena = 1 << 20
    rng = np.random.default_rng(66)
    with make(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [noise(rng, 1 + i % 2, 60000 + 1001 * i) for i in range(8)]
        for x in srcs:
            x[0, 777::9973] = 1.2
        ids = [upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        bad, outs = check_call(s, [case(x, lookahead_frames=100 + 50 * i) for i, x in enumerate(srcs)], ids)
        assert not bad, bad
        assert all(o["applied"] and o["frames_reduced"] > 1000 for o in outs)
        for cid, x in zip(ids, srcs):
            got = s.clip_peak(cid, 1, x.shape[1] - 3, lr.TRUE_PEAK)
            assert max(got["sample_peak"]) <= lr.CEILING and got["chunks"] == (x.shape[1] - 3 + 1023) // 1024


def test_an_engine_that_never_asks_allocates_nothing(built):
    rng = np.random.default_rng(67)
    with make(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        x = noise(rng, 2, 30000); x[1, 5000] = 1.0
        cid = upload(s, x)
        total0, _ = s.memory_bytes()
        s.clip_loudness(cid)
        total1, _ = s.memory_bytes()
        s.clip_peak(cid, flags=1)
        total2, _ = s.memory_bytes()
        s.clip_limit(cid)
        total3, _ = s.memory_bytes()
        assert total3 > total2 > total1 > total0
        s.clip_peak(cid); s.clip_peak(cid, 3, 20000, 1); s.clip_limit(cid, gain=0.5); s.clip_limit(cid, ceiling=0.2, flags=1)      # fit the first calls' buffers
        assert s.memory_bytes()[0] == total3


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_every_clip_and_out_as_they_were(built):
    from libzl_amd import _abi
    INV, CAP, STATE = _abi.ZLHIP_ERR_INVALID, _abi.ZLHIP_ERR_CAPACITY, _abi.ZLHIP_ERR_STATE
    rng = np.random.default_rng(71)
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        lib, e = s._lib, s._e
        a, b = noise(rng, 2, 4000), noise(rng, 1, 5000)
        a[0, 100] = 1.0; b[0, 4999] = -1.0
        big = noise(rng, 2, 70000)                                 # 560 KB: a second extent of it does not fit the arena (1 MiB)
        big[1, 69000] = 1.0
        odd = noise(rng, 1, 3000)
        nonfinite = noise(rng, 1, 2000); nonfinite[0, 7] = np.inf
        ia, ib, ibig, iodd, inf_ = upload(s, a), upload(s, b), upload(s, big), upload(s, odd, 48000.5), upload(s, nonfinite)
        everyone = (ia, ib, ibig, iodd, inf_)
        exts = [s.clip_extent(i) for i in everyone]
        R, P = _abi.LimitRequest, _abi.PeakRequest

        def req(cid, **q):
            return R(cid, int(q.get("flags", 0)), int(q.get("lookahead_frames", 0)), int(q.get("hold_frames", 0)), float(q.get("ceiling", 0.0)), float(q.get("gain", 0.0)))

        def call(reqs, count=None):
            arr = (R * max(1, len(reqs)))(*reqs)
            out = (_abi.Limit * max(1, len(reqs)))()
            C.memset(out, 0x5A, C.sizeof(out))
            rc = lib.zlhip_sound_limit_batch(e, arr, len(reqs) if count is None else count, out)
            return rc, bytes(out) == b"\x5a" * C.sizeof(out)

        def peak(reqs, count=None):
            arr = (P * max(1, len(reqs)))(*reqs)
            out = (_abi.Peak * max(1, len(reqs)))()
            C.memset(out, 0x5A, C.sizeof(out))
            rc = lib.zlhip_sound_peak_batch(e, arr, len(reqs) if count is None else count, out)
            return rc, bytes(out) == b"\x5a" * C.sizeof(out)

        def unchanged():
            return all(same(s.clip_extent(i), x) for i, x in zip(everyone, exts))

        good, other = req(ia), req(ib, hold_frames=10)
        mem = s.memory_bytes()
        bad = [req(ia, flags=2), req(ia, flags=-1), req(ia, lookahead_frames=-1), req(ia, lookahead_frames=513), req(ia, hold_frames=-1), req(ia, hold_frames=513),
               req(ia, ceiling=1.5), req(ia, ceiling=-0.1), req(ia, ceiling=float("nan")), req(ia, gain=-2.0), req(ia, gain=float("inf")), req(ia, gain=float("nan")),
               req(iodd, flags=1), req(31), req(-1), req(99)]
        for r in bad:
            assert call([r]) == (INV, True), bytes(r)
            assert call([other, r]) == (INV, True), bytes(r)       # one bad request fails the call
        assert b"sound_limit" in lib.zlhip_last_error(e)
        assert call([good, good]) == (INV, True) and call([good, other, req(ia, gain=2.0)]) == (INV, True)       # duplicates
        assert call([good], count=-1) == (INV, True) and call([], count=0) == (0, True)
        assert lib.zlhip_sound_limit_batch(e, None, 1, None) == INV and lib.zlhip_sound_limit(None, None, None) == INV
        for p in (P(ia, 0, 0, 0), P(ia, -1, 10, 0), P(ia, 0, 4001, 0), P(ia, 4000, 1, 0), P(ia, 0, 10, 2), P(iodd, 0, 10, 1), P(31, 0, 10, 0), P(-1, 0, 10, 0)):
            assert peak([p]) == (INV, True) and peak([P(ib, 0, 10, 0), p]) == (INV, True), bytes(p)
        assert b"sound_peak" in lib.zlhip_last_error(e)
        assert peak([P(ia, 0, 10, 0)], count=-1) == (INV, True) and peak([], count=0) == (0, True)
        n = C.c_int32(-77)
        assert lib.zlhip_debug_peak_chunks(e, 99, None, 0, C.byref(n)) == INV and n.value == -77
        assert unchanged() and s.memory_bytes() == mem
        # a clip with a sample that is not finite: the analysis takes it (as +0), the limiter refuses it
        assert peak([P(inf_, 0, 2000, 1)])[0] == 0 and not s.clip_info(inf_)["finite"]
        assert call([good, req(inf_)]) == (STATE, True) and b"finite" in lib.zlhip_last_error(e)
        # the odd rate without the flag is fine and under the ceiling: the identity
        assert call([req(iodd)])[0] == 0
        # a clip that plays a re-render
        s.rerender_clip(ib, gain_db=-6.0)
        bre = s.clip_extent(ib)
        assert call([good, other]) == (STATE, True) and call([other]) == (STATE, True)
        assert b"re-render" in lib.zlhip_last_error(e)
        assert same(s.clip_extent(ib), bre) and same(s.clip_extent(ia), exts[0])
        s.rerender_clip(ib)
        assert unchanged()
        # an arena that cannot hold the call, decided behind the detecting pass: the small clip's extent fits, the big one's does not
        assert call([good, req(ibig)]) == (CAP, True)
        assert unchanged()
        assert call([req(ibig, gain=0.5), good]) == (CAP, True)
        assert unchanged()
        # after the errors the call still works; the big clip under a ceiling it does not reach is the identity and needs no room
        bad_, outs = check_call(s, [case(a), case(b, hold_frames=10), case(big, ceiling=1.0)], [ia, ib, ibig])
        assert not bad_, bad_
        assert [o["applied"] for o in outs] == [1, 1, 0]


def test_a_call_of_identities_launches_no_render(built):
    rng = np.random.default_rng(72)
    with make() as s:
        s.set_profiling(True)
        ids = [upload(s, noise(rng, 2, 20000)) for _ in range(3)]
        loud = noise(rng, 2, 20000); loud[0, 9000] = 1.0
        il = upload(s, loud)
        exts = [s.clip_extent(i) for i in ids]
        outs = s.clip_limit_batch([dict(clip=i) for i in ids])
        detect, render = s.limit_timings()
        assert [o["applied"] for o in outs] == [0, 0, 0] and detect > 0.0 and render == 0.0
        assert all(same(s.clip_extent(i), x) for i, x in zip(ids, exts))
        outs = s.clip_limit_batch([dict(clip=ids[0]), dict(clip=il)])
        detect, render = s.limit_timings()
        assert [o["applied"] for o in outs] == [0, 1] and detect > 0.0 and render > 0.0 and same(s.clip_extent(ids[0]), exts[0])
        s.set_profiling(False)
        assert s.clip_limit(ids[1], gain=0.5)["applied"] == 1
        assert s.limit_timings() == (detect, render)               # (the times of the last profiled call stay)


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def test_the_finite_flag(built):
    """a finite clip keeps the flag when every written sample is finite; x = 3e38 with gain 4 is an infinite v, whose product with the
    gain 0 the window's sum gives at the default look-ahead is a NaN: the flag goes.  (At a look-ahead whose fp32 window sums below 1
    the same sample comes out as the ceiling and the flag stays: the restatement decides, the device agrees.)"""
    rng = np.random.default_rng(73)
    base = noise(rng, 2, 3000)
    hot = base.copy(); hot[0, 1500] = 3e38                         # finite: the flag is set
    cases = [case(base, gain=2.0), case(hot), case(hot, gain=4.0), case(hot, gain=4.0, lookahead_frames=64), case(hot, gain=4.0, flags=lr.TRUE_PEAK)]
    with make() as s:
        dirty(s, 100000)
        ids = [upload(s, c["x"]) for c in cases]
        assert all(s.clip_info(i)["finite"] for i in ids)
        bad, outs = check_call(s, cases, ids)
        assert not bad, bad
        assert [s.clip_info(i)["finite"] for i in ids][:3] == [True, True, False]
        assert np.isnan(s.clip_extent(ids[2])).sum() == 1 and np.isinf(outs[2]["peak_before"]) and outs[2]["min_gain"] == 0.0
        # a clip that lost the flag is refused from then on
        from libzl_amd import ZlHipError
        with pytest.raises(ZlHipError):
            s.clip_limit(ids[2])


# ---- the resident kernel ----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_the_resident_kernel_stays_through_peak_calls(built, rt_env):
    """After one warm-up call (it allocates the call's buffers) peak calls between real-time cycles leave the resident kernel where it is:
    one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the records right."""
    from libzl_amd import SamplerSynth
    from oracle import zl_oracle as zo
    from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip
    sc = random_scene(343, num_buses=4, voices_per_bus=4, nclips=6, mode=0, nframes=128, nblocks=16)
    ref_bus, _, _ = run_oracle(sc)
    ref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    syn = SamplerSynth(num_buses=sc.num_buses, voices_per_bus=sc.voices_per_bus, mode=sc.mode, playback_sample_rate=sc.fs,
                       max_frames=max(64, sc.nframes), max_batch_blocks=4, max_sounds=max(8, len(sc.sounds) + 1),
                       sound_arena_bytes=(1 << 20) + sum((s[0].shape[0] + 16) * 8 for s in sc.sounds) + (1 << 16))
    try:
        planar, rates = [], []
        for i, (L, R, sr) in enumerate(sc.sounds):
            assert ref.register_clip(L, R, sr) == i and syn.register_clip(L, R, sr) == i
            if i in sc.clip_setup:
                sc.clip_setup[i](ref.lib, ref.clips[i])
            syn.set_clip_params(i, snapshot_clip(ref.clips[i]))
            planar.append(np.stack([L, R]) if R is not None else L[None, :])
            rates.append(float(sr))
        flag = lambda cid: lr.TRUE_PEAK if lr.rate_ok(rates[cid]) else 0
        syn.clip_peak_batch([dict(clip=i, flags=flag(i)) for i in range(len(planar))] * 2)       # the warm-up call: more than any call below
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts_after_first, todo = None, []
        for k in range(sc.nblocks):
            for ev in sc.events.get(k, []):
                if ev[0] == "cmd":
                    syn.handle_clip_command(engine_cmd(**ev[1]), ev[2])
                elif ev[0] == "start":
                    syn.start_voice(ev[1], ev[2], engine_cmd(**ev[3]), ev[4])
                elif ev[0] == "clip":
                    ev[2](ref.lib, ref.clips[ev[1]])
                    syn.set_clip_params(ev[1], snapshot_clip(ref.clips[ev[1]]))
                elif ev[0] == "update":
                    syn.update_voice(ev[1], ev[2], engine_cmd(**ev[3]))
                elif ev[0] == "stopv":
                    syn.stop_voice(ev[1], ev[2], ev[3])
                elif ev[0] == "enable":
                    syn.set_bus_enabled(ev[1], ev[2])
                else:
                    raise AssertionError(ev[0])
            L, R = syn.process(N, sc.make_clocks(k, 1)[0])
            out[:, 0, k * N:(k + 1) * N] = L
            out[:, 1, k * N:(k + 1) * N] = R
            if starts_after_first is None:
                starts_after_first = syn.rt_stats()[0]
            cid = k % len(planar)
            n = planar[cid].shape[1]
            r = dict(clip=cid, first_frame=min(k, n - 1), num_frames=min(n - min(k, n - 1), 3000), flags=flag(cid))
            got = syn.clip_peak_batch([r])[0]
            todo.append((r, got, syn.peak_chunks(0)))
        starts, cycles = syn.rt_stats()
        assert starts_after_first == 1 and (starts, cycles) == (1, sc.nblocks)
        for r, got, rec in todo:
            res, wrec = lr.peak(planar[r["clip"]], rates[r["clip"]], r["first_frame"], r["num_frames"], r["flags"], tables())
            assert same(rec, wrec) and same(np.array(got["true_peak"], f32), np.array(res["true_peak"], f32)), r
        assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
    finally:
        syn.close()


# ---- playback -------------------------------------------------------------------------------------------------------------------------
LIMIT = dict(ceiling=0.1, lookahead_frames=120, hold_frames=30, flags=lr.TRUE_PEAK)


def playback_scene(y, note, nblocks=24):
    """one looping voice over a free-running loop of some 2300 frames from frame 1440 of clip y (planar)"""
    from scenario import Scene, play_cmd
    sc = Scene(num_buses=1, voices_per_bus=2, fs=SR, mode=0, mix_group=0, nframes=256, nblocks=nblocks, bpm=120)
    sc.sounds.append((y[0].copy(), y[1].copy() if y.shape[0] == 2 else None, SR))

    def setup(lib, clip):
        lib.zlo_clip_set_start_position(clip, C.c_float(0.030005))
        lib.zlo_clip_set_length(clip, C.c_float(0.1), 120)           # no whole number of beats: the free-running loop branch
    sc.clip_setup[0] = setup
    sc.events[0] = [("cmd", play_cmd(0, midi_channel=-2, loop=True, note=note, volume=0.8), 0)]
    return sc


def play_limited(x, note, resident=False):
    """(the engine's audio of a looping voice over clip x limited on the device, the oracle's audio over the restatement's data)"""
    from libzl_amd.engine import synthetic_clocks
    from scenario import engine_cmd, run_oracle
    c = case(x, **LIMIT)
    res, ext, finite, d = want(c)
    assert res["applied"] and res["frames_reduced"] > 1000 and finite
    sc = playback_scene(d["out"], note)
    from oracle import zl_oracle as zo
    from scenario import snapshot_clip
    ref = zo.OracleSynth(1, 1, SR, 0, max_sounds=8)
    assert ref.register_clip(*sc.sounds[0]) == 0
    sc.clip_setup[0](ref.lib, ref.clips[0])
    p = snapshot_clip(ref.clips[0])
    with make(num_buses=1, voices_per_bus=2, max_batch_blocks=sc.nblocks) as s:
        cid = upload(s, x)
        got = s.clip_limit(cid, **LIMIT)
        assert mismatch(s, cid, c, got) is None
        s.set_clip_params(cid, p)
        s.handle_clip_command(engine_cmd(**sc.events[0][0][1]), 0)
        if resident:
            out = np.zeros((1, 2, sc.nblocks * 256), f32)
            clocks = synthetic_clocks(sc.nblocks, 256, SR)
            for k in range(sc.nblocks):
                L, R = s.process(256, clocks[k])
                out[:, 0, k * 256:(k + 1) * 256] = L
                out[:, 1, k * 256:(k + 1) * 256] = R
            assert s.rt_stats()[1] == sc.nblocks
        else:
            s.render_batch(sc.nblocks, 256, synthetic_clocks(sc.nblocks, 256, SR))
            out = np.array(s.read_bus(), copy=True)
    ref_bus, _, _ = run_oracle(sc)
    return out, ref_bus


def signal(seed):
    t = np.arange(6000, dtype=np.float64)
    v = 0.3 * np.sin(2.0 * np.pi * t / 218.4) * np.exp(-t / 3000.0)
    return (np.stack([v, 0.9 * v]) + np.random.default_rng(seed).standard_normal((2, 6000)) * 0.01).astype(f32)


@pytest.mark.parametrize("note", [60, 67], ids=["on-grid", "pitched"])
def test_a_voice_over_a_limited_clip_equals_the_oracle_over_the_restatement(built, note):
    out, ref_bus = play_limited(signal(76), note)
    assert out.shape == ref_bus.shape and len(np.unique(out[0, 0])) > 1000
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


def test_a_voice_through_the_resident_kernel_equals_the_oracle(built, rt_env):
    out, ref_bus = play_limited(signal(77), 60, resident=True)
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"


# ---- the group --------------------------------------------------------------------------------------------------------------------------
def test_group_limits_on_every_member(built):
    from libzl_amd import SamplerSynthGroup, ZlHipError
    rng = np.random.default_rng(78)
    with SamplerSynthGroup([0, 0], 4, 8, max_frames=256, max_batch_blocks=8, max_sounds=16, sound_arena_bytes=1 << 22) as g:
        q = noise(rng, 2, 3000); q[1, 700] = 1.5; q[0, 2100] = -1.0
        m = noise(rng, 1, 1500); m[0, 1499] = 0.95
        cases = [case(q, hold_frames=20), case(m, flags=lr.TRUE_PEAK, lookahead_frames=17), case(noise(rng, 2, 300))]
        ids = [upload(g, c["x"]) for c in cases]
        pk = g.clip_peak_batch([dict(clip=cid, flags=lr.TRUE_PEAK) for cid in ids])
        for c, got in zip(cases, pk):
            res, _ = lr.peak(c["x"], SR, 0, c["x"].shape[1], lr.TRUE_PEAK, tables())
            assert same(np.array(got["true_peak"], f32), np.array(res["true_peak"], f32))
        outs = g.clip_limit_batch([dict(clip=cid, **c["q"]) for cid, c in zip(ids, cases)])
        assert [o["applied"] for o in outs] == [1, 1, 0]
        for r in range(2):
            for cid, c, got in zip(ids, cases, outs):
                n = C.c_size_t(0)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, None, 0, C.byref(n)) == 0
                ext = np.empty(n.value, f32)
                assert g._lib.zlhip_debug_sound_extent(g.member(r), cid, ext.ctypes.data, ext.size, None) == 0
                res, wext, _, _ = want(c)
                assert all(f32(got[k]).view(u32) == f32(res[k]).view(u32) for k in lr.RESULT_FIELDS), (r, cid, got, res)
                if res["applied"]:
                    assert same_bits(ext, wext) is None, (r, cid)
        with pytest.raises(ZlHipError, match="member 0"):
            g.clip_limit_batch([dict(clip=ids[0]), dict(clip=ids[0])])


# ---- the libzl-named layer --------------------------------------------------------------------------------------------------------------
def test_libzl_true_peak_limit_and_level_limited(built, tmp_path):
    """the three calls of the libzl-named layer on loaded clips: the true peak against the restatement; a limit baked at the current level;
    a bank levelled under a ceiling in one loudness call and one limit call -- among it the quiet clip with one full-scale click that
    libzl_hotpath_clips_level can only hold under the ceiling (tests/test_loudness_gpu.py): it now reaches the target within what the
    limiter took, lufs_after <= target and peak <= ceiling exactly"""
    import math
    from libzl_amd import _abi, libzl
    from test_loudness_gpu import _clip
    zl = libzl.load()
    zl.initJuce()
    try:
        assert zl.libzl_hotpath_status() == 0
        lib = _abi.load()
        eng = C.c_void_p(zl.libzl_hotpath_engine())
        pad = _clip(2, 30000, 51, level=0.05)
        kick = (np.exp(-np.arange(30000) / 1500.0) * np.sin(2 * np.pi * 55.0 * np.arange(30000) / SR) * 0.9).astype(f32)[None, :]
        hot = _clip(1, 30000, 52, level=0.02)
        hot[0, 1000] = 0.99                                        # one full-scale click in a quiet clip
        silent = np.zeros((1, 30000), f32)
        clips = {}
        for name, src in (("pad", pad), ("kick", kick), ("hot", hot), ("silent", silent), ("pad2", pad), ("kick2", kick)):
            path = str(tmp_path / (name + ".wav")).encode()
            assert zl.libzl_wav_write(path, src[0].ctypes.data, src[1].ctypes.data if src.shape[0] == 2 else None, src.shape[1], SR, 32) == 0
            clips[name] = zl.ClipAudioSource_new(path, False)
            assert clips[name]

        def played(clip):
            cid, cnt = zl.ClipAudioSource_engineClip(clip), C.c_int32(0)
            assert lib.zlhip_sound_read(eng, cid, None, None, 0, C.byref(cnt)) >= 0
            pl, pr_ = np.empty(cnt.value, f32), np.empty(cnt.value, f32)
            chans = lib.zlhip_sound_read(eng, cid, pl.ctypes.data, pr_.ctypes.data, cnt.value, C.byref(cnt))
            return np.stack([pl, pr_]) if chans == 2 else pl[None, :]

        def loudness(clip):
            lufs, peak = C.c_double(7.0), C.c_float(7.0)
            assert zl.libzl_hotpath_clip_loudness(clip, C.byref(lufs), C.byref(peak)) == 1
            return lufs.value

        ceiling = f32(10.0 ** (-1.0 / 20.0))
        # the true peak
        sp, tp = C.c_float(7.0), C.c_float(7.0)
        assert zl.libzl_hotpath_clip_true_peak(None, C.byref(sp), C.byref(tp)) == _abi.ZLHIP_ERR_INVALID and (sp.value, tp.value) == (7.0, 7.0)
        assert zl.libzl_hotpath_clip_true_peak(clips["kick"], C.byref(sp), C.byref(tp)) == 1
        res, _ = lr.peak(kick, SR, 0, 30000, lr.TRUE_PEAK, tables())
        assert f32(sp.value) == f32(20.0 * math.log10(res["sample_peak"][0])) and f32(tp.value) == f32(20.0 * math.log10(res["true_peak"][0])) and tp.value >= sp.value
        assert zl.libzl_hotpath_clip_true_peak(clips["silent"], C.byref(sp), C.byref(tp)) == 1 and sp.value == tp.value == -math.inf
        # a limit at the current level: the kick's first cycles come under -6 dBFS, its tail keeps its bits
        red = C.c_float(7.0)
        for bad in ((1.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (-6.0, -1.0, 0.0), (-6.0, 20.0, 0.0), (-6.0, 0.0, -1.0), (-6.0, 0.0, 20.0), (-6.0, 0.001, 0.0)):
            assert zl.libzl_hotpath_clip_limit(clips["kick"], *bad, 0, C.byref(red)) == _abi.ZLHIP_ERR_INVALID and red.value == 7.0, bad
        assert zl.libzl_hotpath_clip_limit(clips["kick"], -6.0, 2.0, 1.0, 0, C.byref(red)) == 1
        c = case(kick, ceiling=float(f32(10.0 ** (-6.0 / 20.0))), lookahead_frames=96, hold_frames=48)
        wres, wext, _, d = want(c)
        got = played(clips["kick"])
        assert same(got, d["out"]) and f32(red.value) == f32(-20.0 * math.log10(float(wres["min_gain"]))) and 3.5 < red.value < 4.5      # (the first crest, 0.9 exp(-218 / 1500) = 0.78, over 0.5)
        assert same(got[:, 20000:], kick[:, 20000:]) and np.abs(got).max() <= c["q"]["ceiling"]
        assert zl.libzl_hotpath_clip_limit(clips["kick"], -6.0, 2.0, 1.0, 0, C.byref(red)) == 0 and red.value == 0.0          # under the ceiling now
        # a clip that plays a re-render is refused: limit first, level afterwards
        zl.ClipAudioSource_setGain(clips["pad"], C.c_float(-3.0))
        assert zl.libzl_hotpath_clip_limit(clips["pad"], -6.0, 0.0, 0.0, 0, None) == _abi.ZLHIP_ERR_STATE
        # a bank: the hot clip, a NULL, a silent clip, a pad, the re-rendered pad, a kick -- one call
        target = 0.0                                               # (loud enough that every clip of the bank is driven over the ceiling)
        bank = [clips["hot"], None, clips["silent"], clips["pad2"], clips["pad"], clips["kick2"]]
        before = [loudness(c_) if c_ is not None and c_ != clips["silent"] else None for c_ in bank]
        kept = played(clips["pad"])
        arr = (C.c_void_p * 6)(*bank)
        drive, reduction = (C.c_float * 6)(*[9.0] * 6), (C.c_float * 6)(*[9.0] * 6)
        assert zl.libzl_hotpath_clips_level_limited(arr, 6, target, -1.0, 0.0, 0.0, 1, drive, reduction) == 3
        assert [drive[i] != 0.0 for i in range(6)] == [True, False, False, True, False, True] and drive[1] == drive[2] == drive[4] == 0.0
        for i in (0, 3, 5):
            assert abs(drive[i] - (target - before[i])) < 1e-4 and reduction[i] > 0.0
            y = played(bank[i])
            after = loudness(bank[i])
            print("clip", i, "drive", drive[i], "reduction", reduction[i], "lufs after", after, "short of the target by", target - after)
            assert after <= target and np.abs(y).max() <= ceiling
        assert reduction[0] > 20.0                                 # the click: from 0.99 times the drive down to the ceiling
        assert same(played(clips["pad"]), kept) and not played(clips["silent"]).any()
        gain_db = C.c_float(0.0)
        dup = (C.c_void_p * 3)(clips["hot"], clips["pad2"], clips["hot"])
        drive[0] = 9.0
        assert zl.libzl_hotpath_clips_level_limited(dup, 3, target, -1.0, 0.0, 0.0, 0, drive, reduction) == _abi.ZLHIP_ERR_INVALID and drive[0] == 9.0
        assert zl.libzl_hotpath_clips_level_limited(arr, 6, float("nan"), -1.0, 0.0, 0.0, 0, drive, reduction) == _abi.ZLHIP_ERR_INVALID
        assert zl.libzl_hotpath_clips_level_limited(arr, 6, target, 1.0, 0.0, 0.0, 0, drive, reduction) == _abi.ZLHIP_ERR_INVALID
        assert zl.libzl_hotpath_clips_level_limited(None, 0, target, -1.0, 0.0, 0.0, 0, None, None) == 0
        for clip in clips.values():
            zl.ClipAudioSource_destroy(clip)
    finally:
        zl.shutdownJuce()
