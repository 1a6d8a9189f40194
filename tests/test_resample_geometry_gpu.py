"""Sample-rate conversion on the device, every path of the kernel and every limit of the table (zl_resample.hip, zl_resample.h;
DESIGN.md section 11).  tests/test_resample_gpu.py runs four upsampling ratios to 48000 (64 and 128 taps, M/L <= 2, clips of 1300
frames); here: a tap count that is no multiple of 4 (the two-tap remainder of the tap loop), M = 8 L (the staging at its limit, ten
passes of the staging loop, 512-tap rows), L = 2048 and a table of 262144 floats, the lowest and the highest accepted rate, clips
shorter than the filter, 160 jobs in a call, a clip of 563 workgroups, tables cached across calls, a clip converted twice and to a
rate that is not the engine's, an engine at 44100, a non-finite sample at the new geometries.  Everything is held to the numpy
restatement (tests/resample_ref.py) fed the library's own table, bit for bit -- the clip, its whole extent read back from an arena that
held noise, and zlhip_sound_info_get -- and three ratios to a float64 evaluation of the definition with numpy's own table.
Small engines: 2 buses x 8 voices, 256-frame blocks."""
import numpy as np
import pytest

import resample_ref as rr
from test_resample_gpu import dirty, expected, make, nan_same, play_pair, read, same, source, table, upload, uploaded_extent_is

pytestmark = pytest.mark.gpu
f32, f64, u32, i64 = np.float32, np.float64, np.uint32, np.int64
FT = 48000

# (fs, ft): what the ratio reaches
GRID = [
    (48000, 44100),     # T = 70: the remainder branch of the tap loop
    (88200, 48000),     # T = 118: the remainder branch while downsampling
    (384000, 48000),    # M = 8 L, T = 512: the staging at its limit
    (192000, 44100),    # T = 280, M/L = 4.35
    (51175, 51200),     # L = 2048
    (102375, 51200),    # L * row = 262144: the table at its limit
    (1000, 6000),       # the lowest accepted rate
    (768000, 96000),    # the highest accepted rate
]


def grid_lengths(fs, ft):
    """shorter than the filter (both ends of the taps outside the clip in one lane), around `half`, one frame more than the taps, the
    workgroup edges, and one clip of five workgroups -- in an order that makes short and long jobs neighbours"""
    L, M, half, T, _ = rr.geometry(fs, ft)
    out = [1, 2, half - 1]
    out += rr.lengths_for(fs, ft, 4 * rr.WG + 41)[-1:]             # five workgroups
    out += [half, half + 1, T + 1]
    for N in (255, 256, 257, 513):
        out += rr.lengths_for(fs, ft, N)
    return out


@pytest.fixture(scope="module")
def geo(built):
    s = make()
    yield s
    s.close()


def first_difference(got, ref):
    if got.shape != ref.shape:
        return got.shape, ref.shape
    d = np.flatnonzero(np.ascontiguousarray(got).view(u32).reshape(-1) != np.ascontiguousarray(ref).view(u32).reshape(-1))
    return d[:6], d.size


def holds(s, cid, ref, ft, tag, finite=True):
    """the clip, its whole extent and its info against `ref` (what the restatement gives), bit for bit"""
    N, ch = ref.shape
    info = s.clip_info(cid)
    assert info == {"length": N, "channels": ch, "sample_rate": float(ft), "finite": finite, "rendered": False}, (tag, info)
    got = read(s, cid)
    assert same(got, ref), (tag, first_difference(got, ref))
    ext, want = s.clip_extent(cid), rr.extent(ref)
    assert ext.size == want.size >= (N + 8) * ch and not want[N * ch:].any()
    assert same(ext, want), (tag, first_difference(ext, want))


# ---- the geometry grid ------------------------------------------------------------------------------------------------------------
def test_the_grid_holds_the_geometries_it_is_there_for():
    """so that the grid does not decay: from the restatement's geometry, without the device"""
    geos = {r: rr.geometry(*r) for r in GRID}
    assert all(g is not None for g in geos.values())
    assert [r for r, g in geos.items() if g[3] % 4 == 2] == [(48000, 44100), (88200, 48000)]
    assert geos[(48000, 44100)][3] == 70 and geos[(88200, 48000)][3] == 118 and geos[(192000, 44100)][3] == 280
    staged = {r: max(c for n in grid_lengths(*r) for c in rr.staged_counts(r[0], r[1], n)) for r in GRID}
    assert rr.STAGE_FRAMES == 2553 and max(staged.values()) == staged[(384000, 48000)] == rr.STAGE_FRAMES - 1, staged
    assert geos[(384000, 48000)][:4] == (1, 8, 256, 512)
    assert geos[(51175, 51200)][0] == 2048 and geos[(102375, 51200)][0] == 2048
    assert geos[(102375, 51200)][0] * geos[(102375, 51200)][4] == 262144
    assert min(min(r) for r in GRID) == 1000 and max(max(r) for r in GRID) == 768000
    for r in GRID:
        L, M, half, T, _ = geos[r]
        ns = grid_lengths(*r)
        assert min(ns) == 1 and any(n < half for n in ns if n > 2) and T + 1 in ns
        assert max(rr.out_frames(r[0], r[1], n) for n in ns) > 4 * rr.WG          # five workgroups


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("fs,ft", GRID)
def test_a_grid_ratio_equals_the_restatement_bit_for_bit(geo, fs, ft, ch):
    """all the lengths of the ratio in one call, so that the workgroups of short and long jobs are neighbours"""
    s = geo
    dirty(s, 120000)                                               # (the 8:1 stereo case takes 55 K floats)
    rng = np.random.default_rng(fs * 3 + ft + ch)
    ns = grid_lengths(fs, ft)
    srcs = [source(rng, n, ch) for n in ns]
    ids = [upload(s, x, fs) for x in srcs]
    try:
        s.convert_clips(ids, ft)
        for cid, x, n in zip(ids, srcs, ns):
            ref = expected(x, fs, ft)
            assert ref.shape[0] == rr.out_frames(fs, ft, n)
            holds(s, cid, ref, ft, (fs, ft, ch, n))
    finally:
        for cid in ids:
            s.unregister_clip(cid)


# ---- against float64 --------------------------------------------------------------------------------------------------------------
def convert64(fs, ft, x):
    """(y, S): y[j] = sum over t of h64[p][t] * x[i - half + 1 + t] and S[j] = the sum of the terms' magnitudes, in float64 with
    numpy's own table (rr.design64)"""
    L, M, half, T, _ = rr.geometry(fs, ft)
    h = rr.design64(fs, ft)
    n, ch = x.shape
    N = rr.out_frames(fs, ft, n)
    xp = np.zeros((n + 2 * half, ch), f64)
    xp[half:half + n] = x.astype(f64)
    q = np.arange(N, dtype=i64) * M
    i, p = q // L, q % L
    y, S = np.zeros((N, ch), f64), np.zeros((N, ch), f64)
    for t in range(T):
        m = h[p, t][:, None] * xp[i + 1 + t]
        y += m
        S += np.abs(m)
    return y, S


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("fs,ft", [(48000, 44100), (384000, 48000), (102375, 51200)])
def test_the_device_against_a_float64_evaluation_of_the_definition(geo, fs, ft, ch):
    """numpy's table, float64 sums: it backs up the bit-exact grid against a mistake the kernel and the restatement share (a wrong
    table, phase or tap offset).  The bound is the forward error of T rounded multiplies and T rounded adds over fp32-rounded
    coefficients plus underflow, |y - y64| <= (T + 2) 2^-24 sum|h64 x| + T (2^-149 + 1e-12 max|x|): derived, not measured"""
    s = geo
    L, M, half, T, _ = rr.geometry(fs, ft)
    rng = np.random.default_rng(fs + ft * 5 + ch)
    ns = [half - 1, T + 1, rr.lengths_for(fs, ft, 2 * rr.WG + 77)[-1]]
    srcs = [source(rng, n, ch) for n in ns]
    ids = [upload(s, x, fs) for x in srcs]
    try:
        s.convert_clips(ids, ft)
        for cid, x, n in zip(ids, srcs, ns):
            got = read(s, cid).astype(f64)
            y, S = convert64(fs, ft, x)
            assert got.shape == y.shape
            bound = (T + 2) * 2.0 ** -24 * S + T * (2.0 ** -149 + 1e-12 * float(np.abs(x).max()))
            err = np.abs(got - y)
            worst = float((err / bound).max())
            print(f"float64 {fs}->{ft} ch={ch} n={n}: worst error / bound = {worst:.4f}")
            assert np.all(err <= bound), (fs, ft, ch, n, worst, np.argwhere(err > bound)[:4])
            assert float(np.abs(y).max()) > 0.0
    finally:
        for cid in ids:
            s.unregister_clip(cid)


# ---- many jobs, a long clip -------------------------------------------------------------------------------------------------------
def test_two_hundred_clips_in_one_call(built):
    """200 clips back to back in an arena that held noise, five source rates dealt round robin, one of them the target's (every fifth
    clip is skipped and stays where it lies, between the sources that leave), lengths 1 .. 600, mono and stereo at random: 160 jobs --
    no power of two -- of one to six workgroups under the bisection"""
    rates = (44100, 96000, FT, 22050, 32000)
    rng = np.random.default_rng(31)
    with make(max_sounds=256) as s:
        dirty(s, 600000)                                           # (sources and conversions take 330 K floats)
        cases = [(rates[k % 5], int(rng.integers(1, 3)), int(rng.integers(1, 601))) for k in range(200)]
        srcs = [source(rng, n, ch) for fs, ch, n in cases]
        ids = [upload(s, x, fs) for x, (fs, ch, n) in zip(srcs, cases)]
        stay = {cid: s.clip_extent(cid) for cid, (fs, ch, n) in zip(ids, cases) if fs == FT}
        assert len(stay) == 40 and all(uploaded_extent_is(s, cid, x) for cid, x, c in zip(ids, srcs, cases) if c[0] == FT)
        wgs = [(rr.out_frames(fs, FT, n) + rr.WG - 1) // rr.WG for fs, ch, n in cases if fs != FT]
        assert len(wgs) == 160 and wgs.count(1) > 40 and wgs.count(3) > 5 and max(wgs) > 3
        s.convert_clips(ids)
        for cid, x, (fs, ch, n) in zip(ids, srcs, cases):
            if fs == FT:
                assert s.clip_info(cid) == {"length": n, "channels": ch, "sample_rate": float(FT), "finite": True, "rendered": False}
                assert same(read(s, cid), x) and same(s.clip_extent(cid), stay[cid]), (cid, n)
            else:
                holds(s, cid, expected(x, fs), FT, (cid, fs, ch, n))


def test_a_clip_of_563_workgroups(built):
    """three seconds of 44.1 kHz stereo (144000 frames at 48000) and the same length in mono at 88200 -> 48000 (T = 118), one call"""
    rng = np.random.default_rng(32)
    n = 3 * 44100
    with make() as s:
        dirty(s, 800000)                                           # (757 K floats; the arena has 1 M)
        a, b = source(rng, n, 2), source(rng, n, 1)
        ia, ib = upload(s, a, 44100), upload(s, b, 88200)
        s.convert_clips([ia, ib])
        ra, rb = expected(a, 44100), expected(b, 88200)
        assert ra.shape == (144000, 2) and (ra.shape[0] + rr.WG - 1) // rr.WG == 563 and rb.shape == (72000, 1)
        holds(s, ia, ra, FT, "44100 stereo")
        holds(s, ib, rb, FT, "88200 mono")


# ---- the host side: cached tables, a second conversion, a foreign target, an engine at 44100 --------------------------------------
def table_bytes(fs, ft):
    L, _, _, _, row = rr.geometry(fs, ft)
    return L * row * 4


def test_cached_tables_across_calls(built):
    """the table of a ratio is made by the first call that asks for it; later calls at the ratio read the cached device table (its
    host copy is gone by then), add nothing to the engine's memory, and a failed call in between takes nothing from them"""
    from libzl_amd import ZlHipError
    rng = np.random.default_rng(33)
    arena = 1 << 20
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        dirty(s, 60000)
        xs = [source(rng, n, ch) for n, ch in ((2000, 2), (1500, 1), (777, 2), (1000, 2), (900, 1))]
        a, b, c, d, g = xs
        ia, ib, ic, ig = upload(s, a, 44100), upload(s, b, 44100), upload(s, c, 44100), upload(s, g, 44100)
        idd = upload(s, d, 96000)
        m0 = s.memory_bytes()
        s.convert_clips([ia])                                      # call A: the 44100 -> 48000 table and the call's records
        mA = s.memory_bytes()
        assert mA[0] - m0[0] >= table_bytes(44100, FT) and mA[1] == m0[1]
        holds(s, ia, expected(a, 44100), FT, "A")
        s.convert_clips([ib])                                      # call B: the cached table
        assert s.memory_bytes() == mA
        holds(s, ib, expected(b, 44100), FT, "B")
        s.convert_clips([ic, idd])                                 # call C: the cached ratio and a new one
        mC = s.memory_bytes()
        assert mC[0] - mA[0] == table_bytes(96000, FT) == 512 and mC[1] == mA[1]
        holds(s, ic, expected(c, 44100), FT, "C cached")
        holds(s, idd, expected(d, 96000), FT, "C new")
        # a call the arena cannot hold, at a ratio new to the engine (22050 -> 48000): its table is made and freed again
        small, big = source(rng, 3000, 1), source(rng, 60000, 2)   # 480 KB; converted 522 KB: the arena (1 MiB) cannot take both
        ismall, ibig = upload(s, small, 22050), upload(s, big, 44100)
        with pytest.raises(ZlHipError):
            s.convert_clips([ismall, ibig])
        assert s.memory_bytes() == mC
        assert same(read(s, ismall), small) and same(read(s, ibig), big)
        assert [s.clip_info(i)["sample_rate"] for i in (ismall, ibig)] == [22050.0, 44100.0]
        s.unregister_clip(ibig)
        s.convert_clips([ig])                                      # after the failure: the cached ratio once more
        assert s.memory_bytes() == mC
        holds(s, ig, expected(g, 44100), FT, "after the failed call")
        for cid, x in ((ia, a), (ib, b), (ic, c)):                 # and what the earlier calls left is still there
            assert same(read(s, cid), expected(x, 44100))


def test_converting_twice_and_to_a_rate_that_is_not_the_engines(built):
    """44100 -> 48000 -> 44100 (1176 -> 1280 -> 1176 frames) and 48000 -> 96000 -> 48000: the restatement applied twice; the info
    carries the last target; every extent the chain left behind is free again (the arena is fixed in size: once the clips are
    released, one clip as large as the arena fits); the clip left at 44100 in the 48000 engine plays through the pitched path like
    its twin uploaded at 44100"""
    rng = np.random.default_rng(34)
    arena = 1 << 18                                                # 65536 floats
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s, make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as direct:
        dirty(s, 30000)
        x, y = source(rng, 1176, 2), source(rng, 1000, 1)
        ix, iy = upload(s, x, 44100), upload(s, y, FT)
        m0 = s.memory_bytes()
        s.convert_clips([ix])                                      # 44100 -> 48000: the engine's rate
        x1 = expected(x, 44100, FT)
        holds(s, ix, x1, FT, "x once")
        m1 = s.memory_bytes()
        s.convert_clips([iy], 96000)                               # 48000 -> 96000: a foreign target
        y1 = expected(y, FT, 96000)
        assert y1.shape[0] == 2000
        holds(s, iy, y1, 96000, "y once")
        s.convert_clips([ix, iy], 44100)                           # one call, two ratios: x back to 44100, y from 96000 to 44100
        x2 = expected(x1, FT, 44100)
        y44 = expected(y1, 96000, 44100)
        assert x1.shape[0] == 1280 and x2.shape[0] == 1176
        holds(s, ix, x2, 44100, "x twice")
        holds(s, iy, y44, 44100, "y to 44100")
        # a third clip in a chain of its own: 48000 -> 96000 -> 48000
        z = source(rng, 1000, 2)
        iz = upload(s, z, FT)
        s.convert_clips([iz], 96000)
        s.convert_clips([iz])
        z2 = expected(expected(z, FT, 96000), 96000, FT)
        assert z2.shape[0] == 1000
        holds(s, iz, z2, FT, "z twice")
        # memory: the tables of the four ratios and the first call's records, nothing else -- as an engine that was handed the
        # results directly, tables aside
        for v, rate in ((x2, 44100), (y44, 44100), (z2, FT)):
            upload(direct, v, rate)
        tables = sum(table_bytes(a, b) for a, b in ((FT, 96000), (FT, 44100), (96000, 44100), (96000, FT)))
        mS, mD = s.memory_bytes(), direct.memory_bytes()
        assert mD == m0 and mS[1] == mD[1] and mS[0] - mD[0] == (m1[0] - m0[0]) + tables, (m0, m1, mS, mD)
        # the pitched path: the converted clip at 44100 next to its twin uploaded at 44100
        twin = upload(s, x2, 44100)
        assert s.clip_info(ix) == s.clip_info(twin)
        bus, peaks, levels, reports = play_pair(s, ix, twin)
        assert len(np.unique(bus[0][0])) > 600 and same(bus[0], bus[1])
        assert np.array_equal(peaks[:, 0], peaks[:, 1]) and levels[0] == levels[1] and reports[0] == reports[1]
        assert reports[0][0][0] == 1
    # the old extents are back in the arena: with every clip released, a clip of the arena's size fits again
    with make(sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:
        ix, iz = upload(s, x, 44100), upload(s, z, FT)
        s.convert_clips([ix])
        s.convert_clips([iz], 96000)
        s.convert_clips([ix, iz], 44100)
        holds(s, ix, x2, 44100, "x twice, again")
        s.unregister_clip(ix)
        s.unregister_clip(iz)
        whole = np.zeros(arena // 4 - 8, f32)
        iw = s.register_clip(whole, None, float(FT))
        assert s.clip_extent(iw).size == arena // 4 and s.memory_bytes()[1] == arena


def test_an_engine_at_44100(built):
    """the engine's own rate as the target where it is not 48000: a 48000 Hz clip becomes T = 70 output; looped for 8 blocks under
    clocks at 44100 it equals the restatement's output uploaded at 44100, and it steps by one frame per frame"""
    from scenario import engine_cmd, play_cmd
    from libzl_amd.engine import synthetic_clocks
    from test_resample_gpu import set_loop
    rng = np.random.default_rng(35)
    rate = 44100.0
    with make(playback_sample_rate=rate) as s:
        dirty(s, 20000)
        x = source(rng, 1280, 2)
        cid = upload(s, x, FT)
        s.convert_clips([cid])                                     # no rate: the engine's
        ref = expected(x, FT, 44100)
        assert ref.shape[0] == 1176 and rr.geometry(FT, 44100)[3] == 70
        holds(s, cid, ref, 44100, "48000 -> 44100")
        twin = upload(s, ref, rate)
        assert s.clip_info(cid) == s.clip_info(twin)
        for bus, c in ((0, cid), (1, twin)):
            set_loop(s, c, 1176, rate)                             # a loop of 1/64 s: 689 frames
            assert s.handle_clip_command(engine_cmd(**play_cmd(c, midi_channel=bus - 2, loop=True, note=60, volume=0.8)), 0) == 1
        fields = ("playing", "valid", "gain", "progress", "source_sample_position")
        heard, where = [], []
        for first, blocks in ((0, 1), (1, 1), (2, 6)):             # 8 blocks; the first two one by one: the loop has not wrapped yet
            s.render_batch(blocks, 256, synthetic_clocks(blocks, 256, rate, start_block=first))
            bus = s.read_bus()
            assert same(bus[0], bus[1]), first
            assert np.array_equal(s.block_peaks()[:, 0], s.block_peaks()[:, 1])
            rep = s.voice_reports()
            reports = [[tuple(getattr(rep[b * 8 + v], f) for f in fields) for v in range(8)] for b in range(2)]
            assert reports[0] == reports[1] and reports[0][0][0] == 1, (first, reports[0][0], reports[1][0])
            heard.append(bus[0])
            where.append(reports[0][0][4])
        assert len(np.unique(np.concatenate(heard, axis=1)[0])) > 600   # (it moves through the loop)
        assert where[1] - where[0] == 256.0, where                 # the unit step: a clip still at 48000 would move 278.6 frames
        assert 0 < where[2] < 690, where                           # still looping, inside the loop


# ---- a non-finite sample ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,ft,n,at", [(48000, 44100, 1500, 700), (384000, 48000, 6000, 3000)])
def test_a_non_finite_sample_at_the_new_geometries(geo, fs, ft, n, at):
    """one +inf in a stereo F32 clip, behind other jobs of the call (its verdict word is not the first): finite is False for it and
    True for the others; the other channel and every frame farther than `half` input frames from it are bit-exact; NaNs are NaNs"""
    from libzl_amd import _abi
    s = geo
    L, M, half, T, _ = rr.geometry(fs, ft)
    rng = np.random.default_rng(36 + fs)
    others = [source(rng, k, ch) for k, ch in ((300, 2), (T + 1, 1), (900, 2))]
    x = source(rng, n, 2)
    x[at, 0] = np.inf
    ids = [upload(s, o, fs) for o in others[:2]]
    cid = s.register_clip_pcm(np.ascontiguousarray(x), _abi.PCM_F32, 2, float(fs))
    ids += [cid, upload(s, others[2], fs)]
    try:
        assert s.clip_info(cid)["finite"] is False
        s.convert_clips(ids, ft)
        for i, o in zip(ids[:2] + ids[3:], others):
            holds(s, i, expected(o, fs, ft), ft, (fs, ft, o.shape))   # (finite: True)
        ref = expected(x, fs, ft)
        N = ref.shape[0]
        info = s.clip_info(cid)
        assert info == {"length": N, "channels": 2, "sample_rate": float(ft), "finite": False, "rendered": False}, info
        got = read(s, cid)
        far = np.abs((np.arange(N, dtype=i64) * M) // L - at) > half
        assert far.sum() > N // 2 and (~far).sum() >= 2 * (half * L // M) - 2
        assert same(got[far], ref[far]) and same(got[:, 1], ref[:, 1]) and nan_same(got, ref)
        assert not np.isfinite(got[~far, 0]).all() and np.isfinite(got[far]).all()
        ext = s.clip_extent(cid)
        assert nan_same(ext, rr.extent(ref)) and not ext[N * 2:].any()
    finally:
        for i in ids:
            s.unregister_clip(i)
