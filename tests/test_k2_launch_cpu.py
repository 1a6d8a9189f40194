"""Which K2 kernel a plan window gets, with what grid, and how a call is cut into windows (libzl_amd/csrc/zl_launch.h), CPU tier: the header
built for the host (tests/cpu_harness/launch_host.cpp).  A table of known answers -- derived by hand from the launcher and the call path as they
stood before the header existed -- and invariants over a sweep of shapes.  zlhip_render_batch and zl_launch_render decide nothing themselves:
what this file holds is what runs.  The kernels' results are held on the GPU (tests/test_k2_tail.py, test_k2_pair.py, test_k2_phase_order.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from libzl_amd import build

IN = ("mode", "N", "K", "B", "groups", "NB", "staged", "trace", "ongrid", "fan", "host_out", "order_mode", "call_blocks", "bounce", "order_table",
      "pair_mode", "cheap")
OUT = ("kernel", "bpw", "staged", "gx", "gy", "gz", "threads", "dyn_lds", "tail_from", "tail_split", "tail_nb", "order", "scans_levels")
SW = ("tail", "tail_min", "pad", "pad_hermite", "pair_pad", "pair_static_lds", "pair_lds", "st_ring")
RENDER, PHASE_RENDER, PAIR_RENDER, PAIR_PHASE_RENDER = 0, 1, 2, 3
PAIR_LDS, ST_RING = 18432, 4 * 6 * 1024          # ZL_K2_PAIR_LDS; four waves' rings of ZL_ST_D slots of ZL_ST_SLOT bytes (zl_kernels.hip)
PAIR_STATIC = 12504                              # any static LDS size of the pair kernels below ZL_K2_PAIR_LDS
DEFAULT_SW = dict(tail=1, tail_min=2048, pad=-1, pad_hermite=-1, pair_pad=-1, pair_static_lds=PAIR_STATIC, pair_lds=PAIR_LDS, st_ring=ST_RING)
# the headline's window: mode 0, 8192 blocks of 256 frames, 8 buses of 128 voices, nothing switched on
BASE = dict(mode=0, N=256, K=8192, B=8, groups=1, NB=1, staged=0, trace=0, ongrid=1, fan=0, host_out=0, order_mode=0, call_blocks=None, bounce=0,
            order_table=1, pair_mode=0, cheap=0)

_lib = None
_pair = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_launch_harness())
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        l.zllh_launch.restype = None
        l.zllh_launch.argtypes = [C.c_int, ip, dp, ip, ip]
        l.zllh_narrow_buses.restype = C.c_int
        l.zllh_narrow_buses.argtypes = [C.c_int] * 5
        l.zllh_whole_waves.restype = C.c_int
        l.zllh_whole_waves.argtypes = [C.c_int]
        l.zllh_windows.restype = C.c_int
        l.zllh_windows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong] + [C.c_int] * 5 + [ip, C.c_int]
        l.zllh_env_switches.restype = None
        l.zllh_env_switches.argtypes = [ip]
        _lib = l
    return _lib


def pair_shape(*args):
    """zl_pair_shape through the gate's own harness (tests/cpu_harness/pair_host.cpp)"""
    global _pair
    if _pair is None:
        _pair = C.CDLL(build.build_pair_harness())
        _pair.zlpg_shape.restype = C.c_int
        _pair.zlpg_shape.argtypes = [C.c_uint] + [C.c_int] * 9
    return _pair.zlpg_shape(*args)


def launch_many(rows, loops=None, **sw):
    """rows: int array [n][len(IN)] -> dict of OUT columns"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = rows.shape[0]
    loops = np.zeros(n, dtype=np.float64) if loops is None else np.ascontiguousarray(loops, dtype=np.float64)
    s = dict(DEFAULT_SW); s.update(sw)
    swv = np.array([s[k] for k in SW], dtype=np.int32)
    out = np.empty((n, len(OUT)), dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib().zllh_launch(n, rows.ctypes.data_as(ip), loops.ctypes.data_as(dp), swv.ctypes.data_as(ip), out.ctypes.data_as(ip))
    return {k: out[:, i] for i, k in enumerate(OUT)}


def launch(sw=None, loop=0.0, **kw):
    """one launch: BASE with kw; NB from zl_k2_narrow_buses(VPB) unless given; want_order / want_pair switch the gates to `wherever the shape allows`"""
    a = dict(BASE)
    vpb = kw.pop("VPB", 128)
    if kw.pop("want_order", False):
        a["order_mode"] = 2
    if kw.pop("want_pair", False):
        a["pair_mode"] = 2
    a.update(kw)
    if a["call_blocks"] is None:
        a["call_blocks"] = a["K"]
    if "NB" not in kw:
        a["NB"] = lib().zllh_narrow_buses(a["call_blocks"], a["groups"], vpb, a["B"], a["N"])
    o = launch_many([[a[k] for k in IN]], [loop], **(sw or {}))
    r = {k: int(v[0]) for k, v in o.items()}
    r["NB"] = a["NB"]
    return r


def has(r, **want):
    got = {k: r[k] for k in want}
    assert got == want, (got, want)


def windows(nblocks, nframes, windowFrames, mul=1, twoSets=1, behindPrev=0, windowBlocks=0, windowCap=1 << 30, first=-1):
    args = (nblocks, nframes, windowBlocks, windowFrames, windowCap, mul, twoSets, behindPrev, first)
    n = lib().zllh_windows(*args, None, 0)
    out = (C.c_int * (2 * n))()
    assert lib().zllh_windows(*args, out, n) == n
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)]


# ---- one bus per workgroup (B = 8, VPB = 128, groups = 1) ----------------------------------------------------------------------------
def test_one_bus_per_workgroup():
    r = launch()
    has(r, kernel=RENDER, bpw=1, staged=0, threads=256, gx=1, gy=8192, gz=8, dyn_lds=10240, tail_from=0, tail_split=1, order=0, scans_levels=1)
    has(launch(mode=4), kernel=RENDER, bpw=1, staged=0, threads=256, gx=1, gy=8192, gz=8, dyn_lds=0, scans_levels=1)
    has(launch(want_order=True), kernel=PHASE_RENDER, bpw=1, staged=0, threads=256, gx=1, gy=8192, gz=8, dyn_lds=10240, order=1)
    has(launch(want_order=True, mode=5), kernel=PHASE_RENDER, dyn_lds=0, order=1)
    has(launch(want_order=True, order_table=0), kernel=RENDER, order=0)        # no table to read the order from: the plain kernel
    has(launch(want_pair=True), kernel=PAIR_RENDER, threads=128, gx=1, gy=8192, gz=8, dyn_lds=PAIR_LDS - PAIR_STATIC, order=0, scans_levels=1, tail_from=0)
    has(launch(want_pair=True, want_order=True), kernel=PAIR_PHASE_RENDER, threads=128, gx=1, gy=8192, gz=8, dyn_lds=PAIR_LDS - PAIR_STATIC, order=1)
    has(launch(want_pair=True, sw=dict(pair_static_lds=20000)), kernel=PAIR_RENDER, dyn_lds=0)
    has(launch(want_pair=True, sw=dict(pair_pad=4096)), kernel=PAIR_RENDER, dyn_lds=4096)
    has(launch(want_pair=True, sw=dict(pair_pad=0)), kernel=PAIR_RENDER, dyn_lds=0)
    has(launch(sw=dict(pad=0)), dyn_lds=0)
    has(launch(sw=dict(pad=4096, pad_hermite=2048)), dyn_lds=4096)
    has(launch(mode=4, sw=dict(pad=4096, pad_hermite=2048)), dyn_lds=2048)


# every single condition of zl_pair_shape broken in turn: the 256-lane kernel that launch had before (with and without the order)
PAIR_BREAKS = [dict(mode=1), dict(mode=2), dict(mode=4), dict(N=255), dict(N=512), dict(N=128), dict(K=1, call_blocks=2), dict(NB=2), dict(groups=2),
               dict(staged=1), dict(trace=1), dict(fan=1), dict(host_out=1), dict(ongrid=0)]


@pytest.mark.parametrize("brk", PAIR_BREAKS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_a_launch_outside_the_pair_shape_keeps_its_kernel(brk):
    for order in (False, True):
        plain = launch(want_order=order, **brk)
        r = launch(want_pair=True, want_order=order, **brk)
        assert r == plain, brk
        assert r["kernel"] in (RENDER, PHASE_RENDER) and r["kernel"] == (PHASE_RENDER if r["order"] else RENDER)
        assert r["threads"] != 128 or brk.get("N", 256) <= 128


def test_the_pair_switch():
    """ZL_K2_PAIR: 0 never, 1 auto (every playing voice cheap to plan), 2 wherever the shape allows"""
    for sw, cheap, want in [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1), (2, 0, 1), (2, 1, 1), (3, 1, 0)]:
        assert (launch(pair_mode=sw, cheap=cheap)["kernel"] == PAIR_RENDER) == bool(want), (sw, cheap)


def test_the_order_switch():
    """ZL_K2_PHASE_ORDER: 0 off, 1 auto (blocks of 256 frames or more, no bounce, the window longer than the shortest playing loop), 2 wherever
    the shape allows"""
    loop = 88200.0
    assert launch(order_mode=1, loop=loop)["order"] == 1                       # 8192 * 256 frames > the loop
    assert launch(order_mode=1, loop=loop, K=344, call_blocks=8192)["order"] == 0   # 88064 frames: no longer than the loop
    assert launch(order_mode=1, loop=loop, K=345, call_blocks=8192)["order"] == 1
    assert launch(order_mode=1, loop=float("inf"))["order"] == 0               # a playing voice that is not cheap to plan
    assert launch(order_mode=1, loop=loop, bounce=1)["order"] == 0 and launch(order_mode=2, bounce=1)["order"] == 1
    assert launch(order_mode=1, loop=loop, N=200, VPB=128)["order"] == 0 and launch(order_mode=2, N=200)["order"] == 1
    assert launch(order_mode=0, loop=loop)["order"] == 0 and launch(order_mode=3, loop=loop)["order"] == 0
    assert launch(order_mode=2, K=1, call_blocks=1)["order"] == 0              # a single real-time block
    assert launch(order_mode=2, K=1, call_blocks=2)["order"] == 1              # a one-block window of a batch


# ---- short and odd blocks ----------------------------------------------------------------------------------------------------------------
def test_short_and_odd_blocks():
    for z in (1, 8):
        has(launch(N=64, K=100, B=z, want_order=True), kernel=RENDER, bpw=4, staged=0, threads=256, gx=1, gy=25, gz=z, dyn_lds=0, order=0, scans_levels=1)
    has(launch(N=128, K=101, want_order=True), kernel=RENDER, bpw=2, threads=256, gx=1, gy=51, dyn_lds=0, order=0, scans_levels=1)
    has(launch(N=64, K=1), bpw=1, threads=64, gx=1, gy=1, dyn_lds=10240, scans_levels=1)
    has(launch(N=128, K=1), bpw=1, threads=128, gx=1, gy=1, dyn_lds=10240, scans_levels=1)
    has(launch(N=128, K=1, mode=4), bpw=1, threads=128, dyn_lds=0)
    for n, threads in [(16, 64), (48, 64), (100, 128), (200, 256), (1, 64), (65, 128), (129, 192), (192, 192), (193, 256), (255, 256)]:
        has(launch(N=n, K=10), kernel=RENDER, bpw=1, threads=threads, gx=1, gy=10, dyn_lds=10240, scans_levels=1)
        assert lib().zllh_whole_waves(n) == threads
    for n, gx in [(300, 2), (441, 2), (1000, 4), (4096, 16), (257, 2), (512, 2), (513, 3)]:
        has(launch(N=n, K=10), kernel=RENDER, bpw=1, threads=256, gx=gx, gy=10, gz=8, dyn_lds=10240, scans_levels=0)
        assert lib().zllh_whole_waves(n) == 256


def test_mix_groups():
    r = launch(groups=3, want_order=True, want_pair=True)
    has(r, kernel=RENDER, bpw=1, gz=24, gy=8192, scans_levels=0, order=0, tail_from=0)
    has(launch(groups=3, B=5, N=64), bpw=4, gz=15, scans_levels=0)


# ---- narrow buses and the split tail (VPB = 8 unless stated, N = 256, K = 2100) ------------------------------------------------------------
@pytest.mark.parametrize("B,VPB,NB,gz,split,tail_nb", [
    (12, 8, 12, 1, 4, 3), (8, 8, 8, 1, 4, 2), (16, 8, 16, 1, 4, 4), (4, 8, 4, 1, 4, 1), (10, 8, 10, 1, 2, 5), (6, 16, 6, 1, 2, 3), (2, 16, 2, 1, 2, 1),
    (7, 8, 7, 1, 1, 7), (24, 8, 16, 2, 1, 16), (8, 12, 1, 8, 1, 1), (8, 72, 1, 8, 1, 1), (3, 64, 2, 2, 1, 2), (2, 64, 2, 1, 2, 1), (1, 8, 1, 1, 1, 1)])
def test_narrow_buses_and_the_split_tail(B, VPB, NB, gz, split, tail_nb):
    r = launch(B=B, VPB=VPB, K=2100)
    assert r["NB"] == NB
    if split > 1:
        has(r, kernel=RENDER, bpw=1, threads=256, gx=1, gz=1, tail_split=split, tail_nb=tail_nb, tail_from=1575, gy=1575 + 525 * split, scans_levels=1)
    else:
        has(r, kernel=RENDER, bpw=1, gx=1, gz=gz, gy=2100, tail_from=0, tail_split=1, tail_nb=NB)


def test_narrow_bus_packing():
    nb = lib().zllh_narrow_buses
    assert nb(2100, 1, 8, 12, 256) == 12 and nb(2100, 1, 8, 24, 256) == 16 and nb(2100, 1, 16, 24, 256) == 8 and nb(2100, 1, 64, 8, 256) == 2
    assert nb(2100, 1, 8, 12, 64) == 12 and nb(2100, 1, 8, 12, 100) == 12
    # a single block, mix groups, a width that is no multiple of 8 or above 64, more than one frame tile: one bus per workgroup
    assert nb(1, 1, 8, 12, 256) == 1 and nb(2100, 2, 8, 12, 256) == 1 and nb(2100, 1, 12, 12, 256) == 1 and nb(2100, 1, 72, 12, 256) == 1
    assert nb(2100, 1, 128, 12, 256) == 1 and nb(2100, 1, 8, 12, 257) == 1 and nb(2100, 1, 8, 12, 300) == 1 and nb(2100, 1, 8, 1, 256) == 1


def test_the_tail_further():
    nb12 = dict(B=12, VPB=8)
    has(launch(K=8192, **nb12), tail_from=7552, tail_split=4, tail_nb=3, gy=10112)       # T = 640: half a generation of workgroups
    r = launch(K=60000, **nb12)
    has(r, tail_from=59360, gy=61920)
    assert r["gy"] < 65536
    has(launch(K=2048, **nb12), tail_from=1536, gy=1536 + 4 * 512)
    has(launch(K=2047, **nb12), tail_from=0, gy=2047, tail_split=1, tail_nb=12)
    has(launch(K=2047, sw=dict(tail_min=24), **nb12), tail_from=2047 - 511, tail_split=4, gy=2047 - 511 + 4 * 511)
    has(launch(K=24, sw=dict(tail_min=24), **nb12), tail_from=18, tail_split=4, tail_nb=3, gy=18 + 24)
    has(launch(K=23, sw=dict(tail_min=24), **nb12), tail_from=0, gy=23)
    has(launch(K=8192, sw=dict(tail=0), **nb12), tail_from=0, tail_split=1, tail_nb=12, gy=8192)
    for n in (192, 100, 256, 16):
        has(launch(K=2100, N=n, **nb12), tail_from=1575, tail_split=4, threads=lib().zllh_whole_waves(n))
    r = launch(K=2100, N=300, **nb12)                                                # nframes <= 256 fails: NB = 1
    assert r["NB"] == 1
    has(r, tail_from=0, gx=2, gz=12)
    has(launch(K=2100, N=64, **nb12), bpw=4, tail_from=0, gy=525)                    # several blocks per workgroup: no tail
    has(launch(K=2100, staged=1, **nb12), staged=1, tail_from=0, gy=2100, dyn_lds=ST_RING)
    has(launch(K=2100, staged=1, N=192, **nb12), staged=0, tail_from=1575)           # (staged asked for, the register kernel launched: tailed)
    has(launch(K=2100, want_order=True, **nb12), kernel=PHASE_RENDER, order=1, tail_from=1575, tail_split=4, gz=1, gy=3675, dyn_lds=10240)
    has(launch(K=2100, want_pair=True, **nb12), kernel=RENDER, tail_from=1575)


def test_the_clamp_of_the_tail_threshold(monkeypatch):
    """the launcher's switches as the environment sets them (read once per process by the library; here on every call)"""
    def env():
        out = (C.c_int * 5)()
        lib().zllh_env_switches(out)
        return dict(zip(SW[:5], out))
    for k in ("ZL_K2_TAIL", "ZL_K2_TAIL_MIN_BLOCKS", "ZL_K2_LDS_PAD", "ZL_K2_LDS_PAD_HERMITE", "ZL_K2_PAIR_LDS_PAD"):
        monkeypatch.delenv(k, raising=False)
    assert env() == {k: DEFAULT_SW[k] for k in SW[:5]}
    for text, want in [("24", 24), ("8", 8), ("7", 8), ("0", 8), ("-5", 8), ("4096", 4096)]:
        monkeypatch.setenv("ZL_K2_TAIL_MIN_BLOCKS", text)
        assert env()["tail_min"] == want
    monkeypatch.setenv("ZL_K2_TAIL", "0"); monkeypatch.setenv("ZL_K2_LDS_PAD", "0")
    monkeypatch.setenv("ZL_K2_LDS_PAD_HERMITE", "2048"); monkeypatch.setenv("ZL_K2_PAIR_LDS_PAD", "512")
    assert env() == dict(tail=0, tail_min=4096, pad=0, pad_hermite=2048, pair_pad=512)
    nb12 = dict(B=12, VPB=8)
    has(launch(K=8, sw=dict(tail_min=8), **nb12), tail_from=6, tail_split=4, gy=6 + 8)
    has(launch(K=7, sw=dict(tail_min=8), **nb12), tail_from=0)


# ---- LDS-staged ----------------------------------------------------------------------------------------------------------------------------
def test_staged():
    for n, bpw in [(256, 1), (128, 2), (64, 4)]:
        has(launch(staged=1, N=n, K=100, want_order=True), kernel=RENDER, staged=1, bpw=bpw, threads=256, gx=1, gy=(100 + bpw - 1) // bpw, dyn_lds=ST_RING, order=0)
    has(launch(staged=1, N=512, K=100), staged=1, bpw=1, gx=2, dyn_lds=ST_RING, scans_levels=0)
    has(launch(staged=1, mode=4), staged=1, dyn_lds=ST_RING)
    has(launch(staged=1, K=1), kernel=RENDER, staged=0, bpw=1, threads=256, dyn_lds=10240)
    has(launch(staged=1, N=100, K=100), kernel=RENDER, staged=0, bpw=1, threads=128, dyn_lds=10240)
    has(launch(staged=1, N=64, K=1), staged=0, bpw=1, threads=64, dyn_lds=10240)


# ---- windows ---------------------------------------------------------------------------------------------------------------------------------
def test_windows():
    assert windows(2048, 256, 524288) == [(0, 2048)]
    assert windows(1, 256, 524288) == [(0, 1)] and windows(100, 256, 524288) == [(0, 100)]
    want = [512, 2048, 2048, 2048, 1536]
    got = windows(8192, 256, 524288)
    assert [n for _, n in got] == want and [k for k, _ in got] == [0, 512, 2560, 4608, 6656]
    assert [n for _, n in windows(8192, 256, 524288, behindPrev=1)] == [2048] * 4
    assert [n for _, n in windows(8192, 256, 524288, twoSets=0)] == [2048] * 4
    assert windows(8192, 256, 524288, mul=4) == [(0, 8192)]
    assert [n for _, n in windows(66000, 256, 16 << 20)] == [16384, 49616]            # W capped at 60000
    assert [n for _, n in windows(66000, 256, 16 << 20, behindPrev=1)] == [60000, 6000]
    assert [n for _, n in windows(8192, 256, 524288, windowBlocks=3000)] == [512, 3000, 3000, 1680]     # the override wins
    assert [n for _, n in windows(8192, 256, 524288, windowBlocks=3000, behindPrev=1)] == [3000, 3000, 2192]
    assert [n for _, n in windows(8192, 256, 524288, windowCap=1000, behindPrev=1)] == [1000] * 8 + [192]   # the cap wins
    assert [n for _, n in windows(8192, 256, 524288, windowCap=300)][:3] == [300, 300, 300]              # ... over the first window too
    assert [n for _, n in windows(8192, 256, 524288, first=65536)] == [256, 2048, 2048, 2048, 1792]      # ZL_FIRST_WINDOW_FRAMES
    assert [n for _, n in windows(8192, 256, 524288, first=0)][:2] == [1, 2048]
    assert [n for _, n in windows(300, 1 << 20, 524288)] == [1] * 300                                   # a window is never empty
    assert [n for _, n in windows(5000, 1 << 19, 1 << 40, behindPrev=1)] == [2048, 2048, 904]           # 2^30 frames per window at the most


def test_windows_invariants():
    for nblocks, nframes, wf, mul, two, behind, wb, cap, first in itertools.product(
            (1, 2049, 8192, 60001, 200000), (1, 100, 256, 4096), (65536, 524288, 1 << 34), (1, 4), (0, 1), (0, 1), (0, 777, 70000), (5000, 1 << 30),
            (-1, 1000000)):
        w = windows(nblocks, nframes, wf, mul=mul, twoSets=two, behindPrev=behind, windowBlocks=wb, windowCap=cap, first=first)
        assert w[0][0] == 0 and sum(n for _, n in w) == nblocks
        assert all(n >= 1 and n <= 60000 and n <= cap and n * nframes <= 1 << 30 for _, n in w)
        assert all(w[i][0] + w[i][1] == w[i + 1][0] for i in range(len(w) - 1))
        assert len({n for _, n in w[1:-1]}) <= 1                                    # full windows between the first and the last


# ---- invariants over a sweep -------------------------------------------------------------------------------------------------------------------
def _sweep(ns, ks, seed):
    """every N of ns x K of ks, with B, VPB, groups, mode and every flag drawn per row (all values of each occur thousands of times)"""
    rng = np.random.default_rng(seed)
    N, K = [a.ravel() for a in np.meshgrid(np.asarray(ns), np.asarray(ks), indexing="ij")]
    n = N.size
    pick = lambda vals: rng.choice(np.asarray(vals), size=n)
    B, VPB, groups = pick([1, 2, 3, 4, 7, 8, 12, 16, 24, 64, 128]), pick([8, 16, 24, 64, 128]), pick([1, 1, 1, 2, 3, 8])
    call = np.where(pick([0, 1]) == 1, K, K + pick([0, 1, 5000]))                  # the window is the call, or a part of it
    nbf = lib().zllh_narrow_buses
    NB = np.array([nbf(int(c), int(g), int(v), int(b), int(f)) for c, g, v, b, f in zip(call, groups, VPB, B, N)], dtype=np.int32)
    cols = dict(mode=pick(range(8)), N=N, K=K, B=B, groups=groups, NB=NB, staged=pick([0, 0, 1]), trace=pick([0, 0, 0, 1]), ongrid=pick([0, 1, 1, 1]),
                fan=pick([0, 0, 0, 1]), host_out=pick([0, 0, 0, 1]), order_mode=pick([0, 1, 2, 2]), call_blocks=call, bounce=pick([0, 0, 0, 1]),
                order_table=pick([0, 1, 1, 1]), pair_mode=pick([0, 1, 2, 2]), cheap=pick([0, 1]))
    loops = rng.choice(np.array([0.0, 44100.0, 1e7, np.inf]), size=n)
    return cols, loops, VPB


@pytest.mark.parametrize("tail_min", [2048, 24])
def test_invariants_over_a_sweep(tail_min):
    ks = sorted(set([1, 2, 3, 7, 8, 23, 24, 25, 100, 101, 255, 256, 2047, 2048, 2049, 2100, 2560, 8192, 16384, 30000, 59999, 60000]))
    # (every block length up to 4096 frames; the lengths of one frame tile, where most of the forms live, eight times more)
    c, loops, VPB = _sweep(list(range(1, 4097)) + list(range(1, 257)) * 8, ks, 1234 + tail_min)
    o = launch_many(np.stack([c[k] for k in IN], axis=1), loops, tail_min=tail_min)
    N, K, NB, B = c["N"], c["K"], c["NB"], c["B"]
    pair = (o["kernel"] == PAIR_RENDER) | (o["kernel"] == PAIR_PHASE_RENDER)
    tailed = o["tail_from"] > 0
    assert (o["gy"] < 65536).all() and (o["gy"] >= 1).all() and (o["gx"] >= 1).all() and (o["gz"] >= 1).all() and (o["gx"] <= 16).all()
    assert (o["threads"] % 64 == 0).all() and (o["threads"] >= 64).all() and (o["threads"] <= 256).all()
    assert (o["threads"][pair] == 128).all()
    assert np.isin(o["bpw"], (1, 2, 4)).all() and (o["bpw"] * N <= 256)[o["bpw"] > 1].all()
    one = (o["bpw"] == 1) & ~pair
    assert (o["gx"][one].astype(np.int64) * o["threads"][one] >= N[one]).all()
    assert ((o["gx"][one].astype(np.int64) - 1) * o["threads"][one] < N[one]).all()               # ... and no workgroup without a frame
    assert (o["gx"][~one] == 1).all()
    assert (o["bpw"][~tailed] * o["gy"][~tailed] >= K[~tailed]).all() and ((o["gy"][~tailed] - 1) * o["bpw"][~tailed] < K[~tailed]).all()
    t = tailed
    assert t.sum() > 500                                                                         # the sweep reaches the tail
    assert (o["gy"][t] == o["tail_from"][t] + (K[t] - o["tail_from"][t]) * o["tail_split"][t]).all()
    assert (o["tail_nb"][t] * o["tail_split"][t] == NB[t]).all() and np.isin(o["tail_split"][t], (2, 4)).all()
    assert (o["tail_from"][t] < K[t]).all() and (K[t] >= tail_min).all() and (o["gz"][t] == 1).all() and (NB[t] == B[t]).all()
    assert ((o["bpw"][t] == 1) & (o["staged"][t] == 0) & (o["gx"][t] == 1) & ~pair[t]).all()      # what the kernel's own `tailed` needs
    assert ((o["tail_split"][~t] == 1) & (o["tail_nb"][~t] == NB[~t]) & (o["tail_from"][~t] == 0)).all()
    assert (o["gz"] == np.where(NB > 1, (B + NB - 1) // NB, B * c["groups"])).all()
    # the order: one block per workgroup, register gathers, a table to read, and exactly the two kernels that read it
    od = o["order"] == 1
    assert od.sum() > 1000 and ((o["bpw"][od] == 1) & (o["staged"][od] == 0) & (c["order_table"][od] == 1) & (c["groups"][od] == 1)).all()
    assert (od == ((o["kernel"] == PHASE_RENDER) | (o["kernel"] == PAIR_PHASE_RENDER))).all()
    # the kernel scans the levels itself exactly where one workgroup holds a whole block of the final mix
    assert ((o["scans_levels"] == 1) == ((c["groups"] == 1) & (o["gx"] == 1))).all() and ((o["scans_levels"] == 1) == ((c["groups"] == 1) & (N <= 256))).all()
    # staged: only where asked for, a batch of whole 256-lane workgroups; its ring is the launch's dynamic LDS
    st = o["staged"] == 1
    assert ((c["staged"][st] == 1) & (K[st] > 1) & (o["threads"][st] == 256) & (o["dyn_lds"][st] == ST_RING)).all()
    assert (st == ((c["staged"] == 1) & (K > 1) & ((N >= 193) | (N == 64) | (N == 128)) & ~pair)).all()
    herm = (c["mode"] & 4) != 0
    plain = ~st & ~pair
    assert (o["dyn_lds"][plain] == np.where(o["bpw"][plain] > 1, 0, np.where(herm[plain], 0, 10240))).all()
    assert (o["dyn_lds"][pair] == PAIR_LDS - PAIR_STATIC).all()
    # pair: exactly zl_pair_shape and the switch
    ps = pair_shape
    shape = np.array([ps(*[int(c[k][i]) for k in ("mode", "N", "K", "NB", "groups", "staged", "trace", "fan", "host_out", "ongrid")]) for i in np.flatnonzero(N == 256)])
    sel = np.flatnonzero(N == 256)
    want = (shape == 1) & ((c["pair_mode"][sel] == 2) | ((c["pair_mode"][sel] == 1) & (c["cheap"][sel] == 1)))
    assert (pair[sel] == want).all() and not pair[N != 256].any()       # (few rows here have the shape: the next test is dense in it)
    assert ((o["gx"][pair] == 1) & (o["gy"][pair] == K[pair]) & (o["gz"][pair] == B[pair]) & (o["bpw"][pair] == 1) & (o["staged"][pair] == 0)).all()


def test_the_pair_shape_is_dense_in_its_own_sweep():
    """the sweep above meets the pair shape only at N = 256; here every row has it but for one field drawn away"""
    rng = np.random.default_rng(7)
    n = 20000
    a = {k: np.full(n, BASE[k] if BASE[k] is not None else 8192, dtype=np.int32) for k in IN}
    a["pair_mode"][:] = 2
    a["order_mode"] = rng.choice(np.array([0, 2]), size=n).astype(np.int32)
    field = rng.integers(0, 11, size=n)
    draws = [("mode", range(8)), ("N", (64, 128, 255, 256, 257, 512)), ("K", (1, 2, 8192)), ("NB", (1, 2, 8)), ("groups", (1, 2)), ("staged", (0, 1)),
             ("trace", (0, 1)), ("fan", (0, 1)), ("host_out", (0, 1)), ("ongrid", (0, 1, 2)), ("cheap", (0, 1))]
    for i, (k, vals) in enumerate(draws):
        sel = field == i
        a[k][sel] = rng.choice(np.asarray(vals), size=int(sel.sum()))
    o = launch_many(np.stack([a[k] for k in IN], axis=1))
    ps = pair_shape
    shape = np.array([ps(*[int(a[k][i]) for k in ("mode", "N", "K", "NB", "groups", "staged", "trace", "fan", "host_out", "ongrid")]) for i in range(n)])
    pair = (o["kernel"] == PAIR_RENDER) | (o["kernel"] == PAIR_PHASE_RENDER)
    assert (pair == (shape == 1)).all() and pair.sum() > n // 4 and (~pair).sum() > n // 4
    assert (o["threads"][pair] == 128).all() and (o["threads"][~pair & (a["N"] >= 193)] == 256).all()
