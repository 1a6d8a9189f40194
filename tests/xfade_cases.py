"""The loop crossfade's cases, shared by the CPU tier (tests/test_xfade_cpu.py walks them through the host build of the header) and the
GPU tier (tests/test_xfade_gpu.py runs them through the kernels): clips and requests, each a dict with the planar clip "x" and the
request's fields."""
import numpy as np

import xfade_ref as xr

f32 = np.float32
SR = 48000.0
FADES = (1, 2, 3, 5, 8, 64, 257, 960)


def clip(rng, ch, n):
    x = rng.uniform(-1.0, 1.0, (ch, n)).astype(f32)
    special = np.array([0.0, -0.0, 1e-39, -1e-39, 1.0, -1.0, 7.9999, -8.5], f32)     # +-0, denormals, +-1, at and beyond the quantiser's clamp
    at = rng.integers(0, n, size=max(1, n // 7))
    x[rng.integers(0, ch, size=at.size), at] = special[rng.integers(0, special.size, size=at.size)]
    return x


def grid(seed=1):
    """mono and stereo, every fade of FADES with (e - s) and (e - X) in every residue modulo 4 frames (so the floats of B take every
    misalignment against A's groups and the fade begins at every place inside a group), s = X (B starts at frame 0: d2 = 0), e = length
    (A ends at the last frame: every other case), X = s = e - s (the regions adjoin), the shortest clip, a clip of 4096 frames, a stereo
    clip of 70000 frames (137 workgroups) whose fade straddles a workgroup's edge; requests with nothing to fade first, last and twice in
    a row in the middle"""
    rng = np.random.default_rng(seed)
    cases = []

    def add(ch, n, s, e, X, curve=None):
        cases.append(dict(x=clip(rng, ch, n), start_frame=s, stop_frame=e, fade_frames=X, curve=len(cases) % 3 if curve is None else curve))

    for ch in (1, 2):
        for X in FADES:
            for d1 in range(4):
                for d2 in range(4):
                    s = X + d2
                    e = s + X + 16 + d1
                    add(ch, e + (0 if (d1 + d2) % 2 == 0 else 5), s, e, X)
        for X in (1, 5, 64, 960):
            add(ch, 2 * X, X, 2 * X, X)
            add(ch, 2 * X + 3, X, 2 * X, X)
        add(ch, 4096, 1000, 4096, 960)
        add(ch, 4095, 1001, 4093, 0)                               # the default: 960 frames at 48 kHz
    add(1, 2, 1, 2, 1)
    add(2, 2, 1, 2, 1)
    add(2, 70000, 20000, 512 * 100 + 7, 64)
    assert cases[-1]["stop_frame"] - 64 < 512 * 100 < cases[-1]["stop_frame"]
    nothing = lambda: dict(x=clip(rng, 1 + len(cases) % 2, 300), start_frame=0, stop_frame=200 + len(cases) % 50, fade_frames=0, curve=0)
    half = len(cases) // 2
    return [nothing()] + cases[:half] + [nothing(), nothing()] + cases[half:] + [nothing()]


def facts(cases):
    """what the grid is meant to cover, counted: {(channels, (e - s) ch mod 4)}, {(channels, (e - X) ch mod 4)} and the flags"""
    ds, da = set(), set()
    at0 = last = adjoin = 0
    for c in cases:
        ch, n = c["x"].shape
        X = xr.resolve(SR, n, c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"])
        if not X:
            continue
        s, e = c["start_frame"], c["stop_frame"]
        ds.add((ch, (e - s) * ch % 4)); da.add((ch, (e - X) * ch % 4))
        at0 += s == X; last += e == n; adjoin += X == s == e - s
    return ds, da, at0, last, adjoin


def want(c, rate=SR, ints=None, ab=None):
    """the restatement of one case: (result, the extent's floats)"""
    res, y = xr.crossfade(c["x"], rate, c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"], ints=ints, ab=ab)
    return res, xr.extent(y)


# ---- on the device --------------------------------------------------------------------------------------------------------------------
def upload(syn, x, sr=SR):
    return syn.register_clip(x[0].copy(), x[1].copy() if x.shape[0] == 2 else None, float(sr))


def dirty(syn, floats):
    """noise over the first `floats` floats of a fresh arena, released again: what is allocated next lies on it, so that a float of an
    extent that nobody writes does not read as zero by luck"""
    x = np.random.default_rng(99).uniform(1.0, 2.0, floats - 8).astype(f32)
    cid = syn.register_clip(x, None, SR)
    syn.unregister_clip(cid)


def library_table(lib, X, rho):
    ab = np.full((X, 2), np.nan, f32)
    assert lib.zlhip_xfade_design(X, rho, ab.ctypes.data) == 0
    return ab


def mismatch(syn, cid, c, got, rate=SR, extent=None):
    """what differs between the device's answer for case c (result `got`, the extent clip `cid` holds now) and the restatement, or None.
    The integers are compared with the restatement's own; correlation and rho with their finish (==); the extent with the restatement
    fed the LIBRARY's weight table (zlhip_xfade_design) of the device's rho, so that no libm difference can enter"""
    u32 = np.uint32
    x = c["x"]
    X = xr.resolve(rate, x.shape[1], c["start_frame"], c["stop_frame"], c["fade_frames"], c["curve"])
    ext = syn.clip_extent(cid) if extent is None else extent
    if not X:
        if any(v != 0 for v in got.values()):
            return ("result of a request with nothing to fade", got)
        return None
    ints = xr.sums(x, c["start_frame"], c["stop_frame"], X)
    if (got["sab"], got["saa"], got["sbb"]) != ints:
        return ("integers", got, ints)
    ab = library_table(syn._lib, X, got["rho"])
    if not np.array_equal(ab.view(u32), xr.design(X, got["rho"]).view(u32)):
        return ("the library's table differs from the restatement's", X, got["rho"])
    res, want_ext = want(c, rate, ints=ints, ab=ab)
    if any(got[k] != res[k] for k in xr.RESULT_INTS) or got["correlation"] != res["correlation"] or got["rho"] != res["rho"]:
        return ("result", got, res)
    if ext.size != want_ext.size:
        return ("extent size", ext.size, want_ext.size)
    an, bn = np.isnan(ext), np.isnan(want_ext)                      # (NaN payloads differ between the host and the device)
    if not np.array_equal(an, bn) or not np.array_equal(ext[~an].view(u32), want_ext[~bn].view(u32)):
        return ("extent", np.flatnonzero((ext.view(u32) != want_ext.view(u32)) & ~(an & bn))[:8])
    return None


def check_call(syn, cases, ids, rate=SR):
    """one clip_loop_crossfade_batch over the cases (clip ids[i] holds cases[i]["x"]): (the mismatches, the results)"""
    outs = syn.clip_loop_crossfade_batch([dict(clip=cid, start_frame=c["start_frame"], stop_frame=c["stop_frame"], fade_frames=c["fade_frames"], curve=c["curve"])
                                          for cid, c in zip(ids, cases)])
    bad = []
    for i, (cid, c, got) in enumerate(zip(ids, cases, outs)):
        m = mismatch(syn, cid, c, got, rate)
        if m is not None:
            bad.append((i, c["x"].shape, {k: v for k, v in c.items() if k != "x"}, m))
    return bad, outs
