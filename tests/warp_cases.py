"""The cases of the warp tests (tests/test_warp_cpu.py against the host build of zl_warp.h, tests/test_warp_gpu.py and
tests/test_warp_edges_gpu.py against the device): clips small enough for the restatement because their sample rates are low -- 1000 Hz
gives O = 16 and regions of tens of frames -- each a dict(x float32 [ch][len], rate, anchors, tag).  The restatement's answer to a case
is computed once per session (want) and shared read-only."""
import math

import numpy as np

import warp_ref as wr

f32 = np.float32


def chain(pairs):
    """anchors from (A, D) pairs"""
    out, a, d = [(0, 0)], 0, 0
    for A, D in pairs:
        a += A
        d += D
        out.append((a, d))
    return out


def clip(seed, ch, n):
    """noise with a slow sine under it, so that the seek has something to find"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.4 * np.sin(2 * np.pi * t / 23.0)[None, :] + rng.uniform(-0.4, 0.4, (ch, n))).astype(f32)


def case(tag, rate, ch, pairs, seed=None, x=None):
    anchors = chain(pairs)
    n = anchors[-1][0]
    if x is None:
        x = clip(len(tag) * 131 + n + ch if seed is None else seed, ch, n)
    assert x.shape == (ch, n), (tag, x.shape, n)
    return dict(tag=tag, rate=float(rate), x=x, anchors=anchors)


def last_frame_case(rate, ch, A, D):
    """One stretched region of silence but for two frames, placed so that the seek of segment 2 is decided by the last frame of its
    window that any candidate reads: segment 1 sees a zero reference and stays at offset 0; the last frame of its cross-fade tail
    (in[b_1 + L + O - 1]) is the only non-zero weight of segment 2's reference; the only non-zero frame of segment 2's window is
    frame W + O - 2 of it, which candidate W - 1 alone reaches, with its last product.  So off_2 = W - 1."""
    O = wr.overlap(rate)
    r = wr.region(rate, O, 0, 0, A, D)
    assert r is not None and r["nseg"] >= 3
    nom = [min(int(math.floor(k * r["step"])), r["room"]) for k in range(3)]
    first, second = nom[1] + r["L"] + O - 1, nom[2] + r["W"] + O - 2
    assert not (nom[2] <= first < nom[2] + r["W"] + O) and not (r["L"] <= first < r["L"] + O) and first != second and max(first, second) < A
    assert not (r["L"] <= second < r["L"] + O) and not (nom[1] + r["L"] <= second < nom[1] + r["L"] + O - 1)
    x = np.zeros((ch, A), f32)
    x[:, first] = 7.5
    x[:, second] = 7.5
    return dict(tag="last-frame-%d-%dch" % (int(rate), ch), rate=float(rate), x=x, anchors=[(0, 0), (A, D)], expect_off2=r["W"] - 1)


def grid():
    """the cases of one call.  Identity requests first, last and two in a row; mono and stereo; one region only; a copy region between
    two stretched ones; nseg = 1 with D < O, D = O, D = L and D = L + 1; room = 0; the clamp reached by the last segment only;
    tau = 0.25 and 4 exactly; W = 6, 34, 160 and 640; d_i in every residue modulo 4 (mono) and 2 (stereo); N + 8 = 256, 257, 512, 513;
    a region boundary on a synthesis workgroup's edge (d = 256)"""
    g = []
    g.append(case("identity-first", 1000, 1, [(120, 120), (80, 80)]))
    g.append(case("one-region", 1000, 1, [(100, 150)]))
    g.append(case("copy-between", 1000, 2, [(100, 130), (50, 50), (120, 90)]))
    g.append(case("nseg1", 1000, 1, [(40, 10), (40, 16), (60, 24), (60, 25), (50, 50), (48, 12)]))     # D < O, D = O, D = L, D = L + 1, a copy, D < O behind a copy
    g.append(case("nseg1-stereo", 1000, 2, [(60, 25), (40, 10), (40, 16), (60, 24)]))
    g.append(case("identity-mid-a", 1000, 2, [(64, 64)]))
    g.append(case("identity-mid-b", 2000, 1, [(10, 10), (1, 1), (30, 30)]))
    g.append(case("room0", 1000, 1, [(93, 200), (93, 200)]))
    g.append(case("room0-stereo", 1000, 2, [(93, 200)]))
    g.append(case("clamp-last", 1000, 1, [(162, 180), (216, 240)]))
    g.append(case("tau-quarter", 1000, 2, [(100, 400), (50, 50), (93, 372)]))
    g.append(case("tau-four", 1000, 1, [(240, 60), (400, 100)]))
    g.append(case("tau-four-stereo", 1000, 2, [(240, 60)]))
    g.append(case("w6", 300, 1, [(20, 40), (30, 30), (16, 32), (25, 50)]))
    g.append(case("w34", 1700, 2, [(180, 360), (170, 340)]))
    g.append(case("w160", 8000, 2, [(820, 1640), (700, 640)]))
    g.append(case("w640", 32000, 1, [(3300, 6500), (3100, 3000)]))
    g.append(case("residues-mono", 1000, 1, [(110, 101), (111, 102), (112, 103), (113, 104)]))        # d = 0, 101, 203, 306: residues 0, 1, 3, 2
    g.append(case("residues-stereo", 1000, 2, [(110, 101), (111, 102), (95, 95), (112, 103)]))        # d = 0, 101, 203, 298
    for N in (248, 249, 504, 505):
        g.append(case("n%d" % N, 1000, 1, [(N - 48, N)]))
    g.append(case("n248-stereo", 1000, 2, [(100, 124), (100, 124)]))
    g.append(case("n505-stereo", 1000, 2, [(300, 280), (200, 225)]))
    g.append(case("wg-edge", 1000, 1, [(200, 256), (100, 140), (116, 116)]))
    g.append(case("wg-edge-stereo", 1000, 2, [(200, 256), (230, 256), (100, 140)]))
    g.append(last_frame_case(8000.0, 1, 1000, 2000))
    g.append(last_frame_case(8000.0, 2, 1600, 3200))
    g.append(case("identity-last", 1000, 2, [(77, 77)]))
    for c in g:
        c["x"].setflags(write=False)
    return g


def facts(cases):
    """what the grid is meant to hold, read off the restatement's own resolve"""
    f = dict(W=set(), mono_res=set(), stereo_res=set(), n8=set(), taus=set(), nseg1=set(), room0=0, clamp_last=0, copy_between=0, edge=0, one_region=0)
    for c in cases:
        ch, n = c["x"].shape
        summary, regs = wr.resolve(c["rate"], n, c["anchors"])
        if not summary["applied"]:
            continue
        O = summary["overlap"]
        f["n8"].add(summary["length"] + 8)
        f["one_region"] += len(regs) == 1
        for i, r in enumerate(regs):
            (f["mono_res"] if ch == 1 else f["stereo_res"]).add(r["d"] % (4 if ch == 1 else 2))
            f["edge"] += r["d"] == 256
            if not r["stretched"]:
                f["copy_between"] += 0 < i < len(regs) - 1 and regs[i - 1]["stretched"] and regs[i + 1]["stretched"]
                continue
            f["W"].add(r["W"])
            if r["A"] == 4 * r["D"]:
                f["taus"].add(4.0)
            if r["D"] == 4 * r["A"]:
                f["taus"].add(0.25)
            if r["nseg"] == 1:
                f["nseg1"].add("D<O" if r["D"] < O else "D=O" if r["D"] == O else "D=L" if r["D"] == r["L"] else "other")
            if r["D"] == r["L"] + 1:
                f["nseg1"].add("D=L+1")
            noms = [int(math.floor(k * r["step"])) for k in range(1, r["nseg"])]
            if r["room"] == 0 and r["nseg"] >= 3:
                f["room0"] += 1
            if len(noms) >= 2 and all(v <= r["room"] for v in noms[:-1]) and noms[-1] > r["room"]:
                f["clamp_last"] += 1
    return f


_wants = {}


def want(c):
    """(summary, y [ch][N], offsets, the extent's floats) by the restatement, computed once"""
    key = c["tag"]
    if key not in _wants:
        summary, y, offs, _ = wr.warp(c["x"], c["rate"], c["anchors"])
        ext = wr.extent(y)
        for a in (y, offs, ext):
            a.setflags(write=False)
        _wants[key] = (summary, y, offs, ext)
    return _wants[key]


def tie_case(sr, ch, period):
    """a periodic clip (rerender_cases.tie_source: 30000 frames) in stretched regions: the candidates o, o + P, o + 2 P ... of a
    window inside the clip score the same to the bit, and the tie rule picks the smallest.  (At 96 kHz a segment is some 7900 frames:
    two regions near tau = 0.68 of three segments each, so that there are segments enough.)"""
    from rerender_cases import tie_source
    x = tie_source(sr, ch, period)
    anchors = [(0, 0), (16000, 20000), (30000, 31200)] if sr < 90000.0 else [(0, 0), (15000, 22400), (30000, 44000)]
    return dict(tag="tie-%d-%dch-p%d" % (int(sr), ch, period), rate=float(sr), x=x, anchors=anchors, period=period)


def same_bits(a, b):
    """equal bit for bit, NaN positions compared as NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


# ---- on the device --------------------------------------------------------------------------------------------------------------------
def upload(syn, x, rate):
    return syn.register_clip(x[0].copy(), x[1].copy() if x.shape[0] == 2 else None, float(rate))


def dirty(syn, floats, rate=48000.0):
    """noise over the first `floats` floats of a fresh arena, released again: what is allocated next lies on it, so that a float of an
    extent that nobody writes does not read as zero by luck"""
    x = np.random.default_rng(99).uniform(1.0, 2.0, floats - 8).astype(f32)
    syn.unregister_clip(syn.register_clip(x, None, rate))


def mismatch(syn, cid, c, got, extent=None, offsets=None):
    """what differs between the device's answer for case c (result `got`, the extent clip `cid` holds now, its seek offsets) and the
    restatement, or None"""
    summary, y, offs, ext = want(c)
    if got != summary:
        return ("result", got, summary)
    have = syn.clip_extent(cid) if extent is None else extent
    if not summary["applied"]:
        src = extent_of(c["x"])
        return None if same_bits(have[:src.size], src) and have.size >= src.size else ("the extent of an identity request changed",)
    if have.size != ext.size:
        return ("extent size", have.size, ext.size)
    if not same_bits(have, ext):
        return ("extent", np.flatnonzero(have.view(np.uint32) != ext.view(np.uint32))[:8])
    o = syn.warp_offsets(cid) if offsets is None else offsets
    if not np.array_equal(o, offs):
        return ("offsets", o, offs)
    return None


def extent_of(planar):
    """what the arena holds for an uploaded clip: its frames interleaved, then 8 zero frames"""
    ch, n = planar.shape
    out = np.zeros((n + 8) * ch, f32)
    out[:n * ch] = planar.T.reshape(-1)
    return out


def check_call(syn, cases, ids):
    """one clip_warp_batch over the cases (clip ids[i] holds cases[i]["x"]): (the mismatches, the results)"""
    outs = syn.clip_warp_batch([(cid, c["anchors"]) for cid, c in zip(ids, cases)])
    bad = []
    for cid, c, got in zip(ids, cases, outs):
        m = mismatch(syn, cid, c, got)
        if m is not None:
            bad.append((c["tag"], m))
    return bad, outs
