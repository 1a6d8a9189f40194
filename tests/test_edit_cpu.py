"""Clip edit, CPU tier: the host build of libzl_amd/csrc/zl_edit.h (tests/cpu_harness/edit_host.cpp walks a call the way the kernels
do, workgroup by workgroup and group by group, with the header's own arithmetic) against the numpy restatement (tests/edit_ref.py) with
== on every float of every extent, on F, Z, Xi and Xo and on every weight table, every float of an extent written exactly once and no
read outside the buffer the harness was given; that the grid hits the edges it is aimed at; the resolve at every limit from both
sides; the library's host-only calls, the struct layouts, the new kernels' resources; the walk under the sanitizers
(tests/cpp/edit_check.cpp).  tests/test_edit_gpu.py holds the kernels themselves to the restatement on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edit_cases as ec
import edit_ref as er
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32

_h = None
_z = None


def harness():
    global _h
    if _h is None:
        l = C.CDLL(build.build_edit_harness())
        l.zled_resolve.restype = C.c_int
        l.zled_resolve.argtypes = [C.c_int32, C.POINTER(_abi.EditRequest)]
        l.zled_design.restype = None
        l.zled_design.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        l.zled_extent_floats.restype = C.c_int64
        l.zled_extent_floats.argtypes = [C.c_int64, C.c_int32]
        l.zled_call.restype = C.c_int32
        l.zled_call.argtypes = [C.c_int32] + [C.c_void_p] * 12
        _h = l
    return _h


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


def abi_request(q, cid=0):
    return _abi.EditRequest(cid, *(int(q[k]) for k in er.REQUEST_KEYS[:-1]), float(q["threshold"]))


def run_call(cases, short=None, lacking=()):
    """one harness call over the cases.  short: {case index: floats the accessor is told the source holds}; lacking: the cases whose
    original lacks ZL_SOUND_FINITE.  Returns (status, results, extents, writes, w_in, w_out, verdicts, walk)"""
    n = len(cases)
    reqs = (_abi.EditRequest * n)(*[abi_request(c["q"]) for c in cases])
    srcs = [np.ascontiguousarray(c["x"].T.reshape(-1)) for c in cases]
    floats = [int(harness().zled_extent_floats(c["x"].shape[1], c["x"].shape[0])) for c in cases]
    dst = [np.full(k, np.nan, f32) for k in floats]
    writes = [np.zeros(k, np.int32) for k in floats]
    w_in = [np.full(c["x"].shape[1] // 2 + 1, np.nan, f32) for c in cases]
    w_out = [np.full(c["x"].shape[1] // 2 + 1, np.nan, f32) for c in cases]
    ptrs = lambda arrs: (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    nsrc = (C.c_int64 * n)(*[(short or {}).get(i, s.size) for i, s in enumerate(srcs)])
    length = (C.c_int32 * n)(*[c["x"].shape[1] for c in cases])
    chans = (C.c_int32 * n)(*[c["x"].shape[0] for c in cases])
    out = (_abi.Edit * n)()
    verdicts = (C.c_uint32 * n)(*[1 if i in lacking else 0 for i in range(n)])
    walk = (C.c_int64 * 6)()
    pSrc, pDst, pWrites, pIn, pOut = ptrs(srcs), ptrs(dst), ptrs(writes), ptrs(w_in), ptrs(w_out)
    rc = harness().zled_call(n, C.addressof(reqs), C.addressof(pSrc), C.addressof(nsrc), C.addressof(length), C.addressof(chans), C.addressof(pDst),
                             C.addressof(pWrites), C.addressof(out), C.addressof(pIn), C.addressof(pOut), C.addressof(verdicts), C.addressof(walk))
    res = [{k: getattr(out[i], k) for k in er.RESULT_FIELDS} for i in range(n)]
    return rc, res, dst, writes, w_in, w_out, list(verdicts), tuple(walk)


# ---- the grid hits what it is aimed at ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return ec.grid()


def test_the_header_and_the_restatement_agree_on_the_launch_shapes():
    assert harness().zled_chunk() == er.CHUNK and harness().zled_wg() == er.WG


def test_the_grid_covers_what_it_is_meant_to(grid):
    F = ec.facts(grid)
    assert {(ch, rev, ra, rn) for ch in (1, 2) for rev in (0, 1) for ra in range(0, 4, ch) for rn in range(0, 4, ch)} <= F["copy"]
    assert {(ch, rev, n) for ch in (1, 2) for rev in (0, 1) for n in (1, 2, 3, 4, 5)} <= F["short"]
    assert F["fades"] >= {0, 1, 2} and F["curves"] >= {er.LINEAR, er.SQRT, er.SMOOTH}
    assert F["from0rev"] >= 2 and F["whole_rev"] >= 2 and F["at_end"] >= 16
    assert F["odd_middle"] >= 12 and F["even_all"] >= 12           # (n = 9: frame 4 stays unfaded; n = 10: every frame fades)
    assert F["wg_edge"] >= 4 and F["wgs"] >= 3
    assert F["scan_chunks"] >= 4 and F["first_is_F"] >= 2 and F["last_is_Z"] >= 2
    assert F["tags"] >= {"at the threshold", "below the threshold", "negative", "non-finite", "loud neighbours", "loud neighbours of a silent region", "no room",
                         "chunk edge, last frame", "chunk edge, first frame", "chunk edge, both", "silent middle chunk", "right channel only", "silent", "identity"}
    assert max(c["x"].shape[1] for c in grid) <= 3 * er.CHUNK + 100
    # identity and silent requests first, last and twice in a row
    applied = [er.edit(c["x"], c["q"])[0]["applied"] for c in grid]
    twice = [i for i in range(1, len(grid) - 2) if not applied[i] and not applied[i + 1] and grid[i]["tag"] == "silent" and grid[i + 1]["tag"] == "identity"]
    assert not applied[0] and grid[0]["tag"] == "identity" and not applied[-1] and grid[-1]["tag"] == "silent" and twice
    assert F["silent"] >= 4 and F["identity"] >= 2


def test_the_trim_cases_answer_what_they_are_aimed_at(grid):
    """the conditions on the inputs, from the restatement alone"""
    by = {}
    for c in grid:
        by.setdefault(c["tag"], []).append((c, er.edit(c["x"], c["q"])[0]))
    for c, r in by["at the threshold"]:
        assert r["first_loud"] == r["last_loud"] == 70 and r["applied"]
    for c, r in by["below the threshold"]:
        assert r["first_loud"] == r["last_loud"] == 90                # frame 40, one float below the threshold, is not loud
    for c, r in by["negative"]:
        assert (r["first_loud"], r["last_loud"]) == (33, 120)
    assert len(by["non-finite"]) == 6 and all(r["first_loud"] == r["last_loud"] == 50 for _, r in by["non-finite"])
    for c, r in by["loud neighbours"]:
        assert (r["first_loud"], r["last_loud"]) == (50, 180) and c["q"]["first_frame"] == 13 and c["q"]["first_frame"] + c["q"]["num_frames"] == 214
        assert er.loud(c["x"], er.THRESHOLD)[[12, 214]].all()
    for c, r in by["loud neighbours of a silent region"]:
        assert r["silent"] and not r["applied"] and er.loud(c["x"], er.THRESHOLD)[[12, 214]].all()
    for c, r in by["no room"]:
        assert (r["first_frame"], r["num_frames"]) == (20, 300) and r["applied"]
    for c, r in by["pre-roll and hold"]:
        assert (r["first_frame"], r["num_frames"], r["fade_in_frames"], r["fade_out_frames"], r["reversed"]) == (93, 121, 5, 9, 1)
    a = 5
    assert [(r["first_loud"], r["last_loud"]) for _, r in by["chunk edge, last frame"]] == [(a + er.CHUNK - 1,) * 2] * 2
    assert [(r["first_loud"], r["last_loud"]) for _, r in by["chunk edge, first frame"]] == [(a + er.CHUNK,) * 2] * 2
    assert [(r["first_loud"], r["last_loud"]) for _, r in by["chunk edge, both"]] == [(a + er.CHUNK - 1, a + er.CHUNK)] * 2
    for c, r in by["silent middle chunk"]:
        assert (r["first_loud"], r["last_loud"]) == (1000, 2 * er.CHUNK + 900) and (r["first_frame"], r["num_frames"]) == (997, er.CHUNK * 2 + 900 + 3 - 997)
        assert not er.loud(c["x"][:, 3 + er.CHUNK:3 + 2 * er.CHUNK], er.THRESHOLD).any()
    for c, r in by["right channel only"]:
        assert (r["first_loud"], r["last_loud"]) == (77, 140) and not er.loud(c["x"][:1], er.THRESHOLD).any()


# ---- the header against the restatement ---------------------------------------------------------------------------------------------
def test_harness_matches_the_restatement_on_every_bit(grid):
    rc, res, dst, writes, w_in, w_out, verdicts, walk = run_call(grid)
    wants = [ec.want(c) for c in grid]
    assert rc == sum(w[0]["applied"] for w in wants) and rc >= len(grid) - 8
    assert walk[3] == 0, "a read outside a clip's own floats"
    full = faded = weights = 0
    for i, (c, (want, ext)) in enumerate(zip(grid, wants)):
        assert res[i] == want, (i, c["tag"], res[i], want)
        if not want["applied"]:
            assert not writes[i].any() and np.isnan(dst[i]).all(), (i, c["tag"])
            continue
        Xi, Xo = want["fade_in_frames"], want["fade_out_frames"]
        assert np.array_equal(w_in[i][:Xi].view(u32), er.design(Xi, c["q"]["curve"]).view(u32)) and np.isnan(w_in[i][Xi:]).all(), i
        assert np.array_equal(w_out[i][:Xo].view(u32), er.design(Xo, c["q"]["curve"]).view(u32)) and np.isnan(w_out[i][Xo:]).all(), i
        assert np.all(writes[i][:ext.size] == 1) and not writes[i][ext.size:].any(), (i, c["tag"], np.flatnonzero(writes[i][:ext.size] != 1)[:8])
        assert ec.same_bits(dst[i][:ext.size], ext) is None, (i, c["tag"], c["q"], ec.same_bits(dst[i][:ext.size], ext))
        assert verdicts[i] == (0 if er.faded_finite(ext[:want["length"] * c["x"].shape[0]].reshape(-1, c["x"].shape[0]).T, Xi, Xo) else 1)
        full += want["length"] * c["x"].shape[0] // 4
        faded += Xi + Xo > 0
        weights += Xi + Xo
    assert walk[0] == full and walk[1] >= faded and walk[5] == weights          # one wide load per full group, one weight per faded frame
    assert walk[2] >= rc + 2 + 3 and walk[4] >= sum(1 for c in grid if c["q"]["flags"] & er.TRIM) + 2 * 8


def test_a_call_of_nothing_to_change_touches_nothing(grid):
    cases = [c for c in grid if not er.edit(c["x"], c["q"])[0]["applied"]]
    assert len(cases) >= 6
    rc, res, dst, writes, _, _, _, walk = run_call(cases)
    assert rc == 0 and walk[:4] == (0, 0, 0, 0) and all(not w.any() for w in writes)
    assert [r["silent"] for r in res] == [er.edit(c["x"], c["q"])[0]["silent"] for c in cases]
    plain = [c for c in cases if not c["q"]["flags"] & er.TRIM]
    assert plain and run_call(plain)[7] == (0,) * 6                       # without TRIM not even a scan


def test_the_harness_refuses_a_read_outside_the_buffer_it_was_given():
    """the refusal is the accessor's, not the masks': told that the buffer is one float shorter than the clip, the walk over a region that
    ends at the clip's last frame is refused that float -- forwards in the group the data's end cuts, reversed in the very first group,
    and by the scan -- and the NaN shows in the output"""
    x = ec.clip(np.random.default_rng(4), 1, 301)
    x[0, 300] = 0.5
    fwd = dict(tag="", x=x, q=er.request(first_frame=100))
    rev = dict(tag="", x=x, q=er.request(first_frame=100, flags=er.REVERSE))
    trm = dict(tag="", x=x, q=er.request(first_frame=100, flags=er.TRIM, fade_in_frames=2))
    rc, _, dst, writes, _, _, verdicts, walk = run_call([fwd, rev, trm])
    assert rc == 3 and walk[3] == 0 and verdicts == [0, 0, 0]
    rc, res, dst, writes, _, _, verdicts, walk = run_call([fwd, rev, trm], short={0: 300, 1: 300, 2: 300})
    assert rc == 3 and walk[3] == 4                                # forward, reversed, the scan, the trimmed copy
    assert np.isnan(dst[0][200]) and not np.isnan(dst[0][:200]).any() and np.isnan(dst[1][0]) and not np.isnan(dst[1][1:209]).any()
    assert all(np.all(w[:212] == 1) for w in writes[:2])


def test_the_verdict():
    """an inf inside a fade sets the word, an inf that is only copied or cropped away does not; a clip whose original lacks the flag keeps
    its word; the restatement says the same"""
    base = ec.clip(np.random.default_rng(6), 2, 400)
    cases = []
    for k, (frame, q) in enumerate(((None, {}), (105, {}), (150, {}), (50, {}), (299, {}), (150, dict(flags=er.REVERSE)), (297, dict(flags=er.REVERSE)))):
        x = base.copy()
        if frame is not None:
            x[1, frame] = np.inf
        cases.append(dict(tag="", x=x, q=er.request(first_frame=100, num_frames=200, fade_in_frames=10, fade_out_frames=10, curve=er.SQRT, **q)))
    rc, res, dst, _, _, _, verdicts, walk = run_call(cases + [cases[0]], lacking=(7,))
    assert rc == 8 and walk[3] == 0
    assert verdicts == [0, 1, 0, 0, 1, 0, 1, 1]                     # (frame 299 meets weight 0: 0 inf is a NaN; reversed, source frame 297 is output frame 2)
    for i, c in enumerate(cases):
        want, ext = ec.want(c)
        assert er.faded_finite(ext[:400].reshape(200, 2).T, 10, 10) == (verdicts[i] == 0), i
        assert ec.same_bits(dst[i][:ext.size], ext) is None


# ---- resolve and design ---------------------------------------------------------------------------------------------------------------
def resolve_all(length, **kw):
    """the header's, the library's and the restatement's answer: (num_frames, threshold) or None; they agree"""
    q = er.request(**kw)
    outs = []
    for fn in (harness().zled_resolve, zlhip().zlhip_edit_resolve):
        r = abi_request(q, 7)
        before = bytes(r)
        rc = fn(length, C.byref(r))
        assert (r.id, r.first_frame, r.flags, r.curve) == (7, q["first_frame"], q["flags"], q["curve"])
        if rc != 0:
            assert bytes(r) == before
        outs.append((r.num_frames, r.threshold) if rc == 0 else None)
    ref = er.resolve(length, q)
    ref = None if ref is None else (ref[1] - ref[0], float(ref[2]))
    assert outs[0] == outs[1] == ref, (kw, outs, ref)
    return ref


def test_resolve_at_every_limit(built):
    n = 1000
    thr = float(er.THRESHOLD)
    assert thr == 2.0 ** -10
    assert resolve_all(n) == (n, thr) and resolve_all(n, first_frame=999) == (1, thr) and resolve_all(n, first_frame=1000) is None
    assert resolve_all(n, first_frame=10, num_frames=990) == (990, thr) and resolve_all(n, first_frame=10, num_frames=991) is None
    assert resolve_all(n, first_frame=999, num_frames=1) == (1, thr) and resolve_all(n, first_frame=-1, num_frames=5) is None and resolve_all(n, num_frames=-1) is None
    assert resolve_all(n, first_frame=2 ** 31 - 1, num_frames=2 ** 31 - 1) is None          # (the sum in 64 bits)
    assert resolve_all(n, flags=3) == (n, thr) and resolve_all(n, flags=4) is None and resolve_all(n, flags=-1) is None
    assert resolve_all(n, curve=2) == (n, thr) and resolve_all(n, curve=3) is None and resolve_all(n, curve=-1) is None
    tiny = float(np.nextafter(f32(0.0), f32(1.0)))
    big = float(np.finfo(f32).max)
    assert resolve_all(n, threshold=tiny) == (n, tiny) and resolve_all(n, threshold=big) == (n, big)
    for bad in (-tiny, -1.0, float("inf"), float("nan")):
        assert resolve_all(n, threshold=bad) is None
    for key in ("pre_roll_frames", "hold_frames", "fade_in_frames", "fade_out_frames"):
        assert resolve_all(n, **{key: 2 ** 31 - 1}) == (n, thr) and resolve_all(n, **{key: -1}) is None
    assert resolve_all(1) == (1, thr) and resolve_all(0) is None
    assert zlhip().zlhip_edit_resolve(n, None) == _abi.ZLHIP_ERR_INVALID


def test_design_matches_the_restatement(built):
    for curve in (er.LINEAR, er.SQRT, er.SMOOTH):
        for X in (1, 2, 3, 5, 960, 4801, 65536):
            ref = er.design(X, curve)
            for fn in (harness().zled_design, zlhip().zlhip_edit_design):
                w = np.full(X, np.nan, f32)
                fn(X, curve, w.ctypes.data)
                assert np.array_equal(w.view(u32), ref.view(u32)), (X, curve)
            assert ref[0] == 0.0 and not np.signbit(ref[0]) and np.all(np.diff(ref) >= 0) and ref[-1] <= 1.0 and (X > 960 or np.all(np.diff(ref) > 0))
    t = np.arange(8) / 8.0
    assert np.array_equal(er.design(8, er.LINEAR), t.astype(f32))
    # the square root: a fade in against a fade out keeps the power constant
    w = er.design(960, er.SQRT).astype(np.float64)
    assert np.all(np.abs(w[1:] ** 2 + w[:0:-1] ** 2 - 1.0) <= 2e-7)
    z = zlhip()
    w = np.zeros(4, f32)
    assert z.zlhip_edit_design(0, 0, w.ctypes.data) == z.zlhip_edit_design(4, 3, w.ctypes.data) == z.zlhip_edit_design(4, 0, None) == _abi.ZLHIP_ERR_INVALID and not w.any()


# ---- the C-ABI without a GPU, the layouts, the kernels' resources ---------------------------------------------------------------------
def test_without_a_gpu_the_calls_answer_invalid(built):
    l = zlhip()
    q = abi_request(er.request(flags=er.REVERSE))
    out = _abi.Edit()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert l.zlhip_sound_edit(None, C.byref(q), C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_sound_edit_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_edit_batch(None, C.byref(q), 1, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_edit_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert bytes(out) == b"\x5a" * C.sizeof(out)
    lz = C.CDLL(build.build_engine())
    for name, args in (("libzl_hotpath_clip_trim_silence", [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
                       ("libzl_hotpath_clips_trim", [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]),
                       ("libzl_hotpath_clip_crop", [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]),
                       ("libzl_hotpath_clip_reverse", [C.c_void_p])):
        getattr(lz, name).restype = C.c_int
        getattr(lz, name).argtypes = args
    n = C.c_int(-7)
    assert lz.libzl_hotpath_clip_trim_silence(None, 0.0, 0.0, 0.0, C.byref(n), C.byref(n)) == _abi.ZLHIP_ERR_INVALID and n.value == -7
    assert lz.libzl_hotpath_clips_trim(None, 2, 0.0, 0.0, 0.0, None) == _abi.ZLHIP_ERR_INVALID
    assert lz.libzl_hotpath_clip_crop(None, 0.0, 0.0, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID and n.value == -7
    assert lz.libzl_hotpath_clip_reverse(None) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_abi_version() == 3


def test_edit_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    structs = (("zlhip_edit_request", _abi.EditRequest), ("zlhip_edit", _abi.Edit))
    body = "".join('printf("%%d ",(int)sizeof(%s));' % n for n, _ in structs)
    body += "".join('printf("%%d ",(int)offsetof(%s,%s));' % (n, f) for n, s in structs for f, _ in s._fields_)
    body += 'printf("%d %d %d %d %d ",ZLHIP_EDIT_TRIM,ZLHIP_EDIT_REVERSE,ZLHIP_EDIT_LINEAR,ZLHIP_EDIT_SQRT,ZLHIP_EDIT_SMOOTH);'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){' + body + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-5] == [C.sizeof(s) for _, s in structs] + [getattr(s, f).offset for _, s in structs for f, _ in s._fields_]
    assert got[:2] == [40, 48] == [size for _, size in _abi.STRUCT_SIZES.values()] and all(C.sizeof(s) == size for s, size in _abi.STRUCT_SIZES.values())
    assert got[-5:] == [_abi.EDIT_TRIM, _abi.EDIT_REVERSE, _abi.EDIT_LINEAR, _abi.EDIT_SQRT, _abi.EDIT_SMOOTH] == [er.TRIM, er.REVERSE, er.LINEAR, er.SQRT, er.SMOOTH]
    assert got[2:-5] == list(range(0, 40, 4)) + list(range(0, 48, 4))


def test_edit_kernels_have_no_scratch_memory_and_the_render_kernel_no_lds(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_edit_kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resources of zl_edit.hip's kernels"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    scan = [r for n, r in rows.items() if "zl_k_edit_scan" in n]
    render = [r for n, r in rows.items() if "zl_k_edit_render" in n]
    assert len(scan) == 1 and len(render) == 1 and len(rows) == 2, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    assert render[0]["lds"] == 0 and render[0]["vgprs"] <= 32 and render[0]["waves"] >= 8, rows
    assert scan[0]["lds"] == 2 * 4 * 4 and scan[0]["vgprs"] <= 32 and scan[0]["waves"] >= 8, rows       # eight words for the reduction


# ---- the walk under the sanitizers ------------------------------------------------------------------------------------------------------
def test_harness_walk_under_the_sanitizers(tmp_path):
    """tests/cpp/edit_check.cpp: the harness walk over random calls with buffers of exactly the size needed, built with AddressSanitizer
    and UBSan.  The sanitizers' runtimes are linked into the program (-static-lib*san), so it runs whatever else the environment loads
    in front of it."""
    exe = str(tmp_path / "edit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-I", os.path.join(ROOT, "libzl_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edit_check.cpp"), "-o", exe])
    for args in (["1", "60"], ["2", "60"]):
        rc = subprocess.run([exe] + args, capture_output=True, text=True)
        assert rc.returncode == 0 and rc.stderr == "", rc.stdout + rc.stderr
        assert "edit check ok" in rc.stdout
