"""Transient detection, CPU tier: the host build of libzl_amd/csrc/zl_onset.h (tests/cpu_harness/onset_host.cpp walks a request the way
the kernels do, with the header's own arithmetic) against the numpy / Python-integer restatement (tests/onset_ref.py) -- the level,
the hops' energy with its masked 16-byte groups, pick and select on hand-made energies, the defaults and the limits -- and the new
kernels' resources.  tests/test_onset_gpu.py holds the kernels themselves to the restatement on the GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import onset_ref as onr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 8
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4099)
FIRSTS = (0, 1, 2, 3, 5)
TAILS = (0, 1, 2, 3, 5)
HOPS = (64, 80, 256, 4096)

_lib = None
_z = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_onset_harness())
        l.zlon_level.restype = C.c_int32
        l.zlon_level.argtypes = [C.c_uint64]
        l.zlon_resolve.restype = C.c_int32
        l.zlon_resolve.argtypes = [C.c_double, C.c_void_p]
        l.zlon_q.restype = C.c_int32
        l.zlon_q.argtypes = [C.c_float]
        l.zlon_energy.restype = C.c_int64
        l.zlon_energy.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        l.zlon_pick.restype = C.c_int32
        l.zlon_pick.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        l.zlon_refine.restype = C.c_int32
        l.zlon_refine.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64]
        _lib = l
    return _lib


def zlhip():
    global _z
    if _z is None:
        _z = _abi.bind(C.CDLL(build.build_engine()))
    return _z


# ---- the level ----------------------------------------------------------------------------------------------------------------------
def test_level_against_exact_integers():
    l = lib()
    xs = [1, 2, 3, 63, 64, 65]
    for k in range(1, 45):
        xs += [v for v in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= v <= 2 ** 44]
    for x in xs:
        p = x.bit_length() - 1
        want = 64 * p + ((x - 2 ** p) * 64) // 2 ** p
        got = l.zlon_level(x)
        assert got == want == onr.level(x), (x, got, want)
        assert isinstance(got, int) and 0 <= got < 64 * 45         # the stored result is the defined int32
    assert l.zlon_level(1) == 0 and l.zlon_level(2) == 64 and l.zlon_level(3) == 96 and l.zlon_level(2 ** 44 - 1) == 64 * 44 - 1


def test_level_is_monotone_on_random_values():
    l = lib()
    rng = np.random.default_rng(5)
    xs = np.unique(np.concatenate([rng.integers(1, 2 ** 44, 4000), (2.0 ** rng.uniform(0, 44, 4000)).astype(np.int64) + 1]))
    lv = [l.zlon_level(int(x)) for x in xs]
    assert all(b >= a for a, b in zip(lv, lv[1:]))
    assert lv == [onr.level(int(x)) for x in xs]


# ---- the energy pass ----------------------------------------------------------------------------------------------------------------
def extent(planar):
    """the arena extent of a sound: interleaved, 8 zero frames behind it, rounded up to 16 bytes"""
    ch, length = planar.shape
    words = ((length + PAD) * ch + 3) & ~3
    ext = np.zeros(words, np.float32)
    ext[:length * ch] = planar.T.reshape(-1)
    return ext


def run_energy(planar, first, n, hop):
    ch = planar.shape[0]
    ext = extent(planar)
    visits = np.zeros(ext.size, np.int32)
    E = np.zeros(-(-n // hop), np.uint64)
    top = lib().zlon_energy(ext.ctypes.data, ch, first, n, hop, visits.ctypes.data, E.ctypes.data)
    return E, visits, top, ext


@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("first", FIRSTS)
def test_energy_equals_the_restatement_and_every_word_is_visited_once(ch, first):
    rng = np.random.default_rng(11 + first)
    for n, tail, hop in itertools.product(LENGTHS, TAILS, HOPS):
        length = first + n + tail
        # full-scale neighbours: a frame in front of or behind the request that leaked into a sum would show
        x = rng.uniform(-1.0, 1.0, (ch, length)).astype(np.float32)
        x[:, :first] = 7.9
        x[:, first + n:] = -7.9
        E, visits, top, ext = run_energy(x, first, n, hop)
        assert 0 <= top < ext.size, (n, tail, hop, "a load leaves the extent")
        expect = np.zeros(ext.size, np.int32)
        expect[first * ch:(first + n) * ch] = 1
        assert np.array_equal(visits, expect), (n, tail, hop, np.flatnonzero(visits != expect)[:8])
        assert np.array_equal(E, onr.energy(x, first, n, hop)), (n, tail, hop)


def test_energy_of_special_values():
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                     0xFFFFFFFF, 0x3F800000, 0x41000000, 0xC1000000, 0x39000000, 0x38FFFFFF, 0x39C00000], np.uint32)
    want = [0, 0, 0, 0, 0, 32767, -32767, 0, 0, 0, 0, 4096, 32767, -32767, 0, 0, 2]
    x = bits.view(np.float32)
    assert [lib().zlon_q(float(v)) for v in x[:7]] == want[:7]
    assert list(onr.quantise(x)) == want
    E, *_ = run_energy(np.tile(x, 8)[None, :], 0, 8 * x.size, 64)
    assert int(E.sum()) == 8 * sum(v * v for v in want)


# ---- pick and select on hand-made energies ------------------------------------------------------------------------------------------
def energies_for(levels, F):
    """E with L(E[h] + F) = levels[h] (the smallest x of that level, minus F)"""
    out = []
    for lv in levels:
        p, m = divmod(lv, 64)
        x = 2 ** p + -(-m * 2 ** p // 64)
        assert onr.level(x) == lv and x >= F
        out.append(x - F)
    return np.array(out, np.uint64)


def pick(E, F, threshold, gap, max_onsets):
    hops = len(E)
    N = np.zeros(hops, np.int32); kept = np.full(max_onsets, -1, np.int32); cand = np.zeros(hops, np.uint8)
    n = lib().zlon_pick(E.ctypes.data, hops, F, threshold, gap, max_onsets, N.ctypes.data, kept.ctypes.data, cand.ctypes.data)
    rN = onr.novelty(E, F)
    rc = onr.candidates(rN, threshold, gap)
    assert np.array_equal(N, rN)
    assert list(np.flatnonzero(cand)) == rc
    assert list(kept[:n]) == onr.select(rN, rc, max_onsets)
    return N, list(np.flatnonzero(cand)), list(kept[:n])


F0 = 64 * 2 * 8 * 8        # hop 64, stereo, gate 8: level 832
BASE = onr.level(F0)


def test_a_plateau_of_equal_strength_inside_one_window_keeps_the_earliest():
    # rises of 200 at hops 2, 4 and 6 (back down in between): equal N, all within min_gap 4 of each other
    lv = [BASE, BASE, BASE + 200, BASE, BASE + 200, BASE, BASE + 200, BASE, BASE, BASE, BASE, BASE]
    N, cand, kept = pick(energies_for(lv, F0), F0, 128, 4, 8)
    assert [int(N[h]) for h in (2, 4, 6)] == [200, 200, 200]
    assert cand == [2] and kept == [2]
    # min_gap 1: they are two hops apart, so each stands alone
    N, cand, kept = pick(energies_for(lv, F0), F0, 128, 1, 8)
    assert cand == [2, 4, 6] and kept == [2, 4, 6]


def test_equal_strengths_across_windows_keep_the_earliest_when_there_are_too_many():
    lv = [BASE] * 64
    for h in range(3, 64, 6):
        lv[h] = BASE + 300
    lv[27] = BASE + 500                                            # one stronger, in the middle
    E = energies_for(lv, F0)
    N, cand, kept = pick(E, F0, 128, 2, 64)
    assert cand == list(range(3, 64, 6)) == kept
    N, cand, kept = pick(E, F0, 128, 2, 4)
    assert kept == [3, 9, 15, 27]                                  # the strongest, and of the equal ones the first three
    N, cand, kept = pick(E, F0, 128, 2, 1)
    assert kept == [27]
    N, cand, kept = pick(E, F0, 128, 2, len(cand))
    assert kept == cand


def test_threshold_exactly_at_the_strength():
    lv = [BASE, BASE, BASE + 128, BASE + 128, BASE, BASE + 127, BASE]
    E = energies_for(lv, F0)
    N, cand, kept = pick(E, F0, 128, 1, 8)
    assert int(N[2]) == 128 and int(N[5]) == 127 and cand == [2]
    assert pick(E, F0, 129, 1, 8)[1] == []
    assert pick(E, F0, 127, 1, 8)[1] == [2, 5]


def test_windows_are_cut_at_both_ends():
    # hop 0 rises from E[-1] = 0 (the floor's level); the last hop has nothing behind it; min_gap longer than the request
    lv = [BASE + 400, BASE, BASE, BASE, BASE + 300]
    E = energies_for(lv, F0)
    for gap in (1, 2, 3, 4, 5, 7, 1024):
        N, cand, kept = pick(E, F0, 128, gap, 8)
        assert cand == ([0, 4] if gap < 4 else [0]), gap
    lv = [BASE, BASE, BASE, BASE, BASE + 300]
    for gap in (1, 3, 1024):
        assert pick(energies_for(lv, F0), F0, 128, gap, 8)[1] == [4]
    assert pick(energies_for([BASE + 200], F0), F0, 128, 10, 1)[2] == [0]


def test_pick_on_random_strengths_with_many_ties():
    rng = np.random.default_rng(3)
    for hops, gap, keep in ((1, 1, 1), (2, 1, 1), (257, 1, 16), (1000, 3, 7), (1000, 10, 128), (1500, 64, 1024), (5000, 1, 1024), (3000, 1024, 4)):
        lv = BASE + rng.integers(0, 6, hops) * 130
        pick(energies_for([int(v) for v in lv], F0), F0, 128, gap, keep)


# ---- refine -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_refine_walks_the_sub_blocks_of_two_hops(ch):
    rng = np.random.default_rng(9)
    for hop, first, n in ((64, 0, 1000), (80, 3, 997), (256, 5, 4099), (4096, 1, 9000)):
        x = (rng.uniform(-1, 1, (ch, first + n + 2)) * 1e-3).astype(np.float32)
        hits = sorted(int(v) for v in rng.integers(first, first + n, 4))
        for f in hits:
            x[:, f:f + 40] += rng.uniform(-0.8, 0.8, (ch, x[:, f:f + 40].shape[1])).astype(np.float32)
        e = onr.frame_energy(x)
        E = onr.energy(x, first, n, hop)
        F = hop * ch * 64
        ext = extent(x)
        for h in range(len(E)):
            got = lib().zlon_refine(ext.ctypes.data, ch, first, n, hop, h, E.ctypes.data, F)
            assert got == onr.refine(e, E, F, first, n, hop, h), (hop, h)


# ---- defaults and limits ------------------------------------------------------------------------------------------------------------
def resolve(sr, **kw):
    r = _abi.OnsetRequest(0, kw.pop("first_frame", 0), kw.pop("num_frames", 1000), kw.get("hop", 0), kw.get("gate", 0), kw.get("threshold", 0),
                          kw.get("min_gap", 0), kw.get("max_onsets", 0))
    before = bytes(r)
    rc = zlhip().zlhip_onset_resolve(sr, C.byref(r))
    if rc != 0:
        assert rc == _abi.ZLHIP_ERR_INVALID and bytes(r) == before     # a refused request is left as it was
        return None
    return dict(hop=r.hop_frames, gate=r.gate, threshold=r.threshold, min_gap=r.min_gap_hops, max_onsets=r.max_onsets)


def test_defaults():
    want = {8000: (64, 7), 44100: (240, 10), 48000: (256, 10), 96000: (512, 10), 192000: (1024, 10)}
    for sr, (hop, gap) in want.items():
        got = resolve(float(sr))
        assert got == dict(hop=hop, gate=8, threshold=128, min_gap=gap, max_onsets=128) == onr.resolve(sr), sr
        five = (C.c_int32 * 5)()
        assert lib().zlon_resolve(float(sr), five) == 0 and list(five) == [hop, 8, 128, gap, 128]
    # a given field stays, the others still resolve (min_gap from the given hop)
    assert resolve(48000.0, hop=4096, max_onsets=3) == dict(hop=4096, gate=8, threshold=128, min_gap=1, max_onsets=3) == onr.resolve(48000, hop=4096, max_onsets=3)
    assert resolve(48000.0, hop=64)["min_gap"] == 38 == onr.resolve(48000, hop=64)["min_gap"]
    # nothing to derive from the rate: it is not looked at
    assert resolve(0.0, hop=64, min_gap=1) == dict(hop=64, gate=8, threshold=128, min_gap=1, max_onsets=128)
    assert resolve(0.0) is None and resolve(float("nan")) is None and resolve(-48000.0) is None


def test_every_limit_either_side():
    ok = dict(hop=256, gate=8, threshold=128, min_gap=10, max_onsets=128)
    limits = {"hop": ((64, 4096, 80, 4080), (48, 63, 65, 72, 4097, 4112, -256)), "gate": ((1, 32767), (-1, 32768)),
              "threshold": ((1, 4096), (-1, 4097)), "min_gap": ((1, 1024), (-1, 1025)), "max_onsets": ((1, 1024), (-1, 1025))}
    for field, (good, bad) in limits.items():
        for v in good:
            assert resolve(48000.0, **dict(ok, **{field: v})) == dict(ok, **{field: v}) == onr.resolve(48000, **dict(ok, **{field: v})), (field, v)
        for v in bad:
            assert resolve(48000.0, **dict(ok, **{field: v})) is None and onr.resolve(48000, **dict(ok, **{field: v})) is None, (field, v)
    assert resolve(48000.0, num_frames=1, **ok) == ok and resolve(48000.0, num_frames=0, **ok) is None and resolve(48000.0, num_frames=-5, **ok) is None
    assert resolve(48000.0, first_frame=0, **ok) == ok and resolve(48000.0, first_frame=-1, **ok) is None
    # 65536 hops per request
    small = dict(ok, hop=64)
    assert resolve(48000.0, num_frames=65536 * 64, **small) == small and resolve(48000.0, num_frames=65536 * 64 + 1, **small) is None
    assert zlhip().zlhip_onset_resolve(48000.0, None) == _abi.ZLHIP_ERR_INVALID


def test_the_entry_points_refuse_a_null_engine():
    z = zlhip()
    r = _abi.OnsetRequest(0, 0, 100, 0, 0, 0, 0, 0)
    out = np.full((4, 2), -7, np.int32); n = C.c_int32(-7)
    assert z.zlhip_sound_onsets(None, C.byref(r), out.ctypes.data, 4, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_sound_onsets_batch(None, C.byref(r), 1, out.ctypes.data, 4, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_onset_hops(None, 0, None, None, 0, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_debug_onset_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID
    assert z.zlhip_group_sound_onsets_batch(None, C.byref(r), 1, out.ctypes.data, 4, C.byref(n)) == _abi.ZLHIP_ERR_INVALID
    assert (out == -7).all() and n.value == -7


def test_onset_struct_layouts(tmp_path):
    prog = tmp_path / "p.c"
    fields = ["id", "first_frame", "num_frames", "hop_frames", "gate", "threshold", "min_gap_hops", "max_onsets"]
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){printf("%d %d %d %d %d",(int)sizeof(zlhip_onset_request),'
                    '(int)sizeof(zlhip_onset),(int)offsetof(zlhip_onset,frame),(int)offsetof(zlhip_onset,strength),ZLHIP_ONSET_MAX_ONSETS);'
                    + "".join('printf(" %%d",(int)offsetof(zlhip_onset_request,%s));' % f for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R, O = _abi.OnsetRequest, _abi.Onset
    assert got == [C.sizeof(R), C.sizeof(O), O.frame.offset, O.strength.offset, _abi.ONSET_MAX_ONSETS] + [getattr(R, f).offset for f in fields]
    assert got == [32, 8, 0, 4, 1024, 0, 4, 8, 12, 16, 20, 24, 28]


def test_onset_kernels_have_no_scratch_memory(built):
    build.build_engine()
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_onset_kernel_resources.txt")
    assert os.path.exists(path), "no zl_onset kernel resources file"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    energy = [r for n, r in rows.items() if "zl_k_onset_energy" in n]
    rest = [r for n, r in rows.items() if "zl_k_onset_pick" in n]
    assert len(energy) == 1 and len(rest) == 1 and len(rows) == 2, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, rows
    assert energy[0]["lds"] == 0, rows
    assert energy[0]["waves"] >= 8, rows                           # the energy pass hides HBM latency with resident waves
