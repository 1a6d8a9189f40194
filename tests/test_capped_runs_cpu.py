"""Runs of items that cross records ("The run"), CPU tier: the restated run formula covers a call exactly once,
every case of tests/run_cases.py reaches the regime it is there for, its item counts are the project's own (the host builds of
zl_overview.h, zl_onset.h and zl_decode.h) and the restatements give it an answer worth comparing.  The kernels' copies of the run
logic exist in three .hip files and nowhere else: tests/test_capped_runs_gpu.py runs the same cases through them."""
import ctypes as C

import numpy as np
import pytest

import decode_ref as dr
import run_cases as rc
from libzl_amd import build

CASES = {"onset": rc.onset_case, "overview": rc.overview_case, "decode": rc.decode_case}
IDS = [f"{t}_items" for t in rc.TOTALS]


def test_the_caps_are_the_ones_the_totals_are_written_for():
    for service in rc.SERVICES:
        s = rc.launch_shape(service)
        assert s["MAX_BLOCKS"] * s["THREADS"] // s["WAVE"] == 16384, (service, s)
        assert rc.grid_waves(service, 16383) == 16384 and rc.grid_waves(service, 16381) == 16384 and rc.grid_waves(service, 16380) == 16380
        assert rc.grid_waves(service, 1) == 4 and rc.grid_waves(service, 10 ** 6) == 16384


def test_partition_covers_every_item_once_in_wave_order():
    nwaves = 16384
    for items in range(1, 70001):
        it, end = rc.partition(items, nwaves)
        # consecutive, in wave order, from 0 to items: every item lies in exactly one run
        assert it[0] == 0 and end[-1] == items and np.array_equal(it[1:], end[:-1]), items
        n = end - it
        if items < nwaves:
            assert n[:items].all() and not n[items:].any(), items  # one item each, then the trailing waves' empty runs
        else:
            q = items // nwaves
            assert n.min() == q and n.max() == q + (1 if items % nwaves else 0), items
    # the formula itself in Python's integers, wave by wave
    for items in (1, 5, 16383, 16384, 16385, 32767, 49157, 69999):
        it, end = rc.partition(items, nwaves)
        q, rem = divmod(items, nwaves)
        assert [int(v) for v in it[:40]] == [w * q + min(w, rem) for w in range(40)]
        assert [int(v) for v in end[-40:]] == [w * q + min(w, rem) + q + (1 if w < rem else 0) for w in range(nwaves - 40, nwaves)]
    # a smaller grid (fewer items than the cap's waves): the launch's own wave count
    for items in (1, 2, 3, 4, 5, 63, 1001):
        it, end = rc.partition(items, rc.grid_waves("onset", items))
        assert it[0] == 0 and end[-1] == items and np.array_equal(it[1:], end[:-1]) and (end - it).max() == 1


@pytest.mark.parametrize("total", list(rc.TOTALS), ids=IDS)
@pytest.mark.parametrize("service", list(CASES))
def test_every_case_reaches_its_regime(service, total):
    c = CASES[service](total)
    f = rc.case_facts(c)
    q, rem = rc.TOTALS[total]
    assert c["nwaves"] == 16384 and int(c["items"].sum()) == total
    assert (f["q"], f["rem"]) == (q, rem), f
    longest = q + (1 if rem else 0)
    assert f["longest"] == longest
    # a longest run advances to the next record at every step: it touches as many records as it holds items
    assert f["max_records"] == longest and f["full_advance"], f
    # the bisection lands on a record's first item, and inside a record
    assert f["on_base"] and f["off_base"], f
    if longest == 1:
        assert f["crossing"] == 0                                  # a run is one item: nothing to cross, every item a bisection
    elif total == 16385:
        assert f["crossing"] == 1                                  # wave 0 alone holds two items: the call's first two records
    else:
        assert f["crossing"] > 100 and f["mid_to_later"], f        # runs that begin inside a long record and end in a later one
    if longest >= 4:
        assert f["mid_through"], f                                 # ... and pass whole records on the way
    if total == 8 * 16384 + 3:
        assert f["max_records"] >= 8, f
    # a stretch of at least eight one-item records; the call's first and last record hold one item
    ones = "".join("1" if n == 1 else "0" for n in c["items"])
    assert "1" * 8 in ones and c["items"][0] == 1 and c["items"][-1] == 1
    rc.limits(c)
    if service == "overview":
        o = rc.overview_facts(c)
        if longest >= 3 and total != 32769:
            assert o["forms_in_one_run"] == 3, o                   # narrow, one piece per column, several pieces: one run sees all
        if longest >= 2 and total != 16385:
            assert {(0, 1), (1, 2), (2, 0)} <= o["steps"], o       # every step of narrow -> one piece -> several -> narrow inside some run
        assert o["whole_pass"] == (total == 8 * 16384 + 3), o      # the whole pass and back needs five items
    if service == "decode":
        d = rc.decode_facts(c)
        assert d["quartet_starts_a_run"], d
        # the four verdict pieces lie in one run wherever a run holds four items; shorter runs cut them at their own length
        assert d["quartet_runs"] == (1 if longest >= 4 else {1: 4, 2: 2, 3: 2}[longest] if total != 16385 else 3), d
        # a non-finite item behind another piece's item in the same run: where the verdict must go to R.verdict, not to the run's first piece
        assert d["poison_behind_a_clean_piece"] == (total in (32767, 32768, 3 * 16384 + 5, 8 * 16384 + 3)), d


def test_neighbours_differ_in_channels_source_and_parameters():
    c = rc.onset_case(32769)
    chans = [rc.ON_LENGTHS[s[0]][0] for s in c["specs"]]
    assert sum(a != b for a, b in zip(chans, chans[1:])) > 200 and sum(a[0] != b[0] for a, b in zip(c["specs"], c["specs"][1:])) > 300
    assert {s[3] for s in c["specs"]} == {64, 80, 256, 4096} and {s[1] for s in c["specs"]} == {0, 1, 2, 3, 5}
    assert sum(a[3] != b[3] for a, b in zip(c["specs"], c["specs"][1:])) > 200                   # the hop changes inside runs
    c = rc.overview_case(32769)
    chans = [rc.OV_CLIPS[s[0]][0] for s in c["specs"]]
    assert sum(a != b for a, b in zip(chans, chans[1:])) > 300 and set(c["forms"]) == {0, 1, 2}
    assert (0, 4096, 1, 3) in c["specs"] and all((2 + i % 2, col, first, n) in c["specs"] for i, (n, col, first) in enumerate(rc.OV_PIECES))
    c = rc.decode_case(32769)
    assert {s[0] for s in c["specs"]} == set(dr.FORMATS) and {s[1] for s in c["specs"]} == {1, 2, 3}
    assert sum(min(2, a[1]) != min(2, b[1]) for a, b in zip(c["specs"], c["specs"][1:])) > 200
    # the last item of a piece: exactly 64 groups, and fewer
    groups = [((s[2] + dr.PAD) * min(2, s[1]) + 3) // 4 for s in c["specs"]]
    assert sum(g % 64 == 0 for g in groups) > 50 and sum(g % 64 != 0 for g in groups) > 50
    assert [c["specs"][i][3] for i in c["quartet"]] == ["f32_inf", "s16", "f32_clean", "f64_1e300"]


def _harness(builder, **fns):
    lib = C.CDLL(builder())
    for name, (res, args) in fns.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


@pytest.mark.parametrize("total", list(rc.TOTALS), ids=IDS)
def test_item_counts_are_the_headers_own(total):
    on = _harness(build.build_onset_harness, zlon_hops=(C.c_int64, [C.c_int64, C.c_int64]))
    c = rc.onset_case(total)
    assert [on.zlon_hops(n, hop) for _, _, n, hop in c["specs"]] == list(c["items"])
    o = _harness(build.build_overview_harness, zlov_items=(C.c_int64, [C.c_int64, C.c_int64]), zlov_pieces_per_column=(C.c_int32, [C.c_int64, C.c_int64]))
    c = rc.overview_case(total)
    assert [o.zlov_items(n, col) for _, col, _, n in c["specs"]] == list(c["items"])
    assert [min(2, o.zlov_pieces_per_column(n, col)) for _, col, _, n in c["specs"]] == c["forms"]
    # decode: the header's own cut of the call at the default stage -- one pass, one piece per clip, the pieces' item_base and items
    d = _harness(build.build_decode_harness, zldec_plan=(C.c_int32, [C.c_int32] + [C.c_void_p] * 3 + [C.c_int64, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(C.c_int32)]))
    c = rc.decode_case(total)
    n = len(c["specs"])
    fmts, chans, lengths = (np.array([s[i] for s in c["specs"]], np.int32) for i in (0, 1, 2))
    clip, pas, base, items = (np.full(n + 8, -1, np.int32) for _ in range(4))
    npasses = C.c_int32(0)
    got = d.zldec_plan(n, lengths.ctypes.data, chans.ctypes.data, fmts.ctypes.data, rc.header_value("decode", "STAGE_DEFAULT"), n + 8,
                       clip.ctypes.data, pas.ctypes.data, base.ctypes.data, items.ctypes.data, C.byref(npasses))
    assert got == n and npasses.value == 1 and np.array_equal(clip[:n], np.arange(n)) and not pas[:n].any()
    assert np.array_equal(base[:n], c["bases"]) and np.array_equal(items[:n], c["items"])


def test_the_restatements_give_every_case_an_answer():
    for i, x in enumerate(rc.onset_sources() + rc.overview_sources()):
        assert np.count_nonzero(x) > 0.99 * x.size, i                                            # no silence
    assert np.abs(rc.onset_poison()).min() > 7.0
    for total in rc.TOTALS:
        c = rc.onset_case(total)
        long_ = [s for s, n in zip(c["specs"], c["items"]) if n >= 64]
        assert any(len(rc.onset_want(s)[0]) == 1 for s in long_), total                            # a request of the list has an onset
        assert any(int(rc.onset_want(s)[1].max()) > 0 for s in c["specs"][:20])
        # no hop of a case reaches the poison's energy
        assert max(int(rc.onset_want(s)[1].max()) for s in long_) < rc.onset_poison_energy() == 64 * 32358 ** 2
        c = rc.overview_case(total)
        for s in c["specs"][:40]:
            lo, hi = rc.OV_CLIPS[s[0]][2]
            want = rc.overview_want(s)
            assert want.min() >= np.float32(lo) and want.max() <= np.float32(hi) and want.shape == (s[1], 4)
        c = rc.decode_case(total)
        for placement in rc.PLACEMENTS:
            flags = [rc.decode_want(s, placement)[1] for s in c["specs"]]
            assert [i for i, ok in enumerate(flags) if not ok] == [c["quartet"][0], c["quartet"][3]], (total, placement)
            for i in (c["quartet"][0], c["quartet"][3]):
                # the non-finite sample lies in the last / the first item of its piece
                ext = rc.decode_want(c["specs"][i], placement)[0]
                bad = np.flatnonzero((ext & np.uint32(0x7F800000)) == np.uint32(0x7F800000))
                assert len(bad) == 1 and bad[0] // 256 == (c["items"][i] - 1 if placement == "last" else 0), (total, placement, bad)
            assert any(rc.decode_want(s, placement)[0].any() for s in c["specs"][:8])
            # the clips that lie in the extents before the call: the same sizes and formats, other values, all finite
            other = rc.decode_sources(c, placement, seed=1)
            real = rc.decode_sources(c, placement)
            assert all(a[0].size == b[0].size and a[1:] == b[1:] and not np.array_equal(a[0], b[0]) for a, b in zip(other, real) if a[0].size >= 8)
