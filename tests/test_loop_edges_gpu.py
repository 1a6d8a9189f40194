"""Loop finder, GPU tier, the edges: exact ties through every step of the reduction, a loud neighbour behind a strip that touches the
sound's first or last frame, re-rendered and rate-converted data, a grown arena, the two call limits from the accepting side, empty
requests at a call's ends, the buffers' first allocation and the resident real-time kernel.  Everything is compared as
tests/test_loop_gpu.py compares it (tests/loop_checks.py): costs, item records and every integer of the result bit for bit with the
numpy / Python-integer restatement (tests/loop_ref.py), the three dB fields within 1e-9.  Clips of at most 24000 frames but for the
grown arena's."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_ref as lr
import rt_between_cycles as rtc
from loop_checks import SR, check_batch, played, same, upload, want

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=64, sound_arena_bytes=16 << 20)
    yield s
    s.close()


# ---- exact ties ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tie_bank(syn):
    """lr.ties() uploaded once (a signal several cases share is one clip), two clips for the empty requests, and the restatements"""
    cases = lr.ties()
    by_array, srcs = {}, {}
    for _, x, _ in cases:
        if id(x) not in by_array:
            by_array[id(x)] = upload(syn, x)
            srcs[by_array[id(x)]] = x
    reqs = [dict(q, clip=by_array[id(x)]) for _, x, q in cases]
    short = lr.square(16, 40)                                      # shorter than the window: no candidates
    sid = upload(syn, short)
    srcs[sid] = short
    zid = reqs[[what for what, _, _ in cases].index("silence")]["clip"]
    empties = [dict(clip=sid, start_frame=0, stop_frame=40, window=64),
               dict(clip=zid, start_frame=5000, stop_frame=5010, start_search=-1, stop_search=-1, window=64)]      # one pair below min_length
    yield dict(cases=cases, reqs=reqs, srcs=srcs, empties=empties, cache={})
    for cid in srcs:
        syn.unregister_clip(cid)


def test_every_tie_case_as_its_own_call(syn, tie_bank):
    """lr.ties(), one clip_loop per case: the winner lies in five different items and in every wave of the pairs workgroup, and the
    distance, the smaller start and the smaller end each decide some of them (tests/test_loop_cpu.py asserts that of the list)"""
    for (what, _, _), r in zip(tie_bank["cases"], tie_bank["reqs"]):
        bad, outs = check_batch(syn, [r], tie_bank["srcs"], cache=tie_bank["cache"])
        assert not bad, (what, bad)
        assert outs[0] == syn.clip_loop(**r) and outs[0]["found"] == 1 and outs[0]["cost"] == 0, (what, outs[0])
    for r in tie_bank["empties"]:
        bad, outs = check_batch(syn, [r], tie_bank["srcs"], cache=tie_bank["cache"])
        assert not bad and all(v == 0 for v in outs[0].values()), (r, bad, outs)


def test_the_tie_cases_in_one_call_between_empty_requests(syn, tie_bank):
    """all of them in ONE clip_loop_batch with an empty request first, last and twice in a row in the middle (zl_lp_find's bisection at
    its edges: a request without items shares its item_base with the next one): costs, items and results equal the restatement's, and
    the results equal the single calls'"""
    reqs, (e0, e1) = tie_bank["reqs"], tie_bank["empties"]
    half = len(reqs) // 2
    call = [e0] + reqs[:half] + [e1, e0] + reqs[half:] + [e1]
    assert sum(lr.tie_facts(x, SR, q)["items"] for _, x, q in tie_bank["cases"]) > 200
    bad, outs = check_batch(syn, call, tie_bank["srcs"], cache=tie_bank["cache"])
    assert not bad, (len(bad), bad[:3])
    empty = (0, half + 1, half + 2, len(call) - 1)
    assert [i for i, o in enumerate(outs) if o["found"] == 0] == list(empty)
    assert syn.loop_items(0) == [] and syn.loop_items(half + 2) == [] and len(syn.loop_items(half + 1)) == 1 and len(syn.loop_items(len(call) - 1)) == 1
    singles = [syn.clip_loop(**r) for r in call]
    assert singles == outs


# ---- a neighbour does not leak --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2], ids=["mono", "stereo"])
def test_a_neighbour_does_not_leak(built, ch):
    """a quiet clip between two full-scale ones in a small arena that held noise; the start strip begins at the quiet clip's frame 0
    and the end strip ends at its last frame, whose 16-byte group lies partly behind the data: a neighbour's frame in a head or tail
    group would change the shift and every cost (a full-scale frame is 2000 times a quiet one)"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=2 << 20) as s:
        rng = np.random.default_rng(9)
        fill = [upload(s, rng.uniform(-7.9, 7.9, (ch, 60000)).astype(f32)) for _ in range(3)]
        for cid in fill:
            s.unregister_clip(cid)
        for n in (6001, 3333):
            loud = [rng.choice([-7.9, 7.9], (ch, m)).astype(f32) for m in (3001, 3003)]
            quiet = lr.tone(77.0, ch, n, level=0.004, noise=0.0002, seed=n)
            ids = [upload(s, x) for x in (loud[0], quiet, loud[1])]
            srcs = dict(zip(ids, (loud[0], quiet, loud[1])))
            reqs = []
            for W in (16, 256, 1024):
                H = W // 2
                R = H + 20
                for cid in (ids[1], ids[0], ids[2]):
                    reqs.append(dict(clip=cid, start_frame=H // 2 + 3, stop_frame=srcs[cid].shape[1], start_search=R, stop_search=R, window=W))
                assert reqs[-1]["start_frame"] <= R
            bad, outs = check_batch(s, reqs, srcs)
            assert not bad, bad
            for k, (r, o) in enumerate(zip(reqs, outs)):
                H = r["window"] // 2
                assert o["found"] == 1 and o["starts"] == H // 2 + 24 and o["ends"] == 21, (r, o)       # [H, s0 + R] and [length - H - 20, length - H]
                assert (o["shift"] == 0) if k % 3 == 0 else (o["shift"] >= 5), (r, o)
            for cid in ids:
                s.unregister_clip(cid)


# ---- the data that plays --------------------------------------------------------------------------------------------------------------
def test_loop_follows_the_rendered_data(syn):
    """after a re-render (gain and pitch) the answer comes from the data that plays and the range is checked against it; after a rate
    conversion the default radius is that of the new rate"""
    from libzl_amd import ZlHipError
    src = lr.tone(218.4, 2, 24000, seed=17)
    cid = upload(syn, src)
    r = dict(clip=cid, start_frame=6000, stop_frame=18011, start_search=100, stop_search=90, window=128)
    bad, outs = check_batch(syn, [r], {cid: src})
    assert not bad, bad
    before = outs[0]
    syn.rerender_clip(cid, pitch=3.0, gain_db=-6.0)
    now = played(syn, cid)
    assert now.shape[1] == 24000 and not np.array_equal(now[:, :4000], src[:, :4000])
    bad, outs = check_batch(syn, [r, dict(r, start_frame=3, stop_frame=24000, window=16)], {cid: now})
    assert not bad, bad
    assert outs[0] != before and outs[0]["found"] == 1
    syn.rerender_clip(cid, speed=2.0)
    now = played(syn, cid)
    assert now.shape[1] == 12000
    with pytest.raises(ZlHipError):                                # the range is checked against the data that plays
        syn.clip_loop(**r)
    with pytest.raises(ZlHipError):
        syn.clip_loop(cid, 3000, 12001, 100, 90, 128)
    bad, _ = check_batch(syn, [dict(r, start_frame=3000, stop_frame=12000)], {cid: now})
    assert not bad, bad
    syn.rerender_clip(cid)                                         # identity: the original upload plays again
    assert syn.clip_loop(**r) == before
    syn.unregister_clip(cid)
    # a 44.1 kHz clip: the default radius is 441, after the conversion to 48 kHz it is 480
    low = lr.tone(200.0, 1, 22050, seed=18)
    cid = upload(syn, low, 44100.0)
    r = dict(clip=cid, start_frame=5000, stop_frame=15000)
    bad, outs = check_batch(syn, [r], {cid: low}, rates={cid: 44100.0})
    assert not bad, bad
    assert outs[0]["starts"] == outs[0]["ends"] == 883
    syn.convert_clips([cid], SR)
    now = played(syn, cid)
    assert syn.clip_info(cid)["sample_rate"] == SR and abs(now.shape[1] - 24000) <= 2
    bad, outs = check_batch(syn, [r], {cid: now})
    assert not bad, bad
    assert outs[0]["starts"] == outs[0]["ends"] == 961 and outs[0]["found"] == 1
    syn.unregister_clip(cid)


# ---- a grown arena ----------------------------------------------------------------------------------------------------------------------
def test_a_clip_in_a_grown_arena(built):
    from libzl_amd import SamplerSynth
    arena = 1 << 20
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=16, sound_arena_bytes=arena) as s:
        srcs = [lr.tone(60.0 + 11 * i, 1 + i % 2, 60000 + 1001 * i, seed=40 + i) for i in range(8)]
        ids = [upload(s, x) for x in srcs]
        assert s.memory_bytes()[1] >= 3 * arena                    # the arena grew
        # from near the first frame (the first clip) to near the last one: the end range is clipped at the data's end
        reqs = [dict(clip=cid, start_frame=3 + 7000 * i, stop_frame=x.shape[1] - (5 if i % 3 == 0 else 520) - i, start_search=40 + i, stop_search=33, window=(16, 256, 1024)[i % 3])
                for i, (cid, x) in enumerate(zip(ids, srcs))]
        bad, outs = check_batch(s, reqs, dict(zip(ids, srcs)))
        assert not bad, bad
        assert all(o["found"] == 1 for o in outs) and [o["ends"] for o in outs[:3]] == [31, 67, 44]


# ---- the call limits, from the accepting side -------------------------------------------------------------------------------------------
def test_the_item_limit_is_accepted(syn):
    """16 requests of 4095 x 4095 candidates: 16 x 4096 = 65536 work items, the call's limit (one more request is refused:
    tests/test_loop_gpu.py::test_errors_leave_out_untouched); the last request's items lie at the largest item_base"""
    from libzl_amd import ZlHipError
    src = lr.tone(97.3, 1, 8400, seed=21)
    cid = upload(syn, src)
    r = dict(clip=cid, start_frame=2100, stop_frame=6300, start_search=2047, stop_search=2047, window=16, min_length=1)
    res, items, _ = want(src, SR, r)
    assert len(items) == 4096 and res["starts"] == res["ends"] == 4095
    outs = syn.clip_loop_batch([r] * 16)
    assert len(outs) == 16 and all(same(o, res) for o in outs), [o for o in outs if not same(o, res)][:2]
    assert syn.loop_items(0) == items and syn.loop_items(15) == items
    with pytest.raises(ZlHipError, match=r"\(-5\)"):               # 16 x 4095 x 4095 pairs: no cost matrix
        syn.loop_costs(0)
    syn.unregister_clip(cid)


def test_the_strip_limit_is_accepted(syn):
    """2048 requests with both points kept at W = 1024: 2048 x 2 x 1024 = 4194304 strip frames, the call's limit and the largest
    xs_base / xe_base; one request more is refused with nothing written"""
    from libzl_amd import _abi
    src = lr.tone(133.7, 2, 4000, seed=22)
    cid = upload(syn, src)
    reqs = [dict(clip=cid, start_frame=512 + (7 * i) % 1400, stop_frame=512 + (7 * i) % 1400 + 1 + (13 * i) % 1500, start_search=-1, stop_search=-1, window=1024, min_length=1)
            for i in range(2048)]
    assert max(r["stop_frame"] for r in reqs) <= 4000 - 512
    wants = [want(src, SR, r) for r in reqs]
    outs = syn.clip_loop_batch(reqs)
    wrong = [(i, o, w[0]) for i, (o, w) in enumerate(zip(outs, wants)) if not same(o, w[0])]
    assert not wrong, (len(wrong), wrong[:2])
    assert all(o["pairs"] == 1 and o["nominal_valid"] == 1 and o["found"] == 1 for o in outs)
    for i in (0, 1, 2046, 2047):
        c = syn.loop_costs(i)
        assert syn.loop_items(i) == wants[i][1] and c.shape == (1, 1) and int(c[0, 0]) == int(wants[i][2][0, 0]) == outs[i]["cost"], i
    R = _abi.LoopRequest
    arr = (R * 2049)(*[R(r["clip"], r["start_frame"], r["stop_frame"], -1, -1, 1024, 1) for r in reqs + reqs[:1]])
    out = (_abi.Loop * 2049)()
    C.memset(out, 0x5A, C.sizeof(out))
    assert syn._lib.zlhip_sound_loop_batch(syn._e, arr, 2049, out) == _abi.ZLHIP_ERR_INVALID
    assert b"4194304" in syn._lib.zlhip_last_error(syn._e) and bytes(out) == b"\x5a" * C.sizeof(out)
    assert syn._lib.zlhip_sound_loop_batch(syn._e, arr, 2048, out) == 0 and out[2047].stop_frame == outs[2047]["stop_frame"] and bytes(out)[2048 * 80:] == b"\x5a" * 80
    syn.unregister_clip(cid)


# ---- the buffers and the resident kernel ------------------------------------------------------------------------------------------------
def test_an_engine_that_never_asks_allocates_nothing(built):
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=4, sound_arena_bytes=1 << 20) as s:
        cid = upload(s, lr.tone(120.0, 2, 24000, seed=2))
        total0, _ = s.memory_bytes()
        s.clip_loudness(cid)
        total1, _ = s.memory_bytes()
        s.clip_loop(cid, 6000, 18011)
        total2, _ = s.memory_bytes()
        assert total2 > total1 > total0
        s.clip_loop(cid, 6000, 18011); s.clip_loop(cid, 3, 23000, 100, 100, 64); s.clip_loop(cid, 5000, 5010, -1, -1); s.clip_loudness(cid)      # fit the first call's buffers
        assert s.memory_bytes()[0] == total2


@pytest.fixture()
def rt_env():
    old = os.environ.get("ZL_RT_PERSISTENT")
    os.environ["ZL_RT_PERSISTENT"] = "1"
    yield
    if old is None:
        os.environ.pop("ZL_RT_PERSISTENT", None)
    else:
        os.environ["ZL_RT_PERSISTENT"] = old


def test_the_resident_kernel_stays(built, rt_env):
    """After one warm-up call (it allocates the call's buffers, the cost matrix among them) loop calls between real-time cycles leave the
    resident kernel where it is: one launch of it for the whole scene, the cycles' audio bit-exact against the oracle, the results
    right."""
    sc = rtc.scene()
    tone = lr.tone(109.1, 2, 6000, seed=5)                         # one more clip, which no voice plays

    def request(cid, k, planar):
        n = planar[cid].shape[1]
        return dict(clip=cid, start_frame=n // 4 + k % 5, stop_frame=3 * n // 4 - k % 3, start_search=(20, 40, -1)[k % 3], stop_search=30, window=(16, 64, 256)[k % 3])

    def warm_up(syn, planar, rates):
        # more requests, strip frames, candidates and items than any call below, and a cost matrix: 21 x 129 x 129 pairs
        reqs = [dict(clip=i, start_frame=x.shape[1] // 4, stop_frame=3 * x.shape[1] // 4, start_search=64, stop_search=64, window=256) for i, x in enumerate(planar)]
        outs = syn.clip_loop_batch(reqs)
        assert len(reqs) == 21 and all(o["starts"] == o["ends"] == 129 for o in outs) and 0 < sum(o["starts"] * o["ends"] for o in outs) <= 1 << 20
        assert syn.loop_costs(20).shape == (129, 129)

    def between(syn, k, playing, planar, rates):
        # the loops of clips that play, a single call and a batch in turn
        reqs = [request(cid, k, planar) for cid in playing[:2]] + [request(len(planar) - 1, k, planar)]
        gots = [syn.clip_loop_batch([r])[0] for r in reqs] if k % 2 else syn.clip_loop_batch(reqs)
        return zip(reqs, gots)

    out, ref_bus, stats, todo, planar, rates = rtc.run(sc, [(tone, SR)], warm_up, between)
    assert stats[0] == 1 and stats[1:] == (1, sc.nblocks)
    expect = {}
    for r, got in todo:
        key = tuple(sorted(r.items()))
        if key not in expect:
            expect[key] = lr.loop(planar[r["clip"]], rates[r["clip"]], *(r.get(k, 0) for k in lr.KEYS))
        assert same(got, expect[key]), (r, got, expect[key])
    assert len(todo) >= 2 * sc.nblocks and sum(g["found"] for _, g in todo) >= 2 * sc.nblocks
    assert np.array_equal(out.view(np.int32), ref_bus.view(np.int32)), f"max diff {np.abs(out - ref_bus).max()}"
