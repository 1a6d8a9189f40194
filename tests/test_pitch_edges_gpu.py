"""Pitch detection, GPU tier, the edges: tests/pitch_cases.py through the kernels of libzl_amd/csrc/zl_pitch.hip.  The pick and vote
kernels (a block scan, two min-reductions, an LDS histogram, a max-reduction over a biased key) exist only there and are reached only
through clips, so the list's clips put every decision on its edge: the threshold at equality, a plateau under the descent, a descent
that ends at t_max, t0 and the stop in neighbouring lanes and waves, a valley at t_min - 1 and at t_max + 1, the gate at equality,
every shift at both sides of its limit, the lower median at an even count and at a lane's and a wave's edge of the histogram scan, the
edge of the consistent band, clarity ties within and across waves, 256 frames, and the geometries the grid leaves out
(tests/test_pitch_cpu.py asserts from the restatement alone that every case hits its edge).  Everything is compared as
tests/test_pitch_gpu.py compares it (its _check_batch): every d word, every frame record and every result integer bit for bit with
the numpy / Python-integer restatement (tests/pitch_ref.py), hz and confidence with ==, note and cents within 1e-9 -- and the named
outcomes (lag, flags, frame, consistent, shift) are asserted literally besides, so that a wrong restatement cannot carry a wrong
kernel.  The largest clip has 153512 frames."""
import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr
from test_pitch_gpu import _check_batch, _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=128, sound_arena_bytes=16 << 20)
    yield s
    s.close()


@pytest.fixture(scope="module")
def bank(syn):
    """pc.cases() and pc.too_short() uploaded once; the restatements are computed once and shared by the tests (cache)"""
    cases, short = pc.cases(), pc.too_short()
    srcs, reqs = {}, []
    for c in cases + short:
        cid = _upload(syn, c["x"], c["rate"])
        srcs[cid] = c["x"]
        reqs.append(dict(c["req"], clip=cid))
    yield dict(cases=cases, reqs=reqs[:len(cases)], empties=reqs[len(cases):], srcs=srcs, cache={})
    for cid in srcs:
        syn.unregister_clip(cid)


def _nothing(syn, i, out):
    return out["frames"] == 0 and all(out[k] == 0 for k in out) and syn.pitch_frames(i) == []


def test_every_edge_case_as_its_own_call(syn, bank):
    for c, r in zip(bank["cases"], bank["reqs"]):
        bad, outs = _check_batch(syn, [r], bank["srcs"], cache=bank["cache"])
        assert not bad, (c["name"], bad)
        pc.literal(c, outs[0], syn.pitch_frames(0))
    for r in bank["empties"]:
        bad, outs = _check_batch(syn, [r], bank["srcs"], cache=bank["cache"])
        assert not bad and _nothing(syn, 0, outs[0]), (r, bad, outs)


def test_the_edge_cases_in_one_call(syn, bank):
    """all of them in ONE clip_pitch_batch: 587 analysis frames in 82 requests"""
    bad, outs = _check_batch(syn, bank["reqs"], bank["srcs"], cache=bank["cache"])
    assert not bad, (len(bad), [b[1] for b in bad[:3]], bad[:1])
    assert sum(o["frames"] for o in outs) == sum(pc.geometry(c)[4] for c in bank["cases"]) == 587
    for i, c in enumerate(bank["cases"]):
        pc.literal(c, outs[i], syn.pitch_frames(i))


def test_the_edge_cases_between_requests_without_frames(syn, bank):
    """one call with a request too short for a frame first, last and twice in a row in the middle (zl_pt_find's bisection at its edges:
    a request without frames shares its bases with the next one)"""
    reqs, (e0, e1) = bank["reqs"], bank["empties"]
    half = len(reqs) // 2
    call = [e0] + reqs[:half] + [e1, e0] + reqs[half:] + [e1]
    where = [None] + list(range(half)) + [None, None] + list(range(half, len(reqs))) + [None]
    bad, outs = _check_batch(syn, call, bank["srcs"], cache=bank["cache"])
    assert not bad, (len(bad), [b[1] for b in bad[:3]], bad[:1])
    for i, k in enumerate(where):
        if k is None:
            assert _nothing(syn, i, outs[i]), (i, outs[i])
        else:
            pc.literal(bank["cases"][k], outs[i], syn.pitch_frames(i))
    assert [i for i, o in enumerate(outs) if o["frames"] == 0] == [i for i, k in enumerate(where) if k is None]


def test_a_fresh_engines_first_call_has_no_frames(built):
    """the first call of an engine allocates the call's buffers: with requests that have no frame at all, then one that has"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=1 << 20) as s:
        short = pc.too_short()
        ids = [_upload(s, c["x"], c["rate"]) for c in short]
        srcs = {cid: c["x"] for cid, c in zip(ids, short)}
        call = [dict(short[k]["req"], clip=ids[k]) for k in (0, 1, 0)]
        bad, outs = _check_batch(s, call, srcs)
        assert not bad and all(_nothing(s, i, o) for i, o in enumerate(outs)), (bad, outs)
        c = pc.cases()[0]
        cid = _upload(s, c["x"], c["rate"])
        bad, outs = _check_batch(s, [call[0], dict(c["req"], clip=cid), call[1]], {**srcs, cid: c["x"]})
        assert not bad and _nothing(s, 0, outs[0]) and _nothing(s, 2, outs[2]), (bad, outs)
        pc.literal(c, outs[1], s.pitch_frames(1))
        assert outs[1]["lag"] == 64 and np.float32(outs[1]["hz"]) == np.float32(750.0) and [f["flag"] for f in s.pitch_frames(1)] == [pr.VOICED]
