"""Tempo estimate, GPU tier, exact ties: tests/tempo_cases.py through the kernels of libzl_amd/csrc/zl_tempo.hip.  zl_k_tempo_pick
reduces the coarse argmax per lane, then by wave shuffle, then over the waves in LDS, each step in the order of zl_tp_beats ("equal
goes to the smaller lag"); sound never makes two lags tie, so the list's clips make them tie exactly at a chosen step: every lag with
every other, neighbouring lanes of a wave, one lane of all four waves, one thread on successive passes, and two lags of a doubling's
triple (tests/test_tempo_cpu.py asserts from the restatement alone that every case ties where it says).  Everything is compared as
tests/test_tempo_gpu.py compares it (its _check_batch): W, A and the record bit for bit with the numpy / Python-integer restatement
(tests/tempo_ref.py), bpm and confidence with == -- and the coarse and the fine lag are asserted literally besides.  The largest clip
has 179200 frames."""
import pytest

import tempo_cases as tc
from test_tempo_gpu import _check_batch, _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def syn(built):
    from libzl_amd import SamplerSynth
    s = SamplerSynth(num_buses=2, voices_per_bus=4, max_sounds=32, sound_arena_bytes=16 << 20)
    yield s
    s.close()


@pytest.fixture(scope="module")
def bank(syn):
    cases, short = tc.cases(), tc.too_short()
    srcs, reqs = {}, []
    for c in cases + short:
        cid = _upload(syn, c["x"], c["rate"])
        srcs[cid] = c["x"]
        reqs.append((cid,) + c["req"])
    yield dict(cases=cases, reqs=reqs[:len(cases)], empties=reqs[len(cases):], srcs=srcs)
    for cid in srcs:
        syn.unregister_clip(cid)


def _nothing(syn, i, out):
    return all(out[k] == 0 for k in ("bpm", "confidence", "lag_coarse", "lag_fine", "doublings", "acf_lo", "acf_mid", "acf_hi")) and len(syn.tempo_acf(i)[2]) == 0


def test_every_tie_case_as_its_own_call(syn, bank):
    for c, r in zip(bank["cases"], bank["reqs"]):
        bad, outs = _check_batch(syn, [r], bank["srcs"])
        assert not bad, (c["name"], bad)
        tc.literal(c, outs[0])
        assert outs[0] == syn.clip_tempo(*r)
    for r in bank["empties"]:
        bad, outs = _check_batch(syn, [r], bank["srcs"])
        assert not bad and _nothing(syn, 0, outs[0]) and outs[0]["hops"] > 0 and outs[0]["acf_zero"] > 0, (r, bad, outs)


def test_the_tie_cases_in_one_call(syn, bank):
    bad, outs = _check_batch(syn, bank["reqs"], bank["srcs"])
    assert not bad, (len(bad), bad[:2])
    for c, o in zip(bank["cases"], outs):
        tc.literal(c, o)
    assert [(o["lag_coarse"], o["lag_fine"]) for o in outs] == [(75, 297), (75, 300), (128, 256), (256, 512), (150, 300)]


def test_the_tie_cases_between_requests_without_lags(syn, bank):
    """one call with a request too short for any lag first, last and twice in a row in the middle: it shares its A and item bases
    with the next one"""
    reqs, (e0, e1) = bank["reqs"], bank["empties"]
    half = len(reqs) // 2
    call = [e0] + reqs[:half] + [e1, e0] + reqs[half:] + [e1]
    where = [None] + list(range(half)) + [None, None] + list(range(half, len(reqs))) + [None]
    bad, outs = _check_batch(syn, call, bank["srcs"])
    assert not bad, (len(bad), bad[:2])
    for i, k in enumerate(where):
        if k is None:
            assert _nothing(syn, i, outs[i]), (i, outs[i])
        else:
            tc.literal(bank["cases"][k], outs[i])
    assert [i for i, o in enumerate(outs) if o["lag_fine"] == 0] == [i for i, k in enumerate(where) if k is None]


def test_a_fresh_engines_first_call_has_no_lags(built):
    """the first call of an engine allocates the call's buffers: with requests that have no lag to look at, then one that has"""
    from libzl_amd import SamplerSynth
    with SamplerSynth(num_buses=1, voices_per_bus=1, max_sounds=8, sound_arena_bytes=2 << 20) as s:
        short = tc.too_short()
        ids = [_upload(s, c["x"], c["rate"]) for c in short]
        srcs = {cid: c["x"] for cid, c in zip(ids, short)}
        call = [(ids[k],) + short[k]["req"] for k in (0, 1, 0)]
        bad, outs = _check_batch(s, call, srcs)
        assert not bad and all(_nothing(s, i, o) for i, o in enumerate(outs)), (bad, outs)
        assert [o["hops"] for o in outs] == [90, 1, 90]
        c = tc.cases()[2]
        cid = _upload(s, c["x"], c["rate"])
        bad, outs = _check_batch(s, [call[0], (cid,) + c["req"], call[1]], {**srcs, cid: c["x"]})
        assert not bad and _nothing(s, 0, outs[0]) and _nothing(s, 2, outs[2]), (bad, outs)
        tc.literal(c, outs[1])
        assert (outs[1]["lag_coarse"], outs[1]["lag_fine"], outs[1]["doublings"]) == (128, 256, 1)
