"""Runs of items that cross records, on the device ("The run"): zl_k_overview_reduce, zl_k_onset_energy (which the
tempo call launches too) and zl_k_pcm_decode stop growing their grid at 4096 workgroups; above that a wavefront takes a run of
consecutive items, finds the record of its first item by bisection and steps from record to record inside the run.  That logic lives
in the three .hip files only, so it is held here: the cases of tests/run_cases.py -- calls of 16384 to 131075 items whose runs walk
through one-item requests, change channel count, hop size, format and the overview's three forms halfway, and carry a non-finite
verdict past a piece boundary -- against the restatements, bit for bit.  tests/test_capped_runs_cpu.py asserts that every case
reaches its regime.

Two properties of the code would hide a skipped item, and the tests defeat both:
  * E is not cleared (a hop has one writer, there is no memset): the onset and tempo cases run on a fresh engine behind a poison call
    over a full-scale clip, so a hop that no wave takes holds a value no case produces;
  * decode writes into arena extents that are handed out again: clips of the same sizes and formats with other values are uploaded
    and released first, so a group that no lane writes holds a wrong float."""
import numpy as np
import pytest

import decode_ref as dr
import overview_ref as ov
import run_cases as rc
import tempo_ref as tr

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SR = 48000.0
TOTALS = list(rc.TOTALS)
IDS = [f"{t}_items" for t in TOTALS]


def _upload(s, x):
    return s.register_clip(x[0], x[1] if x.shape[0] == 2 else None, SR)


def _engine(**kw):
    from libzl_amd import SamplerSynth
    return SamplerSynth(num_buses=1, voices_per_bus=1, **kw)


# ---- onset ---------------------------------------------------------------------------------------------------------------------------
def check_onsets(s, c, ids):
    """one clip_onsets_batch call; E, N and the onsets of every request against the restatement -> (mismatches, everything read)"""
    outs = s.clip_onsets_batch(rc.onset_requests(c, ids))
    bad, got = [], []
    for i, (spec, out) in enumerate(zip(c["specs"], outs)):
        want, E, N = rc.onset_want(spec)
        gE, gN = s.onset_hops(i)
        got.append((gE, gN, out.copy()))
        if not (gE.dtype == np.uint64 and np.array_equal(gE, E)):
            bad.append((i, int(c["bases"][i]), spec, "E", [int(h) for h in np.flatnonzero(gE != E)[:4]] if gE.shape == E.shape else gE.shape))
        elif not (np.array_equal(gN, N) and np.array_equal(out, want)):
            bad.append((i, int(c["bases"][i]), spec, "N or the onsets"))
    return bad, got


def onset_case_on_a_fresh_engine(total, poison=True):
    c = rc.onset_case(total)
    assert rc.limits(c) == total
    with _engine(max_sounds=8, sound_arena_bytes=16 << 20) as s:
        ids = [_upload(s, x) for x in rc.onset_sources()]
        if poison:
            pid = _upload(s, rc.onset_poison())
            reqs = rc.onset_poison_requests(pid, total)
            s.clip_onsets_batch(reqs)
            E = s.onset_hops(len(reqs) - 1)[0]
            assert len(reqs) * rc.ON_CHUNK >= total and (E == rc.onset_poison_energy()).all()                # the buffer holds what no case produces
        bad, got = check_onsets(s, c, ids)
    return c, bad, got


@pytest.mark.parametrize("total", TOTALS, ids=IDS)
def test_onset_runs_cross_requests(built, total):
    c, bad, got = onset_case_on_a_fresh_engine(total)
    assert not bad, (len(bad), bad[:6])
    assert sum(len(o) for _, _, o in got) >= 8                     # onsets were found


# ---- tempo ---------------------------------------------------------------------------------------------------------------------------
_tempo_want = {}


def tempo_want(spec):
    if spec not in _tempo_want:
        clip, first, n, hop = spec
        _tempo_want[spec] = tr.tempo(rc.onset_sources()[clip], SR, first, n, hop, 0.0, 0.0)
    return _tempo_want[spec]


def test_tempo_shares_the_energy_launch(built):
    """the q = 2, rem = 1 list through clip_tempo_batch with the default range, behind a poison call of its own (the tempo call keeps
    its own E): the whole record, W and A of every request; a one-hop request answers "no tempo" between neighbours that have one"""
    total = 32769
    c = rc.onset_case(total)
    with _engine(max_sounds=8, sound_arena_bytes=16 << 20) as s:
        ids = [_upload(s, x) for x in rc.onset_sources()]
        pid = _upload(s, rc.onset_poison())
        s.clip_tempo_batch([r[:4] for r in rc.onset_poison_requests(pid, total)])
        outs = s.clip_tempo_batch([(ids[clip], first, n, hop) for clip, first, n, hop in c["specs"]])
        bad = []
        for i, (spec, got) in enumerate(zip(c["specs"], outs)):
            rec, W, first_lag, A = tempo_want(spec)
            gW, gfirst, gA = s.tempo_acf(i)
            okW = np.array_equal(gW, W)
            okA = [int(v) for v in gA] == A and (len(A) == 0 or gfirst == first_lag)
            ints = all(int(got[k]) == int(rec[k]) for k in rec if k not in ("bpm", "confidence"))
            if not (okW and okA and ints and f32(got["bpm"]) == rec["bpm"] and f32(got["confidence"]) == rec["confidence"]):
                bad.append((i, int(c["bases"][i]), spec, "W" if not okW else "A" if not okA else ("record", got, rec)))
    assert not bad, (len(bad), bad[:4])
    one = [i for i, n in enumerate(c["items"]) if n == 1]
    assert len(one) > 300 and all(outs[i]["lag_fine"] == 0 and outs[i]["bpm"] == 0.0 and outs[i]["hops"] == 1 for i in one)
    assert sum(1 for o in outs if o["lag_fine"] > 0) >= 8


# ---- overview ------------------------------------------------------------------------------------------------------------------------
def check_overviews(s, c, ids):
    """one clip_overviews call; every request's columns against the restatement and against its clip's own value range"""
    outs = s.clip_overviews(rc.overview_requests(c, ids))
    bad = []
    for i, (spec, out) in enumerate(zip(c["specs"], outs)):
        lo, hi = rc.OV_CLIPS[spec[0]][2]
        if not (out.min() >= f32(lo) and out.max() <= f32(hi)):
            bad.append((i, int(c["bases"][i]), spec, "a column outside the clip's range", float(out.min()), float(out.max())))
        elif not ov.same_bits(out, rc.overview_want(spec)):
            bad.append((i, int(c["bases"][i]), spec, "bits"))
    return bad, np.concatenate(outs)


@pytest.mark.parametrize("total", TOTALS, ids=IDS)
def test_overview_runs_cross_requests_and_forms(built, total):
    c = rc.overview_case(total)
    assert rc.limits(c) <= 262144
    with _engine(max_sounds=8, sound_arena_bytes=16 << 20) as s:
        ids = [_upload(s, x) for x in rc.overview_sources()]
        bad, _ = check_overviews(s, c, ids)
    assert not bad, (len(bad), bad[:6])


# ---- decode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("total", TOTALS, ids=IDS)
def test_decode_runs_cross_pieces(built, monkeypatch, total, placement):
    monkeypatch.delenv("ZL_PCM_STAGE_BYTES", raising=False)        # the default stage ...
    c = rc.decode_case(total)
    assert rc.limits(c) <= rc.header_value("decode", "STAGE_DEFAULT") == 64 << 20      # ... holds the call: one pass, one decode launch
    want = [rc.decode_want(spec, placement) for spec in c["specs"]]
    n = len(want)
    arena = 4 * sum(w[0].size for w in want) + (1 << 20)
    with _engine(max_sounds=n, sound_arena_bytes=arena, sound_arena_max_bytes=arena) as s:           # one segment that cannot grow
        before = s.register_clips_pcm(rc.decode_sources(c, placement, seed=1))
        assert before == list(range(n)) and all(s.clip_info(i)["finite"] for i in c["quartet"])
        for cid in before:
            s.unregister_clip(cid)
        mem = s.memory_bytes()
        ids = s.register_clips_pcm(rc.decode_sources(c, placement))                                # the one call: the extents hold wrong floats
        assert ids == list(range(n)) and s.memory_bytes() == mem
        bad, flags = [], []
        for cid, spec, (ext, _) in zip(ids, c["specs"], want):
            got = s.clip_extent(cid).view(u32)                     # the pad behind the clip included
            if not dr.same(got, ext, spec[0]):
                bad.append((cid, int(c["bases"][cid]), spec, [int(v) for v in np.flatnonzero(got != ext)[:4]] if got.shape == ext.shape else got.shape))
            flags.append(s.clip_info(cid)["finite"])
    assert not bad, (len(bad), bad[:6])
    assert flags == [w[1] for w in want]
    assert [i for i, ok in enumerate(flags) if not ok] == [c["quartet"][0], c["quartet"][3]]     # the two poisoned clips, nobody else


# ---- the per-call buffers are shared and only grow ---------------------------------------------------------------------------------
def test_overview_after_onset_in_one_engine(built):
    total = 32769
    on, ovc = rc.onset_case(total), rc.overview_case(total)
    with _engine(max_sounds=16, sound_arena_bytes=32 << 20) as s:
        on_ids = [_upload(s, x) for x in rc.onset_sources()]
        ov_ids = [_upload(s, x) for x in rc.overview_sources()]
        pid = _upload(s, rc.onset_poison())
        s.clip_onsets_batch(rc.onset_poison_requests(pid, total))
        bad1, first_on = check_onsets(s, on, on_ids)
        bad2, first_ov = check_overviews(s, ovc, ov_ids)
        assert not bad1 and not bad2, (bad1[:4], bad2[:4])
        # and each again in the other order
        bad3, again_ov = check_overviews(s, ovc, ov_ids)
        s.clip_onsets_batch(rc.onset_poison_requests(pid, total))
        bad4, again_on = check_onsets(s, on, on_ids)
        assert not bad3 and not bad4, (bad3[:4], bad4[:4])
    assert np.array_equal(first_ov.view(u32), again_ov.view(u32))
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(first_on, again_on) for k in range(3))
