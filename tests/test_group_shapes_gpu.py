"""The span partition's spanning-bus sum (zl_k_group_reduce_scan, zlhip_group_render_batch) at every member count, root and block size,
bit for bit: the scenes of tests/group_cases.py -- tests/test_group_shapes_cpu.py shows on the oracle that each of them tells a wrong
summation order -- through a group on device 0, against the oracle with mix_group = VPB / n and one engine with voices_per_task =
VPB / n.  Member counts 3, 5, 6, 7 and 8; blocks that are no whole number of 64-frame tiles, with and without the front frame;
a root other than member 0, with the caller's buffer on it; calls in which members have no (block, bus) pair to sum; one-block calls of
members wide enough to split their buses by voice; a member that plays nothing for some calls; the voice-level calls; and the
bus-aligned partition with one bus per member and with uneven bus counts."""

import numpy as np
import pytest

from group_cases import (BLOCK_SIZE_CASES, ROOT_OUT_CALLS, ROOT_OUT_CASE, SPAN_CASES, assert_same_bus, case_id, check_against, group,
                         oracle_runs)
from libzl_amd import MODE_FIX_DELAY, SamplerSynthGroup
from scenario import compare_runs, engine_cmd, random_scene, run_backend, snapshot_clip, zo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SPAN_CASES, ids=case_id)
def test_span_equals_one_engine_and_oracle(case):
    """bus, reports, every block's levels and the block peaks: the group, one engine and the oracle agree"""
    check_against(case.scene(), case.factory(), batch=case.batch)


def assert_meters_of_oracle_bus(syn, rows, off, what):
    """the levels and peaks of the group's last call against the oracle's bus rows [B][2][K][N]: rms_a / rms_b of every block are
    zlo_block_rms of the row (the front frame with off = 1, then 64-frame tiles), the block peaks max |131072 x| as an integer"""
    lib = zo.load()
    B, _, K, N = rows.shape
    rows = np.ascontiguousarray(rows)
    for k in range(K):
        lv = syn.levels_tick(block_index=k)
        for b in range(B):
            for c, got in ((0, lv[b].rms_a), (1, lv[b].rms_b)):
                want = lib.zlo_block_rms(np.ascontiguousarray(rows[b, c, k]).ctypes.data, N, off)
                assert np.float32(got).tobytes() == np.float32(want).tobytes(), f"{what}: rms, block {k} bus {b} channel {c}: {got} vs {want}"
                assert want > 0
    want_peaks = np.abs(np.float32(131072.0) * rows).astype(np.int64).max(axis=3).transpose(2, 0, 1)
    assert np.array_equal(syn.block_peaks(), want_peaks), what


@pytest.mark.parametrize("case", BLOCK_SIZE_CASES, ids=case_id)
def test_block_sizes_meter_the_oracle_bus(case):
    """one call of 5 blocks, shares of 3, 3 and 4 pairs: the tail mask of the last tile and both forms of the front frame"""
    ref, orep, osyn, _ = oracle_runs(case)
    sc = case.scene()
    grp, rep, syn, _ = run_backend(sc, case.factory())
    compare_runs(ref, orep, osyn, grp, rep, sc.num_buses * sc.voices_per_bus)
    assert syn._last == (case.K, case.N)
    assert_meters_of_oracle_bus(syn, ref.reshape(case.B, 2, case.K, case.N), 0 if case.mode & MODE_FIX_DELAY else 1, case.name)
    syn.close()


def test_root_two_sums_into_the_callers_buffer():
    """n = 3, root = 2: three calls of 5, 2 and 5 blocks queued without a synchronisation, each into its own buffer on the root's
    device -- member 2's render writes its partial there and the sum replaces it in place; every float of every buffer is the
    oracle's, and the meters of the last call are member 2's"""
    import torch
    case = ROOT_OUT_CASE
    sc = case.scene()
    ref, _, _, _ = oracle_runs(case)
    B, N, V = case.B, case.N, case.B * case.n * case.vl
    syn = SamplerSynthGroup([0] * case.n, B, case.n * case.vl, partition="span", root=case.root, mode=case.mode, max_batch_blocks=max(ROOT_OUT_CALLS),
                            max_frames=N, max_sounds=16, sound_arena_bytes=1 << 22)
    assert [m["partition"] for m in syn.layout()] == ["span"] * case.n
    oref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=16)
    for i, (L, R, sr) in enumerate(sc.sounds):
        oref.register_clip(L, R, sr)
        assert syn.register_clip(L, R, sr) == i
        sc.clip_setup[i](oref.lib, oref.clips[i])
        syn.set_clip_params(i, snapshot_clip(oref.clips[i]))
    assert sorted(k for k in sc.events if sc.events[k]) == [0]
    for ev in sc.events[0]:
        syn.start_voice(ev[1], ev[2], engine_cmd(**ev[3]), ev[4])
    outs = [torch.full((B, 2, K * N), 3.0, device="cuda:0", dtype=torch.float32) for K in ROOT_OUT_CALLS]
    k0 = 0
    for K, out in zip(ROOT_OUT_CALLS, outs):
        syn.render_batch(K, N, sc.make_clocks(k0, K), bus_out_dev=out.data_ptr())
        k0 += K
    syn.synchronize()
    torch.cuda.synchronize()
    k0 = 0
    for c, (K, out) in enumerate(zip(ROOT_OUT_CALLS, outs)):
        assert_same_bus(np.ascontiguousarray(ref[:, :, k0 * N:(k0 + K) * N]), out.cpu().numpy(), f"call {c}")
        k0 += K
    K = ROOT_OUT_CALLS[-1]
    assert_meters_of_oracle_bus(syn, np.ascontiguousarray(ref[:, :, (k0 - K) * N:]).reshape(B, 2, K, N), 1, "root 2")
    rep = syn.voice_reports()
    assert sum(1 for v in range(V) if rep[v].playing) >= V // 2
    syn.close()


@pytest.mark.parametrize("n,B,hold,seed", [(8, 8, 5, 31), (5, 13, 7, 37)])
def test_bus_aligned_one_bus_each_and_uneven_counts(n, B, hold, seed):
    """eight members with one bus each, the hold bus on member 5; five members with 3, 3, 3, 2 and 2 buses or the like; blocks of 100
    frames"""
    sc = random_scene(seed, num_buses=B, voices_per_bus=8, nframes=100)
    check_against(sc, group([0] * n, "bus"), hold=hold)
    syn = SamplerSynthGroup([0] * n, B, 8, partition="bus", max_frames=64, max_batch_blocks=1, max_sounds=8, sound_arena_bytes=1 << 20)
    lay = syn.layout()
    syn.close()
    assert [m["partition"] for m in lay] == ["bus"] * n
    counts = [m["num_buses"] for m in lay]
    assert sum(counts) == B and [m["first_bus"] for m in lay] == [sum(counts[:r]) for r in range(n)]
    if n == B:
        assert counts == [1] * n and lay[5]["first_bus"] == hold
    else:
        assert len(set(counts)) > 1 and min(counts) >= 1
        owner = next(r for r, m in enumerate(lay) if m["first_bus"] <= hold < m["first_bus"] + m["num_buses"])
        assert owner > 0
