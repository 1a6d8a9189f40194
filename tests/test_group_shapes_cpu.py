"""The span scenes of tests/group_cases.py on the oracle alone: every scene that tests/test_group_shapes_gpu.py runs through a group can
fail.  The spanning-bus sum (zl_k_group_reduce_scan) is restated as the fp32 sum, in rank order from a zero array, of the members'
partials -- the oracle with mix_group = 0 on the events of one slice each -- and that sum is the oracle's grouped mix bit for bit;
the same partials in another order are not; every member adds something; the rows move; and the tile tails and the members'
shares of the (block, bus) pairs are what each case is listed for."""
import numpy as np
import pytest

from group_cases import ROOT_OUT_CALLS, ROOT_OUT_CASE, SPAN_CASES, TILE, bits, case_id, oracle_runs, rank_sum, shares
from libzl_amd import MODE_FIX_DELAY

CASES = SPAN_CASES + [ROOT_OUT_CASE]
cases = pytest.mark.parametrize("case", CASES, ids=case_id)


def rows(bus, N):
    """[B][2][K * N] -> [B][2][K][N]"""
    return bus.reshape(bus.shape[0], 2, -1, N)


@cases
def test_rank_order_sum_of_the_partials_is_the_grouped_mix(case):
    ref, _, _, parts = oracle_runs(case)
    assert ref.shape == (case.B, 2, case.K * case.N)
    assert np.array_equal(bits(rank_sum(parts, range(case.n))), bits(ref))


@cases
def test_another_order_is_not(case):
    """fp32 addition commutes: two members cannot tell their order, three can"""
    ref, _, _, parts = oracle_runs(case)
    if case.n < 3:
        assert case.n == 2 and np.array_equal(bits(rank_sum(parts, [1, 0])), bits(ref))
        return
    n = case.n
    for order in (list(range(n))[::-1], [0, 2, 1] + list(range(3, n))):
        other = rank_sum(parts, order)
        for b in range(case.B):
            assert (bits(other[b]) != bits(ref[b])).any(), (order, b)


@cases
def test_every_member_adds_to_every_bus(case):
    _, _, _, parts = oracle_runs(case)
    for r, p in enumerate(parts):
        played = np.abs(rows(p, case.N)).max(axis=(1, 3)) > 0        # [B][K]
        assert played.any(axis=1).all(), (r, played)
        if case.idle is not None and r == case.idle[0]:              # silent from `stop` to `again`, not before
            _, stop, again = case.idle
            assert not played[:, stop:again].any() and played[:, :stop].all() and played[:, again:].all()
    if case.idle is not None:                                        # calls in which the member has nothing to add
        _, stop, again = case.idle
        assert any(stop <= k0 and k0 + K <= again for k0, K in case.calls())


@cases
def test_rows_move(case):
    """a scene whose voices hold one sample per block sums to the same bits in any order: in every row that plays at least half of
    the frames differ from the frame before"""
    ref, _, _, _ = oracle_runs(case)
    r = rows(ref, case.N)
    plays = np.abs(r).max(axis=3) > 0
    moved = (bits(r)[..., 1:] != bits(r)[..., :-1]).sum(axis=3)
    assert plays.any(axis=(1, 2)).all()
    assert (moved[plays] * 2 >= case.N).all(), np.argwhere(plays & (moved * 2 < case.N))[:4].tolist()


@cases
def test_tails_and_shares_are_what_the_case_is_listed_for(case):
    off = 0 if case.mode & MODE_FIX_DELAY else 1
    assert case.tail == (case.N - off) % TILE
    want = {33: (32, 33), 64: (63, 0), 65: (0, 1), 100: (35, 36), 441: (56, 57), 128: (63, 0)}[case.N]    # N: (off = 1, off = 0)
    assert case.tail == want[1 - off]
    assert case.N % TILE == {33: 33, 64: 0, 65: 1, 100: 36, 441: 57, 128: 0}[case.N]
    calls = case.calls()
    assert sum(K for _, K in calls) == case.K
    per_call = [shares(K * case.B, case.n) for _, K in calls]
    for (_, K), sh in zip(calls, per_call):
        assert sum(sh) == K * case.B and len(sh) == case.n
    assert any((K * case.B) % case.n != 0 and len(set(sh)) > 1 for (_, K), sh in zip(calls, per_call)) == case.uneven
    assert any(0 in sh for sh in per_call) == case.empty
    if case is ROOT_OUT_CASE:
        assert tuple(K for _, K in calls) == ROOT_OUT_CALLS
    if case.name.startswith("N"):                                    # the block-size cases: one call, shares 3, 3 and 4
        assert per_call == [[3, 3, 4]]
    if case.name == "n8-K1-then-K3":
        assert [K for _, K in calls] == [1, 3] and per_call[0].count(0) == 6
    if case.vl == 32:                                                # one-block calls only
        assert all(K == 1 for _, K in calls)
