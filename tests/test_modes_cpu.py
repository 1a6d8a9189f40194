"""The case table of the mode tests (tests/mode_cases.py) held to the launch decision, CPU tier.  A GPU test cannot see which kernel ran;
zl_k2_launch (libzl_amd/csrc/zl_launch.h) is the pure function that decides it, and zlhip_render_batch and zl_launch_render launch what it
says (tests/test_k2_launch_cpu.py, whose helper this file drives).  For every row of the table the launch description of each of its render
calls is computed from the row's own frames per block, blocks per call, buses, bus width, mix groups, mode and switches: together the rows
reach every non-staged instantiation zl_launch_render can launch -- 8 modes x {zl_k2_render with 4, 2 and 1 blocks per workgroup,
zl_k2_phase_render} -- and each row reaches the kernel its name says, with the level scan fused into K2 or left to K3 as its name says."""
import pytest

import test_k2_launch_cpu as tl
from mode_cases import BATCH_CASES, LAST_CALL_MIN, MODES, PHASE_RENDER, RENDER, SHAPES, calls, case_id, mix_groups

# buses per workgroup of a row's calls of several blocks (zl_k2_narrow_buses): every bus of the narrow rows; 1 where the bus width is no
# multiple of 8, a block has two frame tiles or a bus has mix groups
NARROW_BUSES = {"bpw4": 3, "bpw2": 4, "bpw1_narrow": 3, "bpw1_single_bus": 1, "partial_wave": 3, "two_tiles": 1, "ragged": 1, "mix_groups": 1, "phase": 2}
TAIL_MIN = 24                                # tests/conftest.py: ZL_K2_TAIL_MIN_BLOCKS of the test tier


def launches(case):
    """the launch description of every render call of the case (a call of so few frames is one plan window: the engine's window is 2048 * 256
    frames at the least).  What the helper's BASE leaves as it is: an order table to read, the on-grid switch at its default, no fan-out,
    no direct bounce delivery.  The fan-out and bounce tests of the GPU tier run the same rows with `fan` or `host_out` set; in zl_k2_launch
    those two only gate the pair kernels, which no row here can get (mode 0 has ZL_K2_PAIR=0, the other modes have no pair kernel)."""
    kw, out = case.scene, []
    for _, K in calls(case):
        assert tl.windows(K, kw["nframes"], 2048 * 256) == [(0, K)]
        r = tl.launch(sw=dict(tail_min=TAIL_MIN), mode=case.mode, N=kw["nframes"], K=K, call_blocks=K, B=kw["num_buses"], VPB=kw["voices_per_bus"],
                      groups=mix_groups(kw, K), order_mode=int(case.env.get("ZL_K2_PHASE_ORDER", 1)), pair_mode=int(case.env.get("ZL_K2_PAIR", 1)),
                      cheap=1, loop=0.0)     # (cheap, loop: the playing voices' say in the switches' auto setting, which no row leaves on where it counts)
        r["K"] = K
        out.append(r)
    return out


def keys(ls):
    return {(r["kernel"], r["bpw"], r["staged"]) for r in ls}


def test_the_table_reaches_every_non_staged_kernel():
    got = set()
    for case in BATCH_CASES:
        got |= {k + (case.mode,) for k in keys(launches(case))}
    want = {(kernel, bpw, 0, mode) for mode in MODES for kernel, bpw in [(RENDER, 4), (RENDER, 2), (RENDER, 1), (PHASE_RENDER, 1)]}
    assert len(want) == 32 and got == want, (sorted(want - got), sorted(got - want))


def test_the_table_is_every_shape_in_every_mode():
    assert sorted((c.name, c.mode) for c in BATCH_CASES) == sorted((name, mode) for name in SHAPES for mode in MODES)
    assert len({c.scene["seed"] for c in BATCH_CASES}) == len(BATCH_CASES)
    for c in BATCH_CASES:
        assert "ZL_K2_STAGED" not in c.env and (c.env.get("ZL_K2_PAIR") == "0") == (c.mode == 0)
        assert 2 <= c.scene["num_buses"] <= 5 and 8 <= c.scene["nblocks"] <= 16
        assert c.scene["voices_per_bus"] <= 16 or (c.name.startswith("wide") and 32 <= c.scene["voices_per_bus"] <= 40)


@pytest.mark.parametrize("case", BATCH_CASES, ids=case_id)
def test_a_row_reaches_the_kernel_its_name_says(case):
    sh, ls = SHAPES[case.name], launches(case)
    one = [r for r in ls if r["K"] == 1]                           # (a one-block call of a batch: one block per workgroup, no order)
    many = [r for r in ls if r["K"] > 1]
    if case.run.get("batch") == 1:
        assert not many and one
        promised = one
    else:
        assert many
        promised = many
    assert keys(promised) == {(sh.kernel, sh.bpw, 0)}, keys(promised)
    # the LAST call is the one whose levels the GPU tier reads (block_peaks, levels_tick): it is a launch of the promised kernel, and long
    # enough for a first, a middle and a last block that differ
    last = ls[-1]
    assert last in promised and (last["kernel"], last["bpw"], last["staged"]) == (sh.kernel, sh.bpw, 0)
    if many:
        assert last["K"] >= LAST_CALL_MIN and len({0, last["K"] // 3, last["K"] - 1}) == 3
        assert sh.bpw == 1 or last["K"] % sh.bpw                   # a last workgroup that is not full
        assert last["NB"] == NARROW_BUSES[case.name] and last["order"] == (1 if sh.kernel == PHASE_RENDER else 0)
    assert keys(one) <= {(RENDER, 1, 0)}
    # the order only where the row asks for it, and every launch of a row scans the levels in K2, or none does
    assert all(r["order"] == (1 if sh.kernel == PHASE_RENDER and r["K"] > 1 else 0) for r in ls)
    assert all(r["scans_levels"] == (1 if sh.scans_levels else 0) for r in ls), [(r["K"], r["scans_levels"]) for r in ls]
    assert all(r["tail_from"] == 0 and r["threads"] == (256 if r["bpw"] > 1 else tl.lib().zllh_whole_waves(case.scene["nframes"])) for r in ls)
    N, groups = case.scene["nframes"], {mix_groups(case.scene, r["K"]) for r in ls}
    if case.name == "bpw1_narrow":
        assert all(r["NB"] == 3 and r["gz"] == 1 for r in many)
    if case.name == "bpw1_single_bus":
        assert all(r["NB"] == 1 and r["gz"] == 2 for r in ls) and case.scene["voices_per_bus"] % 8
    if case.name == "partial_wave":
        assert all(r["gx"] == 1 and r["threads"] == 128 for r in ls) and N % 64
    if case.name in ("two_tiles", "ragged"):
        assert all(r["gx"] == 2 for r in ls) and (N % 256 != 0) == (case.name == "ragged")
    if case.name == "mix_groups":
        assert groups == {2} and all(r["gz"] == 2 * case.scene["num_buses"] for r in ls)
    if case.name == "single_blocks":
        assert groups == {1} and all(r["threads"] == 128 and r["gy"] == 1 for r in ls)
    if case.name == "wide_single_blocks":
        assert groups == {case.scene["voices_per_bus"]} and all(r["gz"] == case.scene["num_buses"] * case.scene["voices_per_bus"] for r in ls)
    assert (groups == {1}) == (case.name not in ("mix_groups", "wide_single_blocks"))


def test_scans_levels_by_name():
    fused = {name for name, sh in SHAPES.items() if sh.scans_levels}
    assert {"bpw4", "bpw2", "bpw1_narrow", "bpw1_single_bus", "partial_wave", "phase"} <= fused
    assert not fused & {"two_tiles", "mix_groups", "ragged", "wide_single_blocks"}
