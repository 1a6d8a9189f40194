"""What the compiler made of K2's two-frames-per-lane kernels (zl_k2_pair_render, zl_k2_pair_phase_render), from
libzl_amd/lib/libzlhip_kernel_resources.txt (see tests/test_kernel_resources.py): both exist, keep everything in registers -- no private
segment at all, the phase-order twin included -- and reach the occupancy their launch counts on: zl_launch_render pads a 128-lane workgroup
to ZL_K2_PAIR_LDS bytes of LDS, 8 workgroups per CU = 4 waves per SIMD, which the registers and the static LDS must allow."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_kernel_resources.txt")

PAIR_LDS = 18432            # ZL_K2_PAIR_LDS (zl_kernels.hip)
PAIR_WAVES = 4              # ZL_K2_PAIR_WAVES


def _rows():
    rows = {}
    for line in open(PATH):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    return rows


def test_pair_kernels_exist_without_scratch_at_their_occupancy(built):
    rows = _rows()
    pair = {n: r for n, r in rows.items() if "zl_k2_pair_render" in n or "zl_k2_pair_phase_render" in n}
    assert sorted(pair) == ["_Z17zl_k2_pair_render7ZlBatch", "_Z23zl_k2_pair_phase_render7ZlBatch"], sorted(pair)
    for n, r in pair.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (n, r)
        assert r["waves"] >= PAIR_WAVES, (n, r)
        # 4 waves per SIMD of this kernel leave a planner wave (88 registers) its share of the 512
        assert PAIR_WAVES * ((r["vgprs"] + 7) // 8 * 8) + 88 <= 512, (n, r)
        # the static LDS fits the padded size: 8 workgroups and the planner's 12 KB in a CU's 160 KB, and no ninth workgroup
        assert r["lds"] <= PAIR_LDS and 8 * PAIR_LDS + 12 * 1024 <= 160 * 1024 < 9 * PAIR_LDS, (n, r)


def test_names_do_not_count_as_the_render_kernels(built):
    """tests/test_kernel_resources.py counts the kernels whose name holds zl_k2_render: the pair kernels are none of them"""
    assert not [n for n in _rows() if "zl_k2_pair" in n and "zl_k2_render" in n]
