"""Engine group (zlhip_group_*, libzl_amd/csrc/zl_group.h), CPU tier: the partition arithmetic against libzl_amd/sharding.py, the
command routing of a spanning bus against one control plane with the whole config, the argument checks of zlhip_group_create before
any HIP call, the ctypes mirror of zlhip_group_config and the compiler's resources of the spanning-bus sum kernel."""
import ctypes as C
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

from libzl_amd import _abi, build, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def glib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_group_harness())
        ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
        l.zlgrp_plan.restype = C.c_int
        l.zlgrp_plan.argtypes = [C.c_int] * 6 + [ip]
        l.zlgrp_route_compare.restype = C.c_int
        l.zlgrp_route_compare.argtypes = [C.c_int] * 6 + [ip, ip, C.POINTER(_abi.ClipCommand), ip, ip, ip, ip, C.POINTER(C.c_int64)]
        _lib = l
    return _lib


def plan(n, B, VPB, vpt=0, partition=_abi.GROUP_AUTO, root=0):
    out = np.zeros(40, np.int32)
    rc = glib().zlgrp_plan(n, B, VPB, vpt, partition, root, out)
    return rc, out.reshape(5, 8)[:, :n]


@pytest.mark.parametrize("B,n", [(12, 1), (12, 2), (12, 3), (12, 5), (12, 8), (8, 8), (9, 4), (13, 7), (100, 8)])
def test_bus_aligned_ranges_are_sharding_bus_owner(B, n):
    rc, L = plan(n, B, 8, partition=_abi.GROUP_BUS_ALIGNED)
    assert rc == _abi.ZLHIP_OK
    for r in range(n):
        want = [g for g in range(B) if sharding.bus_owner(g, B, n) == r]
        assert list(range(L[1][r], L[1][r] + L[2][r])) == want
        assert sharding.BusPartition(B, n, r).buses == want
        assert (L[0][r], L[3][r], L[4][r]) == (_abi.GROUP_BUS_ALIGNED, 0, 8)


@pytest.mark.parametrize("VPB,n", [(8, 1), (8, 2), (8, 4), (8, 8), (128, 2), (128, 8), (12, 3), (24, 6)])
def test_span_slot_ranges_are_sharding_slots_for_rank(VPB, n):
    rc, L = plan(n, 3, VPB, partition=_abi.GROUP_SPAN)
    assert rc == _abi.ZLHIP_OK
    for r in range(n):
        a, b = sharding.slots_for_rank(VPB, n, r)
        assert (L[3][r], L[3][r] + L[4][r]) == (a, b)
        assert (L[0][r], L[1][r], L[2][r]) == (_abi.GROUP_SPAN, 0, 3)


def test_auto_partition():
    assert plan(4, 12, 8)[1][0][0] == _abi.GROUP_BUS_ALIGNED
    assert plan(4, 4, 8)[1][0][0] == _abi.GROUP_BUS_ALIGNED
    assert plan(4, 2, 8)[1][0][0] == _abi.GROUP_SPAN


def _random_steps(rng, B, VPB, nsounds, count):
    kinds, args, cmds = [], [], []
    for _ in range(count):
        c = _abi.ClipCommand()
        c.clip, c.midi_note, c.midi_channel, c.slice = -1, -1, -1, -1
        bus = int(rng.integers(0, B))
        u = rng.random()
        kind = 0 if u < 0.72 else 1 if u < 0.8 else 2 if u < 0.9 else 3 if u < 0.95 else 4
        c.clip = int(rng.integers(0, nsounds)) if rng.random() > 0.03 else int(rng.choice([-1, nsounds]))
        c.midi_channel = bus - 2 if rng.random() > 0.03 else B - 1      # (an occasional channel without a bus)
        c.midi_note = int(rng.choice([60, 62]))
        if rng.random() < 0.3:
            c.change_slice, c.slice = 1, int(rng.integers(0, 2))
        t = rng.random()
        if t < 0.45:
            c.start_playback = 1
        elif t < 0.65:
            c.stop_playback = 1
        elif t < 0.85:
            c.start_playback, c.stop_playback = 1, 1
        else:                                                       # a merge into playing voices
            c.change_volume, c.volume = 1, float(rng.random())
            c.change_looping, c.looping = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            c.change_gain_db, c.gain_db = int(rng.integers(0, 2)), -3.0
        c.looping = 1 if c.start_playback and rng.random() < 0.7 else c.looping
        c.volume = c.volume if c.change_volume else 0.8
        kinds.append(kind)
        args.append([bus, int(rng.integers(0, VPB)), int(rng.integers(0, 2))] if kind != 2 else [int(rng.integers(0, B * VPB)), 0, 0])
        cmds.append(c)
    return (np.asarray(kinds, np.int32), np.ascontiguousarray(np.asarray(args, np.int32).reshape(-1)), (_abi.ClipCommand * count)(*cmds))


@pytest.mark.parametrize("partition,n,B,VPB", [(_abi.GROUP_SPAN, 1, 2, 8), (_abi.GROUP_SPAN, 2, 2, 8), (_abi.GROUP_SPAN, 4, 2, 8),
                                               (_abi.GROUP_SPAN, 8, 2, 8), (_abi.GROUP_SPAN, 4, 3, 16), (_abi.GROUP_SPAN, 8, 1, 64),
                                               (_abi.GROUP_BUS_ALIGNED, 2, 12, 8), (_abi.GROUP_BUS_ALIGNED, 3, 12, 8),
                                               (_abi.GROUP_BUS_ALIGNED, 8, 12, 4)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_routing_equals_one_control_plane(partition, n, B, VPB, seed):
    """Seeded sequences of start / stop / stop + start / merge commands, explicit-slot starts, stops and updates, and voices ending on
    the device, on buses that fill up and empty again: what the group's routing queues on its members -- mapped to global voices --
    and what it returns equal one ZlHostControl with the whole config."""
    rng = np.random.default_rng(seed * 100 + n)
    nsounds, count = 5, 1500
    kinds, args, cmds = _random_steps(rng, B, VPB, nsounds, count)
    ro, rv, go, gv = (np.zeros(count, np.int32) for _ in range(4))
    ops = C.c_int64(0)
    bad = glib().zlgrp_route_compare(n, partition, B, VPB, nsounds, count, kinds, args, cmds, ro, rv, go, gv, C.byref(ops))
    assert bad == 0
    assert ops.value > count // 5
    np.testing.assert_array_equal(ro, go)
    np.testing.assert_array_equal(rv, gv)
    # the sequences reach both ends: starts that a full bus drops, and starts that are taken
    starts = np.array([bool(kinds[i] == 0 and cmds[i].start_playback and 0 <= cmds[i].clip < nsounds and cmds[i].midi_channel + 2 < B)
                       for i in range(count)])
    assert (ro[starts] == 0).any() and (ro[starts] == 1).any()
    assert (rv >= 0).sum() > 10


# ---- zlhip_group_create: argument checks before any HIP call --------------------------------------------------------------
@pytest.fixture(scope="module")
def elib(built):
    return _abi.bind(C.CDLL(build.build_engine()))


def _create(lib, devices, B=12, VPB=8, vpt=0, partition=_abi.GROUP_AUTO, root=0, struct_size=None):
    cfg = _abi.Config()
    lib.zlhip_config_default(C.byref(cfg))
    cfg.num_buses, cfg.voices_per_bus, cfg.voices_per_task = B, VPB, vpt
    gc = _abi.GroupConfig()
    lib.zlhip_group_config_default(C.byref(gc))
    gc.partition, gc.root = partition, root
    if struct_size is not None:
        gc.struct_size = struct_size
    devs = (C.c_int32 * max(1, len(devices)))(*devices)
    g = C.c_void_p(12345)
    rc = lib.zlhip_group_create(devs, len(devices), C.byref(cfg), C.byref(gc), C.byref(g))
    return rc, g


@pytest.mark.parametrize("kw", [
    dict(devices=[]),
    dict(devices=[0] * 9),
    dict(devices=[0, 0, 0], B=2, partition=_abi.GROUP_SPAN),                 # VPB 8 % 3
    dict(devices=[0, 0], B=2, vpt=2, partition=_abi.GROUP_SPAN),             # a foreign voices_per_task
    dict(devices=[0, 0], B=2, vpt=8, partition=_abi.GROUP_SPAN),
    dict(devices=[0, 0, 0], B=2, partition=_abi.GROUP_BUS_ALIGNED),          # fewer buses than members
    dict(devices=[0, 0], root=2),
    dict(devices=[0, 0], root=-1),
    dict(devices=[0, 0], B=1, root=5),                                        # (auto -> span: the root still has to be a member)
    dict(devices=[0, 0], partition=7),
    dict(devices=[0, -1]),
    dict(devices=[0, 0], struct_size=4),
])
def test_create_rejects_bad_configurations_before_hip(elib, kw):
    rc, g = _create(elib, **kw)
    assert rc == _abi.ZLHIP_ERR_INVALID and not g.value
    assert elib.zlhip_group_last_error(None)


def test_create_without_a_device_fails_loudly(elib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for kw in (dict(devices=[0, 0]), dict(devices=[0, 0, 0, 0], B=2, partition=_abi.GROUP_SPAN), dict(devices=[0])):
        rc, g = _create(elib, **kw)
        assert rc == _abi.ZLHIP_ERR_NO_DEVICE and not g.value
        assert b"no usable HIP device" in elib.zlhip_group_last_error(None)
    from libzl_amd import SamplerSynthGroup, ZlHipError
    with pytest.raises(ZlHipError):
        SamplerSynthGroup([0, 0], 2, 8, partition="span")


def test_group_config_struct_size_matches_the_c_layout():
    src = textwrap.dedent("""
        #include <stdio.h>
        #include "zlhip.h"
        int main(void) { printf("%zu %d\\n", sizeof(zlhip_group_config), ZLHIP_GROUP_MAX_MEMBERS); return 0; }""")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        size, mx = (int(x) for x in subprocess.check_output([os.path.join(d, "p")]).split())
    assert C.sizeof(_abi.GroupConfig) == size
    assert mx == _abi.GROUP_MAX_MEMBERS


def test_group_config_default(elib):
    gc = _abi.GroupConfig()
    elib.zlhip_group_config_default(C.byref(gc))
    assert (gc.struct_size, gc.partition, gc.root, gc.reserved) == (C.sizeof(_abi.GroupConfig), _abi.GROUP_AUTO, 0, 0)


def test_group_reduce_kernel_keeps_no_scratch(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_kernel_resources.txt")
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    grp = {n: r for n, r in rows.items() if "zl_k_group_reduce_scan" in n}
    assert len(grp) == 8                                           # one per member count 1 .. 8
    for n, r in grp.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (n, r)
