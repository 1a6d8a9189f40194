"""The gate of K2's two-frames-per-lane kernels (libzl_amd/csrc/zl_pair.h), CPU tier: which launches take zl_k2_pair_render /
zl_k2_pair_phase_render, built for the host (tests/cpu_harness/pair_host.cpp).  Every condition of the gate is moved one at a time away from a
launch that qualifies, under each value of the switch ZL_K2_PAIR (0 never, 1 auto, 2 wherever the shape allows) and in modes 0 / 1 / 2.
tests/test_k2_pair.py holds the kernels' parity with the oracle on the GPU."""
import ctypes as C

import pytest

from libzl_amd import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_pair_harness())
        l.zlpg_shape.restype = C.c_int
        l.zlpg_shape.argtypes = [C.c_uint] + [C.c_int] * 9
        l.zlpg_window.restype = C.c_int
        l.zlpg_window.argtypes = [C.c_int, C.c_int, C.c_uint] + [C.c_int] * 9
        _lib = l
    return _lib


# a launch that qualifies: the headline's (mode 0, 256 frames, a window of many blocks, one bus per workgroup, nothing fused)
OK = dict(mode=0, N=256, K=8192, NB=1, groups=1, staged=0, trace=0, fan=0, host_out=0, ongrid=1)
ORDER = ("mode", "N", "K", "NB", "groups", "staged", "trace", "fan", "host_out", "ongrid")

# one condition at a time: (field, value that must close the gate)
BREAKS = [("mode", 1), ("mode", 2), ("mode", 3), ("mode", 4), ("mode", 6), ("mode", 8),
          ("N", 64), ("N", 100), ("N", 128), ("N", 255), ("N", 257), ("N", 512), ("N", 1024),
          ("K", 1), ("K", 0),
          ("NB", 2), ("NB", 12), ("groups", 2), ("groups", 8), ("staged", 1), ("trace", 1), ("fan", 1), ("host_out", 1), ("ongrid", 0)]


def shape(**kw):
    a = dict(OK); a.update(kw)
    return lib().zlpg_shape(*[a[k] for k in ORDER])


def window(sw, cheap, **kw):
    a = dict(OK); a.update(kw)
    return lib().zlpg_window(sw, cheap, *[a[k] for k in ORDER])


def test_the_shape_that_qualifies_and_every_condition_alone():
    assert shape() == 1
    assert shape(K=2) == 1 and shape(K=60000) == 1                 # any batch; ongrid is a flag: any non-zero value
    assert shape(ongrid=2) == 1
    for field, value in BREAKS:
        assert shape(**{field: value}) == 0, (field, value)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_truth_table_of_the_switch(mode):
    """switch x cheap x every condition, in modes 0 / 1 / 2: only mode 0 ever opens"""
    opens = mode == 0
    for sw in (0, 1, 2, 3, -1):
        for cheap in (0, 1):
            want = opens and (sw == 2 or (sw == 1 and cheap == 1))
            assert window(sw, cheap, mode=mode) == (1 if want else 0), (sw, cheap)
            for field, value in BREAKS:
                if field == "mode":
                    continue
                assert window(sw, cheap, mode=mode, **{field: value}) == 0, (sw, cheap, field, value)


def test_auto_needs_every_playing_voice_cheap_and_two_does_not():
    assert window(1, 1) == 1 and window(1, 0) == 0
    assert window(2, 0) == 1 and window(2, 1) == 1
    assert window(0, 1) == 0 and window(0, 0) == 0
