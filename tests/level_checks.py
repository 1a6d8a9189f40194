"""What the GPU tests of the level scans share (no GPU, no HIP): the integer block peak as the oracle defines it, and the check of the
last call's block peaks and RMS extension against the bus they belong to."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def peak_int(rows):
    """(int)fabsf(131072.f * x) with the oracle's definition of the open cases: NaN -> 0, 2^31 and above -> INT_MAX"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.abs(np.float32(131072.0) * rows.astype(np.float32))
    out = np.zeros(v.shape, dtype=np.int64)
    big, ok = v >= np.float32(2.0 ** 31), np.isfinite(v) & (v < np.float32(2.0 ** 31))
    out[big] = INT_MAX
    out[ok] = v[ok].astype(np.int64)
    return out


def check_levels(syn, bus, nframes, off=1):
    """the level scan of the LAST call (what block_peaks / levels_tick see) against the bus it belongs to: the integer peaks of every block,
    rms_a / rms_b of the first, a middle and the last block.  off: the tile offset of the RMS extension -- 1 where frame 0 of a block is
    the front frame (the reference's delayed store), 0 in the modes with ZLHIP_MODE_FIX_DELAY"""
    from oracle import zl_oracle as zo
    lib = zo.load()
    K, N = syn._last
    assert N == nframes
    B = bus.shape[0]
    tail = bus[:, :, bus.shape[2] - K * N:]
    exp = np.stack([peak_int(tail[:, c].reshape(B, K, N)).max(axis=2) for c in (0, 1)], axis=-1)      # [B][K][2]
    assert np.array_equal(syn.block_peaks(), exp.transpose(1, 0, 2))
    for k in sorted({0, K // 3, K - 1}):
        lv = syn.levels_tick(block_index=k)
        for b in range(B):
            for c, got in ((0, lv[b].rms_a), (1, lv[b].rms_b)):
                row = np.ascontiguousarray(tail[b, c, k * N:(k + 1) * N])
                want = lib.zlo_block_rms(row.ctypes.data, N, off)
                assert got == want or (np.isnan(got) and np.isnan(want)), (k, b, c, got, want)
