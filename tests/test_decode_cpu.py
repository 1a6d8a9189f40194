"""Clips from raw PCM, CPU tier: the host build of libzl_amd/csrc/zl_decode.h (tests/cpu_harness/decode_host.cpp converts with the
header's own arithmetic and walks a call the way the kernel does) against the numpy restatement (tests/decode_ref.py), the
restatement against libzl_wav_read as a second witness, the new kernels' resources and what the C-ABI answers without a GPU.
tests/test_decode_gpu.py holds the kernel itself to the restatement on the GPU.  Everything is compared bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decode_ref as dr
from libzl_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32, f32 = np.uint32, np.float32

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build.build_decode_harness())
        l.zldec_convert.restype = None
        l.zldec_convert.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        l.zldec_stage_bytes.restype = C.c_uint32
        l.zldec_stage_bytes.argtypes = [C.c_int64]
        l.zldec_extent_floats.restype = C.c_uint64
        l.zldec_extent_floats.argtypes = [C.c_int64, C.c_int]
        l.zldec_run.restype = C.c_int64
        l.zldec_run.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib = l
    return _lib


def convert(raw, fmt):
    raw = np.ascontiguousarray(dr.raw_bytes(raw))
    n = raw.size // dr.BYTES[fmt]
    out = np.zeros(n, u32)
    lib().zldec_convert(fmt, raw.ctypes.data, n, out.ctypes.data)
    return out


def check(raw, fmt):
    got, ref = convert(raw, fmt), dr.samples(raw, fmt)
    assert dr.same(got, ref, fmt), (dr.NAMES[fmt], np.flatnonzero(got != ref.view(u32))[:8])
    return got.view(f32)


def s24(values):
    v = np.asarray(values, np.int64) & 0xFFFFFF
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=1).astype(np.uint8)


def test_every_u8_and_s16_value():
    got = check(np.arange(256, dtype=np.uint8), dr.U8)
    assert got[128] == 0.0 and got[0] == -1.0 and got[255] == f32(127.0 / 128.0)
    got = check(np.arange(-32768, 32768, dtype=np.int16), dr.S16)
    assert got[0] == -1.0 and got[32768] == 0.0 and got[-1] == f32(32767.0 / 32768.0)
    assert np.array_equal(got, np.arange(-32768, 32768, dtype=np.float64).astype(f32) / f32(32768.0))


def test_s24_edges_byte_order_and_random_values():
    got = check(s24([0, 1, -1, 0x7FFFFF, 0x800000]), dr.S24)
    assert list(got) == [0.0, f32(2.0 ** -23), f32(-2.0 ** -23), f32(1.0 - 2.0 ** -23), -1.0]
    # three distinct bytes, least significant first: 0x563412 -> 0x56341200
    got = check(np.array([0x12, 0x34, 0x56], np.uint8), dr.S24)
    assert got[0] == f32(0x56341200 / 2.0 ** 31) and got[0] != f32(0x12345600 / 2.0 ** 31)
    check(np.random.default_rng(24).integers(0, 256, 3 * 100000, dtype=np.uint8), dr.S24)


def test_s32_edges_ties_and_random_values():
    edges = np.array([-2 ** 31, 2 ** 31 - 1, 0, 1, -1, 0x01000001, 0x01000003, 0x01000002, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, -(2 ** 24 + 3),
                      2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31 - 63, -(2 ** 31) + 65], np.int64).astype(np.int32)
    got = check(edges, dr.S32)
    assert got[0] == -1.0 and got[1] == 1.0                        # INT_MAX rounds up to 2^31
    # ties go to the even mantissa: 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4
    assert got[4 + 1] == f32(0x01000000 / 2.0 ** 31) and got[4 + 2] == f32(0x01000004 / 2.0 ** 31)
    assert got[8] == f32(2.0 ** 24 / 2.0 ** 31) and got[9] == f32(-2.0 ** 24 / 2.0 ** 31) and got[10] == f32((2.0 ** 24 + 4) / 2.0 ** 31)
    check(np.random.default_rng(32).integers(-2 ** 31, 2 ** 31, 100000, dtype=np.int64).astype(np.int32), dr.S32)


F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA00000, 0xFFFFFFFF, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], u32)
F64_SPECIAL = np.concatenate([
    np.array([0.0, -0.0, 2.0 ** -140, -2.0 ** -140, 2.0 ** -149, 2.0 ** -150, -2.0 ** -150, 2.0 ** -150 * 1.5, 2.0 ** -126, 2.0 ** -127,
              1e300, -1e300, np.finfo(np.float64).max, -np.finfo(np.float64).max, float(np.finfo(f32).max), 2.0 ** 128, 2.0 ** 128 * (1 - 2.0 ** -25),
              1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 - 2.0 ** -25, np.inf, -np.inf, 1.0, -1.0, 0.1], np.float64),
    np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF4000000000000], np.uint64).view(np.float64)])


def test_f32_is_moved_as_bits():
    got = convert(F32_SPECIAL, dr.F32)
    assert np.array_equal(got, F32_SPECIAL)
    words = np.random.default_rng(5).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(u32)
    assert np.array_equal(convert(words, dr.F32), words)


def test_f64_rounds_to_nearest_even_keeps_denormals_and_overflows_to_inf():
    got = check(F64_SPECIAL, dr.F64)
    bits = got.view(u32)
    assert bits[2] == 1 << 9 and bits[3] == 0x80000000 | 1 << 9    # 2^-140: an fp32 denormal, not flushed
    assert bits[4] == 1 and bits[5] == 0 and bits[6] == 0x80000000 and bits[7] == 1     # 2^-150 is a tie to even: zero
    assert np.isposinf(got[10]) and np.isneginf(got[11]) and np.isposinf(got[12]) and np.isneginf(got[13])
    assert bits[14] == 0x7F7FFFFF and np.isposinf(got[15]) and np.isposinf(got[16])
    assert got[17] == 1.0 and got[18] == f32(1.0 + 2.0 ** -22) and got[19] == f32(1.0 + 2.0 ** -23)
    nan = bits[-4:]
    assert np.isnan(got[-4:]).all() and list(nan >> 31) == [0, 1, 0, 1]
    check(np.random.default_rng(64).uniform(-2.0, 2.0, 100000), dr.F64)
    check((np.random.default_rng(65).uniform(-1.0, 1.0, 100000) * 2.0 ** -130), dr.F64)     # around the denormal range


LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4099)
CHANNELS = (1, 2, 3, 5)


def run_call(clips, stage):
    """clips: [(raw bytes, fmt, channels, length)] -> (violations, passes, pieces, extents, writes, verdicts)"""
    n = len(clips)
    raws = [np.ascontiguousarray(dr.raw_bytes(c[0])) for c in clips]
    lengths = np.array([c[3] for c in clips], np.int32)
    chans = np.array([c[2] for c in clips], np.int32)
    fmts = np.array([c[1] for c in clips], np.int32)
    words = [int(lib().zldec_extent_floats(c[3], min(2, c[2]))) for c in clips]
    outs = [np.full(w, 0xDEADBEEF, u32) for w in words]
    writes = [np.zeros(w, np.int32) for w in words]
    verdicts = np.zeros(n, u32)
    srcp = (C.c_void_p * n)(*[r.ctypes.data for r in raws])
    outp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    wrp = (C.c_void_p * n)(*[w.ctypes.data for w in writes])
    npass, npiece = C.c_int32(0), C.c_int32(0)
    bad = lib().zldec_run(n, lengths.ctypes.data, chans.ctypes.data, fmts.ctypes.data, srcp, stage, outp, wrp, verdicts.ctypes.data,
                          C.byref(npass), C.byref(npiece))
    return bad, npass.value, npiece.value, outs, writes, verdicts


@pytest.mark.parametrize("stage", [4096, 64 << 20], ids=["stage4096", "stage64MiB"])
@pytest.mark.parametrize("fmt", dr.FORMATS, ids=[dr.NAMES[f] for f in dr.FORMATS])
def test_the_walk_writes_every_float_once_and_reads_no_foreign_byte(fmt, stage):
    rng = np.random.default_rng(100 * fmt + 1)
    clips = [(dr.random_raw(rng, fmt, ch, n), fmt, ch, n) for ch in CHANNELS for n in LENGTHS]
    bad, npass, npiece, outs, writes, verdicts = run_call(clips, stage)
    assert bad == 0                                                # no foreign stage byte read, every piece on its boundaries, no store outside
    if stage == 4096:
        assert npass > 1 and npiece > len(clips)                   # many passes, clips cut inside (4099 frames do not fit 4096 bytes)
    else:
        assert npass == 1 and npiece == len(clips)
    for (raw, _, ch, n), out, wr in zip(clips, outs, writes):
        assert (wr == 1).all(), (ch, n, np.flatnonzero(wr != 1)[:8])                   # pad included, exactly once
        ref = dr.extent(dr.decode(raw, fmt, ch))
        assert out.size == ref.size and dr.same(out, ref, fmt), (dr.NAMES[fmt], ch, n, np.flatnonzero(out != ref)[:8])
    assert not verdicts.any()


def test_mixed_formats_in_one_call_and_the_verdicts():
    rng = np.random.default_rng(7)
    clips = []
    for i, (fmt, ch, n) in enumerate([(dr.S16, 2, 1000), (dr.F32, 2, 777), (dr.S24, 1, 333), (dr.F64, 3, 100), (dr.U8, 5, 4099), (dr.F32, 3, 64), (dr.F64, 1, 9)]):
        clips.append([dr.random_raw(rng, fmt, ch, n), fmt, ch, n])
    # an inf in a kept channel of clip 1; an inf in the THIRD channel of clip 5 (not looked at); 1e300 in clip 6
    clips[1][0].view(f32)[2 * 500 + 1] = np.inf
    clips[5][0].view(f32)[3 * 10 + 2] = np.inf
    clips[6][0].view(np.float64)[4] = 1e300
    for stage in (4096, 64 << 20):
        bad, _, _, outs, writes, verdicts = run_call([tuple(c) for c in clips], stage)
        assert bad == 0 and list(verdicts) == [0, 1, 0, 0, 0, 0, 1]
        for (raw, fmt, ch, n), out, wr in zip(clips, outs, writes):
            planar = dr.decode(raw, fmt, ch)
            assert (wr == 1).all() and dr.same(out, dr.extent(planar), fmt)
        assert [dr.finite(dr.decode(c[0], c[1], c[2])) for c in clips] == [True, False, True, True, True, True, False]


def test_stage_size_is_clamped_and_rounded():
    l = lib()
    assert l.zldec_stage_bytes(0) == 4096 and l.zldec_stage_bytes(-5) == 4096 and l.zldec_stage_bytes(4097) == 4112
    assert l.zldec_stage_bytes(64 << 20) == 64 << 20 and l.zldec_stage_bytes(1 << 40) % 16 == 0
    assert l.zldec_piece_record_bytes() == 40


WAVS = [(dr.U8, 1), (dr.U8, 2), (dr.S16, 1), (dr.S16, 2), (dr.S16, 3), (dr.S24, 1), (dr.S24, 2), (dr.S24, 3), (dr.S32, 2), (dr.F32, 1), (dr.F32, 2),
        (dr.F32, 3), (dr.F64, 1), (dr.F64, 2), (dr.F64, 3)]


def wav_cases(tmp_path):
    """[(path, raw, fmt, channels, rate)]: every format, mono, stereo and 3 channels, one WAVE_FORMAT_EXTENSIBLE"""
    rng = np.random.default_rng(11)
    out = []
    for i, (fmt, ch) in enumerate(WAVS):
        n = 257 + 13 * i
        raw = dr.random_raw(rng, fmt, ch, n)
        path = str(tmp_path / f"{dr.NAMES[fmt]}_{ch}.wav")
        dr.write_wav(path, raw, fmt, ch, 44100 if i % 2 else 48000, extensible=(fmt, ch) == (dr.S24, 3))
        out.append((path, raw, fmt, ch, 44100 if i % 2 else 48000))
    return out


def test_libzl_wav_read_gives_the_restatements_bits(built, tmp_path):
    from libzl_amd import libzl
    zl = libzl.load()
    for path, raw, fmt, ch, rate in wav_cases(tmp_path):
        L, R = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        n, sr = C.c_int(0), C.c_double(0.0)
        assert zl.libzl_wav_read(path.encode(), C.byref(L), C.byref(R), C.byref(n), C.byref(sr)) == 0, path
        ref = dr.decode(raw, fmt, ch)
        assert n.value == ref.shape[1] and sr.value == rate and bool(R) == (ch >= 2)
        got = np.stack([np.ctypeslib.as_array(p, (n.value,)).copy() for p in ((L, R) if ch >= 2 else (L,))])
        zl.libzl_wav_free(L); zl.libzl_wav_free(R)
        assert dr.same(got, ref, fmt), path


def test_decode_kernels_have_no_scratch_memory_and_no_lds(built):
    path = os.path.join(ROOT, "libzl_amd", "lib", "libzlhip_zl_decode_kernel_resources.txt")
    assert os.path.exists(path), "build() writes the resources of zl_decode.hip's kernels"
    rows = {}
    for line in open(path):
        name, *kv = line.split()
        rows[name] = {k: int(v) for k, v in (x.split("=") for x in kv)}
    decode = [r for n, r in rows.items() if "zl_k_pcm_decode" in n]
    assert len(decode) == 1, rows
    for r in rows.values():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, rows
    assert decode[0]["waves"] >= 8, rows                           # the copy through the CUs hides latency with resident waves


def test_without_a_gpu_the_calls_answer_invalid(built):
    l = _abi.bind(C.CDLL(build.build_engine()))
    x = np.zeros(16, np.int16)
    out = C.c_int32(7)
    assert l.zlhip_sound_upload_pcm(None, x.ctypes.data, _abi.PCM_S16, 2, 8, 48000.0, C.byref(out)) == _abi.ZLHIP_ERR_INVALID
    src = (_abi.PcmSource * 1)(_abi.PcmSource(x.ctypes.data, 8, 2, _abi.PCM_S16, 0, 48000.0))
    ids = (C.c_int32 * 1)(7)
    assert l.zlhip_sound_upload_pcm_batch(None, src, 1, ids) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_group_sound_upload_pcm_batch(None, src, 1, ids) == _abi.ZLHIP_ERR_INVALID
    assert l.zlhip_debug_upload_pcm_timings(None, None, None) == _abi.ZLHIP_ERR_INVALID


def test_pcm_source_struct_layout(tmp_path):
    prog = tmp_path / "p.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zlhip.h"\nint main(void){printf("%d %d %d %d %d %d %d %d %d %d\\n",(int)sizeof(zlhip_pcm_source),'
                    '(int)offsetof(zlhip_pcm_source,frames),(int)offsetof(zlhip_pcm_source,length),(int)offsetof(zlhip_pcm_source,channels),'
                    '(int)offsetof(zlhip_pcm_source,format),(int)offsetof(zlhip_pcm_source,reserved),(int)offsetof(zlhip_pcm_source,sample_rate),'
                    'ZLHIP_PCM_MAX_CHANNELS,ZLHIP_PCM_U8,ZLHIP_PCM_F64);return 0;}\n')
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _abi.PcmSource
    assert got == [C.sizeof(P), P.frames.offset, P.length.offset, P.channels.offset, P.format.offset, P.reserved.offset, P.sample_rate.offset,
                   _abi.PCM_MAX_CHANNELS, _abi.PCM_U8, _abi.PCM_F64] == [32, 0, 8, 12, 16, 20, 24, 64, 1, 6]
    assert (_abi.PCM_S16, _abi.PCM_S24, _abi.PCM_S32, _abi.PCM_F32) == (dr.S16, dr.S24, dr.S32, dr.F32) and _abi.PCM_BYTES == dr.BYTES
