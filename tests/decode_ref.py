"""The PCM upload's definition (include/zlhip.h, zlhip_sound_upload_pcm; libzl_amd/csrc/zl_decode.h), restated in numpy and
independently of the product's code: interleaved little-endian samples -> the planar float32 playback data, the arena extent with
its zero frames, the finite verdict -- and a WAV writer for every format the decode side takes."""
import struct

import numpy as np

U8, S16, S24, S32, F32, F64 = 1, 2, 3, 4, 5, 6
FORMATS = (U8, S16, S24, S32, F32, F64)
NAMES = {U8: "u8", S16: "s16", S24: "s24", S32: "s32", F32: "f32", F64: "f64"}
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
PAD = 8
f32, u32 = np.float32, np.uint32


def raw_bytes(data):
    """numpy array or bytes -> a flat uint8 array of the bytes as they lie in memory (little-endian host)"""
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), np.uint8)
    return np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def widen(raw, fmt):
    """integer formats: the samples as left-justified int32"""
    b = raw_bytes(raw).astype(np.int64)
    if fmt == U8:
        v = (b - 128) << 24
    elif fmt == S16:
        b = b.reshape(-1, 2)
        v = (b[:, 0] << 16) | (b[:, 1] << 24)
    elif fmt == S24:
        b = b.reshape(-1, 3)
        v = (b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)
    elif fmt == S32:
        b = b.reshape(-1, 4)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)
    else:
        raise ValueError(fmt)
    v = np.where(v >= 2 ** 31, v - 2 ** 32, v)                     # two's complement
    assert (v >= -2 ** 31).all() and (v < 2 ** 31).all()
    return v


def samples(raw, fmt):
    """every sample of the stream as float32, in stream order"""
    if fmt == F32:
        return raw_bytes(raw).view(f32).copy()                     # moved as bits
    if fmt == F64:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return raw_bytes(raw).view(np.float64).astype(f32)     # round-to-nearest-even, denormals kept, overflow to inf
    # an int32 is exact in a double, so is its product with 2^-31; one rounding to float32 (nearest even) is the rounding of the
    # conversion, the scale by a power of two being exact behind it (the smallest magnitude is 2^-31: no denormal is near)
    return (widen(raw, fmt).astype(np.float64) * 2.0 ** -31).astype(f32)


def decode(raw, fmt, channels):
    """-> planar float32 [min(2, channels)][length]"""
    s = samples(raw, fmt).reshape(-1, channels)
    return np.ascontiguousarray(s[:, :min(2, channels)].T)


def extent(planar):
    """the words of the arena extent: interleaved, PAD zero frames behind the clip, zeros up to 16 bytes"""
    ch, length = planar.shape
    words = ((length + PAD) * ch + 3) & ~3
    ext = np.zeros(words, u32)
    ext[:length * ch] = np.ascontiguousarray(planar.T).reshape(-1).view(u32)
    return ext


def finite(planar):
    return bool(((planar.view(u32) & u32(0x7F800000)) != u32(0x7F800000)).all())


def same(got, ref, fmt):
    """bit for bit; an F64 source's NaNs compare by NaN-ness and sign only (their payload is build-defined)"""
    g, r = np.ascontiguousarray(got).view(u32), np.ascontiguousarray(ref).view(u32)
    if g.shape != r.shape:
        return False
    if fmt != F64:
        return bool(np.array_equal(g, r))
    gn, rn = np.isnan(g.view(f32)), np.isnan(r.view(f32))
    return bool(np.array_equal(gn, rn) and np.array_equal(g[~gn], r[~rn]) and np.array_equal(g[gn] >> 31, r[rn] >> 31))


def random_raw(rng, fmt, channels, length):
    """a stream of `length` frames: full-range integers, floats in [-1, 1)"""
    n = length * channels
    if fmt in (U8, S16, S24, S32):
        return rng.integers(0, 256, n * BYTES[fmt], dtype=np.uint8)
    x = rng.uniform(-1.0, 1.0, n)
    return raw_bytes(x.astype(f32 if fmt == F32 else np.float64)).copy()


def wav_bytes(raw, fmt, channels, rate, extensible=False):
    data = raw_bytes(raw).tobytes()
    bits = 8 * BYTES[fmt]
    tag = 3 if fmt in (F32, F64) else 1
    block = channels * BYTES[fmt]
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:
        # cbSize, valid bits, channel mask, sub-format GUID (the tag, then the fixed tail of KSDATAFORMAT_SUBTYPE_*)
        head += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write_wav(path, raw, fmt, channels, rate, extensible=False):
    with open(path, "wb") as f:
        f.write(wav_bytes(raw, fmt, channels, rate, extensible))
