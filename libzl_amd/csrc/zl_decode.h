// zl_decode.h -- clips from raw PCM (zlhip_sound_upload_pcm / _batch): interleaved little-endian samples, exactly
// the bytes of a WAV `data` chunk, are copied raw into a device staging buffer and decoded there into the arena's layout.  Shared by
// the HIP kernel (zl_decode.hip), the engine and a host build for the CPU tier (tests/cpu_harness/decode_host.cpp): the conversion of
// every format, the cut of a call into passes and pieces, and what one lane does with one 16-byte output group are defined HERE, once.
//
//   Formats.  U8 / S16 / S24 / S32 widen to left-justified int32 -- (b - 128) << 24, << 16, three bytes << 8, as it is -- convert to
//             float with round-to-nearest-even and multiply by 2^-31 (exact after the conversion): libzl_wav_read's rule.  F32 is moved
//             as 32 bits, no float operation touches it.  F64 is (float)d, round-to-nearest-even: fp32 denormals stay denormal,
//             overflow gives +-inf, a NaN a NaN of the same sign.
//   Channels. The first min(2, channels) channels are kept (SamplerSynthSound.cpp:45); the sound is mono only when channels == 1.
//   Extent.   What zl_k_interleave writes: [L0 R0 L1 R1 ...] or [x0 x1 ...], ZL_ST_PAD zero frames behind it, zeros up to the 16-byte
//             boundary.  Floats at or beyond `length` are +0 and are produced WITHOUT reading the stage: the bytes behind a clip in
//             the stage belong to another clip, or to nobody.
//
// The work.  A call runs in PASSES: the next PIECES are copied into the stage, one launch decodes them.  A piece is a run of one clip's
// frames that starts at a multiple of 4 frames -- so its first output float starts a 16-byte group for one and for two kept channels --
// and lies at a 16-byte-aligned stage offset; a clip longer than the stage is cut into several.  The LAST piece of a clip also owns the
// clip's zero frames and the floats up to the end of the extent.  One lane writes one 16-byte GROUP (four floats: two stereo frames or
// four mono frames); an ITEM is the 64 consecutive groups of one wavefront, numbered over the pass (item_base).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "zl_types.h"

#define ZL_DEC_PAD            8           // zero frames behind a clip (ZL_ST_PAD, zl_stretch.h; the 8 of zlhip_sound_upload)
#define ZL_DEC_WAVE           64
#define ZL_DEC_MAX_CHANNELS   64          // ZLHIP_PCM_MAX_CHANNELS
#define ZL_DEC_STAGE_DEFAULT  (64u << 20)
#define ZL_DEC_STAGE_MIN      4096u       // holds four frames of 64 channels of F64 (2048 bytes)
#define ZL_DEC_STAGE_MAX      (1u << 30)  // a pass stays well below 4 GiB: offsets in the kernel are 32-bit

enum { ZL_PCM_U8 = 1, ZL_PCM_S16 = 2, ZL_PCM_S24 = 3, ZL_PCM_S32 = 4, ZL_PCM_F32 = 5, ZL_PCM_F64 = 6 };

ZL_HD inline int zl_dec_bytes(int format) { return format == ZL_PCM_U8 ? 1 : format == ZL_PCM_S16 ? 2 : format == ZL_PCM_S24 ? 3 : format == ZL_PCM_F64 ? 8 : 4; }
ZL_HD inline bool zl_dec_is_float(int format) { return format == ZL_PCM_F32 || format == ZL_PCM_F64; }
ZL_HD inline int zl_dec_out_channels(int channels) { return channels < 2 ? 1 : 2; }
// floats of the arena extent of a clip (extent_floats, zl_engine.cpp)
ZL_HD inline uint64_t zl_dec_extent_floats(int64_t length, int out_channels) { return (((uint64_t)length + ZL_DEC_PAD) * (uint64_t)out_channels + 3u) & ~(uint64_t)3; }
// the size of the stage: at least ZL_DEC_STAGE_MIN, a multiple of 16
ZL_HD inline uint32_t zl_dec_stage_bytes(int64_t asked)
{
    if (asked < (int64_t)ZL_DEC_STAGE_MIN) asked = ZL_DEC_STAGE_MIN;
    if (asked > (int64_t)ZL_DEC_STAGE_MAX) asked = ZL_DEC_STAGE_MAX;
    return (uint32_t)((asked + 15) & ~(int64_t)15);
}

// ---- conversions (bits in, float bits out) ------------------------------------------------------------------------------------
ZL_HD inline uint32_t zl_dec_f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
ZL_HD inline uint32_t zl_dec_int(int32_t s) { return zl_dec_f2u((float)s * (1.0f / 2147483648.0f)); }   // cvt (round-to-nearest-even), then an exact scale
ZL_HD inline int32_t zl_dec_widen_u8(uint32_t b) { return (int32_t)(((b & 0xffu) - 128u) << 24); }
ZL_HD inline int32_t zl_dec_widen_s16(uint32_t h) { return (int32_t)(h << 16); }
ZL_HD inline int32_t zl_dec_widen_s24(uint32_t t) { return (int32_t)(t << 8); }                         // t: b0 | b1 << 8 | b2 << 16
ZL_HD inline uint32_t zl_dec_f64(uint32_t lo, uint32_t hi)
{
    const uint64_t b = ((uint64_t)hi << 32) | lo;
    double d; __builtin_memcpy(&d, &b, 8);
    return zl_dec_f2u((float)d);
}
ZL_HD inline bool zl_dec_bits_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// One piece of a pass as the kernel sees it (built by the host: no per-frame work there)
struct ZlDecPiece {
    uint64_t dst;                // device address of the CLIP's extent (16-byte aligned; 64-bit: a grown arena's segments lie far apart)
    uint32_t stage_off;          // bytes from the stage's start to the piece's first frame (a multiple of 16)
    int32_t  first;              // the piece's first frame in the clip (a multiple of 4)
    int32_t  frames;             // frames of the piece (a multiple of 4 unless the piece ends the clip)
    int32_t  length;             // frames of the clip
    int32_t  channels;           // of the source, 1 .. 64
    int32_t  format;             // ZL_PCM_*
    int32_t  verdict;            // the clip's word among the call's verdicts (set when a kept, converted sample is not finite)
    int32_t  item_base;          // the piece's first item in its pass
};

// groups the piece writes: its frames' floats; the clip's last piece goes on to the end of the extent
ZL_HD inline int64_t zl_dec_piece_groups(const ZlDecPiece &R)
{
    const int oc = zl_dec_out_channels(R.channels);
    const bool last = (int64_t)R.first + R.frames == R.length;
    const uint64_t f0 = (uint64_t)R.first * (uint64_t)oc;
    const uint64_t f1 = last ? zl_dec_extent_floats(R.length, oc) : ((uint64_t)R.first + (uint64_t)R.frames) * (uint64_t)oc;
    return (int64_t)((f1 - f0) >> 2);
}
ZL_HD inline int32_t zl_dec_piece_items(const ZlDecPiece &R) { return (int32_t)((zl_dec_piece_groups(R) + ZL_DEC_WAVE - 1) / ZL_DEC_WAVE); }

// What one lane does with group g of a piece (g counts from the piece's first group): out[0..3] are the bits of the four floats the
// group holds in the extent, from float index 4 * g behind the piece's first float; returns 1 when one of them is not finite.
//   S: the stage.  S::dwords<N>(byte offset, w) loads N consecutive dwords from a 4-byte-aligned offset, S::byte(offset) one byte.
// A group that lies wholly inside the piece's frames of a source with one or two channels is contiguous in the stage and starts on
// a dword: one or two vector loads, then shifts and masks.  Any other group that holds samples (more than two channels, or the
// clip's last group when it is not full) takes them byte by byte; floats behind the clip are +0 and nothing is read for them.
template <class S> ZL_HD inline uint32_t zl_dec_lane(const ZlDecPiece &R, int32_t g, const S &stage, uint32_t out[4])
{
    const int oc = zl_dec_out_channels(R.channels);
    const int bytes = zl_dec_bytes(R.format);
    const int64_t j0 = 4 * (int64_t)g;                              // float index behind the piece's first float
    const int64_t have = (int64_t)R.frames * oc - j0;               // floats of the piece's frames from there on
    const int nvalid = have >= 4 ? 4 : (have > 0 ? (int)have : 0);
    out[0] = out[1] = out[2] = out[3] = 0u;
    if (nvalid == 4 && R.channels <= 2) {
        const uint32_t off = R.stage_off + (uint32_t)j0 * (uint32_t)bytes;
        uint32_t w[8];
        switch (R.format) {
        case ZL_PCM_U8:
            stage.template dwords<1>(off, w);
            for (int k = 0; k < 4; ++k) out[k] = zl_dec_int(zl_dec_widen_u8(w[0] >> (8 * k)));
            break;
        case ZL_PCM_S16:
            stage.template dwords<2>(off, w);
            out[0] = zl_dec_int(zl_dec_widen_s16(w[0])); out[1] = zl_dec_int((int32_t)(w[0] & 0xffff0000u));
            out[2] = zl_dec_int(zl_dec_widen_s16(w[1])); out[3] = zl_dec_int((int32_t)(w[1] & 0xffff0000u));
            break;
        case ZL_PCM_S24:
            stage.template dwords<3>(off, w);                       // bytes 0-2 | 3-5 | 6-8 | 9-11
            out[0] = zl_dec_int((int32_t)(w[0] << 8));
            out[1] = zl_dec_int((int32_t)((w[0] >> 16) & 0x0000ff00u) | (int32_t)(w[1] << 16));
            out[2] = zl_dec_int((int32_t)((w[1] >> 8) & 0x00ffff00u) | (int32_t)(w[2] << 24));
            out[3] = zl_dec_int((int32_t)(w[2] & 0xffffff00u));
            break;
        case ZL_PCM_S32:
            stage.template dwords<4>(off, w);
            for (int k = 0; k < 4; ++k) out[k] = zl_dec_int((int32_t)w[k]);
            break;
        case ZL_PCM_F32:
            stage.template dwords<4>(off, out);
            break;
        default:
            stage.template dwords<4>(off, w); stage.template dwords<4>(off + 16u, w + 4);
            for (int k = 0; k < 4; ++k) out[k] = zl_dec_f64(w[2 * k], w[2 * k + 1]);
            break;
        }
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k) {                               // (constant indices: out[] stays in registers)
            if (k >= nvalid) break;
            const int64_t j = j0 + k;
            const int64_t frame = oc == 2 ? (j >> 1) : j;
            const int ch = oc == 2 ? (int)(j & 1) : 0;
            const uint32_t off = R.stage_off + (uint32_t)((frame * R.channels + ch) * bytes);
            uint32_t lo = 0u, hi = 0u;
            for (int b = 0; b < bytes; ++b) {
                const uint32_t v = stage.byte(off + (uint32_t)b);
                if (b < 4) lo |= v << (8 * b); else hi |= v << (8 * (b - 4));
            }
            switch (R.format) {
            case ZL_PCM_U8:  out[k] = zl_dec_int(zl_dec_widen_u8(lo)); break;
            case ZL_PCM_S16: out[k] = zl_dec_int(zl_dec_widen_s16(lo)); break;
            case ZL_PCM_S24: out[k] = zl_dec_int(zl_dec_widen_s24(lo)); break;
            case ZL_PCM_S32: out[k] = zl_dec_int((int32_t)lo); break;
            case ZL_PCM_F32: out[k] = lo; break;
            default:         out[k] = zl_dec_f64(lo, hi); break;
            }
        }
    }
    if (!zl_dec_is_float(R.format)) return 0u;
    return (zl_dec_bits_finite(out[0]) && zl_dec_bits_finite(out[1]) && zl_dec_bits_finite(out[2]) && zl_dec_bits_finite(out[3])) ? 0u : 1u;
}

// float index in the clip's extent of the first float of group g of the piece (64-bit: a clip may hold more than 2^31 floats)
ZL_HD inline int64_t zl_dec_group_float(const ZlDecPiece &R, int32_t g) { return (int64_t)R.first * zl_dec_out_channels(R.channels) + 4 * (int64_t)g; }

// ---- the cut of a call into passes and pieces (host) ----------------------------------------------------------------------------
struct ZlDecClip { int32_t length, channels, format; };
struct ZlDecPass { int32_t first_piece, npieces, items; uint32_t bytes; };   // bytes: the stage bytes the pass uses

#include <vector>
// bytes from the clip's first sample to the piece's first frame in the CALLER's memory (64-bit)
inline uint64_t zl_dec_source_offset(const ZlDecPiece &R) { return (uint64_t)R.first * (uint64_t)R.channels * (uint64_t)zl_dec_bytes(R.format); }
inline uint64_t zl_dec_piece_bytes(const ZlDecPiece &R) { return (uint64_t)R.frames * (uint64_t)R.channels * (uint64_t)zl_dec_bytes(R.format); }

// pieces[i].verdict is the clip's index in `clips`; dst is left 0 for the caller to fill
inline void zl_dec_plan(const ZlDecClip *clips, int32_t count, uint32_t stage_bytes, std::vector<ZlDecPiece> &pieces, std::vector<ZlDecPass> &passes)
{
    pieces.clear(); passes.clear();
    ZlDecPass P = { 0, 0, 0, 0u };
    uint64_t pos = 0;
    auto close = [&]() {
        if (P.npieces > 0) { P.bytes = (uint32_t)pos; passes.push_back(P); }
        P.first_piece = (int32_t)pieces.size(); P.npieces = 0; P.items = 0; P.bytes = 0u;
        pos = 0;
    };
    for (int32_t c = 0; c < count; ++c) {
        const uint64_t fb = (uint64_t)clips[c].channels * (uint64_t)zl_dec_bytes(clips[c].format);
        int64_t f = 0;
        while (f < clips[c].length) {
            const int64_t fit = (int64_t)(((uint64_t)stage_bytes - pos) / fb) & ~(int64_t)3;   // whole runs of four frames the stage still holds
            const int64_t rest = (int64_t)clips[c].length - f;
            if (fit < rest && fit < 4) { close(); continue; }       // (an empty stage holds four frames of any format: ZL_DEC_STAGE_MIN)
            ZlDecPiece R;
            R.dst = 0; R.stage_off = (uint32_t)pos; R.first = (int32_t)f; R.frames = (int32_t)(fit >= rest ? rest : fit);
            R.length = clips[c].length; R.channels = clips[c].channels; R.format = clips[c].format; R.verdict = c; R.item_base = P.items;
            P.items += zl_dec_piece_items(R);
            P.npieces += 1;
            pieces.push_back(R);
            pos = (pos + (uint64_t)R.frames * fb + 15u) & ~(uint64_t)15;
            f += R.frames;
        }
    }
    close();
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// One entry of the sound table a call publishes: the device sets ZL_SOUND_FINITE from the clip's verdict word (check != 0) or without
// looking (integer formats), so the table entries of the whole call go up behind the last pass with no host wait in between
struct ZlDecPublish { ZlSound s; int32_t id, check; };
// launchers (zl_decode.hip; 0 or a hipError_t value)
int zl_launch_pcm_decode(const ZlDecPiece *pieces, int32_t npieces, int32_t items, const void *stage, uint32_t *verdicts, hipStream_t s);
int zl_launch_pcm_publish(const ZlDecPublish *recs, int32_t n, const uint32_t *verdicts, ZlSound *table, hipStream_t s);
#endif
