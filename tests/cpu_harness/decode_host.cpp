// decode_host.cpp -- host build of libzl_amd/csrc/zl_decode.h for the CPU tier (tests/test_decode_cpu.py): the conversions of every
// format, and a whole call walked the way zl_k_pcm_decode walks it -- the header's cut into passes and pieces, every item of every
// pass, 64 lanes per item, zl_dec_lane per lane -- against a stage that records every byte it is asked for.
#include <cstdint>
#include <cstring>
#include <vector>

#include "zl_decode.h"

namespace {

// the stage of one pass: `owner[b]` is the piece whose bytes lie at b (-1: nobody's); a read of a byte the current piece does not own
// is counted, and answered with a byte no clip holds in that place
struct HostStage {
    const unsigned char *bytes; const int32_t *owner; size_t size; int32_t piece; int64_t *foreign;
    uint32_t byte(uint32_t off) const
    {
        if (off >= size || owner[off] != piece) { ++*foreign; return 0xA5u; }
        return bytes[off];
    }
    template <int N> void dwords(uint32_t off, uint32_t *w) const
    {
        if (off % 4u) ++*foreign;                                  // (an unaligned vector load)
        for (int i = 0; i < N; ++i) {
            w[i] = 0u;
            for (int b = 0; b < 4; ++b) w[i] |= byte(off + 4u * (uint32_t)i + (uint32_t)b) << (8 * b);
        }
    }
};

}  // namespace

extern "C" {

int zldec_bytes(int format) { return zl_dec_bytes(format); }
uint32_t zldec_stage_bytes(int64_t asked) { return zl_dec_stage_bytes(asked); }
uint64_t zldec_extent_floats(int64_t length, int out_channels) { return zl_dec_extent_floats(length, out_channels); }
int zldec_piece_record_bytes(void) { return (int)sizeof(ZlDecPiece); }

// The header's cut of one call (zl_dec_plan): per piece its clip, its pass, its item_base and its items (arrays of `capacity`, filled
// up to it); returns the number of pieces and leaves the number of passes.
int32_t zldec_plan(int32_t count, const int32_t *lengths, const int32_t *channels, const int32_t *formats, int64_t stage_asked, int32_t capacity,
                   int32_t *clip, int32_t *pass, int32_t *item_base, int32_t *items, int32_t *npasses)
{
    std::vector<ZlDecClip> clips((size_t)count);
    for (int32_t c = 0; c < count; ++c) clips[(size_t)c] = ZlDecClip{ lengths[c], channels[c], formats[c] };
    std::vector<ZlDecPiece> pieces; std::vector<ZlDecPass> passes;
    zl_dec_plan(clips.data(), count, zl_dec_stage_bytes(stage_asked), pieces, passes);
    *npasses = (int32_t)passes.size();
    for (size_t a = 0; a < passes.size(); ++a)
        for (int32_t k = passes[a].first_piece; k < passes[a].first_piece + passes[a].npieces && k < capacity; ++k) {
            const ZlDecPiece &R = pieces[(size_t)k];
            clip[k] = R.verdict; pass[k] = (int32_t)a; item_base[k] = R.item_base; items[k] = zl_dec_piece_items(R);
        }
    return (int32_t)pieces.size();
}

// n samples of one format, one by one, with the header's widening and conversion
void zldec_convert(int format, const unsigned char *src, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i) {
        const unsigned char *p = src + i * zl_dec_bytes(format);
        uint32_t lo = 0u, hi = 0u;
        for (int b = 0; b < zl_dec_bytes(format); ++b) { if (b < 4) lo |= (uint32_t)p[b] << (8 * b); else hi |= (uint32_t)p[b] << (8 * (b - 4)); }
        switch (format) {
        case ZL_PCM_U8:  out[i] = zl_dec_int(zl_dec_widen_u8(lo)); break;
        case ZL_PCM_S16: out[i] = zl_dec_int(zl_dec_widen_s16(lo)); break;
        case ZL_PCM_S24: out[i] = zl_dec_int(zl_dec_widen_s24(lo)); break;
        case ZL_PCM_S32: out[i] = zl_dec_int((int32_t)lo); break;
        case ZL_PCM_F32: out[i] = lo; break;
        default:         out[i] = zl_dec_f64(lo, hi); break;
        }
    }
}

// One call.  srcs[c]: the clip's raw bytes; outs[c] / writes[c]: the words of its extent and how often each was written;
// verdicts[c]: set when a lane reported a non-finite sample.  Returns the number of violations -- a stage byte read that the
// piece at work does not own, a piece off its 4-frame or 16-byte boundary or past the stage, a store outside the extent, an item
// without a piece -- and leaves the number of passes and pieces.
int64_t zldec_run(int32_t count, const int32_t *lengths, const int32_t *channels, const int32_t *formats, const unsigned char *const *srcs,
                  int64_t stage_asked, uint32_t *const *outs, int32_t *const *writes, uint32_t *verdicts, int32_t *npasses, int32_t *npieces)
{
    std::vector<ZlDecClip> clips((size_t)count);
    for (int32_t c = 0; c < count; ++c) clips[(size_t)c] = ZlDecClip{ lengths[c], channels[c], formats[c] };
    const uint32_t stageBytes = zl_dec_stage_bytes(stage_asked);
    std::vector<ZlDecPiece> pieces; std::vector<ZlDecPass> passes;
    zl_dec_plan(clips.data(), count, stageBytes, pieces, passes);
    *npasses = (int32_t)passes.size(); *npieces = (int32_t)pieces.size();
    int64_t bad = 0;
    // every frame of every clip lies in exactly one piece, in order
    {
        std::vector<int64_t> next((size_t)count, 0);
        for (const ZlDecPiece &R : pieces) {
            if (R.first != next[(size_t)R.verdict] || R.frames < 1) ++bad;
            next[(size_t)R.verdict] = (int64_t)R.first + R.frames;
        }
        for (int32_t c = 0; c < count; ++c) if (next[(size_t)c] != lengths[c]) ++bad;
    }
    for (const ZlDecPass &P : passes) {
        if (P.bytes > stageBytes) { ++bad; continue; }
        std::vector<unsigned char> stage(P.bytes, 0x5A);
        std::vector<int32_t> owner(P.bytes, -1);
        int32_t items = 0;
        for (int32_t k = P.first_piece; k < P.first_piece + P.npieces; ++k) {
            const ZlDecPiece &R = pieces[(size_t)k];
            const uint64_t n = zl_dec_piece_bytes(R);
            if (R.first % 4 || R.stage_off % 16u || (uint64_t)R.stage_off + n > P.bytes || R.item_base != items) { ++bad; continue; }
            if ((int64_t)R.first + R.frames != R.length && R.frames % 4) ++bad;
            std::memcpy(stage.data() + R.stage_off, srcs[R.verdict] + zl_dec_source_offset(R), (size_t)n);
            for (uint64_t b = 0; b < n; ++b) { if (owner[R.stage_off + b] != -1) ++bad; owner[R.stage_off + b] = k; }
            items += zl_dec_piece_items(R);
        }
        if (items != P.items) ++bad;
        if (bad) continue;
        const ZlDecPiece *pp = pieces.data() + P.first_piece;
        for (int32_t it = 0; it < P.items; ++it) {
            // the piece of the item: the last one whose item_base is <= it, by bisection as in the kernel
            int32_t r = 0;
            for (int32_t lo = 0, hi = P.npieces - 1; ; ) {
                if (lo >= hi) { r = lo; break; }
                const int32_t mid = (lo + hi + 1) >> 1;
                if (pp[mid].item_base <= it) lo = mid; else hi = mid - 1;
            }
            const ZlDecPiece &R = pp[r];
            const int32_t ngroups = (int32_t)zl_dec_piece_groups(R);
            if (it - R.item_base >= zl_dec_piece_items(R)) { ++bad; continue; }
            const HostStage S = { stage.data(), owner.data(), stage.size(), P.first_piece + r, &bad };
            const uint64_t extent = zl_dec_extent_floats(R.length, zl_dec_out_channels(R.channels));
            for (int lane = 0; lane < ZL_DEC_WAVE; ++lane) {
                const int32_t g = (it - R.item_base) * ZL_DEC_WAVE + lane;
                if (g >= ngroups) continue;
                uint32_t o[4];
                if (zl_dec_lane(R, g, S, o)) verdicts[R.verdict] = 1u;
                const int64_t f = zl_dec_group_float(R, g);
                if (f < 0 || (f & 3) || (uint64_t)f + 4 > extent) { ++bad; continue; }
                for (int k = 0; k < 4; ++k) { outs[R.verdict][f + k] = o[k]; writes[R.verdict][f + k] += 1; }
            }
        }
    }
    return bad;
}

}  // extern "C"
