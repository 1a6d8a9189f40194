// zl_overview.h -- waveform overviews of a sound's playback data (zlhip_sound_overview / _batch): one
// (min, max) pair per channel and pixel column, the data behind the reference's WaveFormItem (lib/WaveFormItem.cpp:130-139 paints a
// juce::AudioThumbnail of the clip between `start` and `end`).  Shared by the HIP kernels (zl_overview.hip), the engine and a host
// build for the CPU tier (tests/cpu_harness/overview_host.cpp): the column bounds, the order of the samples and the way a request is
// cut into the units of work of one wavefront are defined HERE, once.
//
// A request is (sound, first_frame, num_frames, columns) over the sound's current playback data, 1 <= columns <= 4096,
// num_frames >= 1, first_frame >= 0, first_frame + num_frames <= length.
//
//   Columns.  Column c covers the frames [lo_c, hi_c):  lo_c = first_frame + floor(c * num_frames / columns),
//             hi_c = first_frame + floor((c + 1) * num_frames / columns), in int64; hi_c == lo_c (more columns than frames) makes the
//             column [lo_c, lo_c + 1).  Every column is non-empty and lies inside the request; with columns <= num_frames the columns
//             tile the request in order and their widths differ by at most one frame.
//
//   Order.    No float operation ever touches a sample.  The 32 bits b of a sample map to the key
//                 key(b) = ~b               if the sign bit of b is set
//                          b ^ 0x80000000   otherwise
//             and minimum and maximum are taken over the keys as UNSIGNED integers, then mapped back (zl_ov_unkey).  The map is a
//             bijection that is strictly monotone in the order  -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN:
//             -0 is below +0, a denormal comes back with its own bits, a NaN with the sign bit clear sorts above +inf (the larger
//             its payload the higher), one with the sign bit set below -inf.  A total order on integers is what makes every
//             reduction order, every cut into pieces and every lane mapping give the same bits.
//
//   Output.   Per column four floats (minL, maxL, minR, maxR); a mono sound repeats its channel in the R pair.  The requests of a
//             batch are packed one behind the other.
//
// The work.  A request is cut into ITEMS, each the work of one wavefront, numbered consecutively over the call (item_base):
//   wide requests   (a column may hold more than ZL_OV_NARROW_FRAMES frames): every column is cut evenly into ppc PIECES of at most
//                   ZL_OV_PIECE_FRAMES frames that never cross a column edge (ppc is the same for all columns of the request); an
//                   item is one piece.  The wave reads the piece's 16-byte groups of the arena's own layout (stereo [L0 R0 L1 R1],
//                   mono [x0 x1 x2 x3]; extents are 16-byte aligned), one group per lane and load; the elements of the first and
//                   last group that lie outside the piece are masked by their float index (zl_ov_valid) -- they belong to the
//                   neighbouring piece or column, to the frames around the request, or to the zero frames behind the extent, which
//                   also keep the last group's over-read inside the allocation.  The wave reduces with DPP integer max; one lane
//                   writes the column's four words (ppc == 1) or combines with the other pieces of the column by atomic max.
//   narrow requests (every column holds at most ZL_OV_NARROW_FRAMES frames): ONE LANE PER COLUMN loops over its few frames; an item
//                   is 64 consecutive columns.
// The accumulators are max(key) and max(~key): both unsigned, both start from zero, so a memset initialises them.
#pragma once
#include <stdint.h>

#include "zl_types.h"

#define ZL_OV_MAX_COLUMNS        4096        // per request (ZLHIP_OVERVIEW_MAX_COLUMNS)
#define ZL_OV_MAX_CALL_COLUMNS   262144      // per call
#define ZL_OV_PIECE_FRAMES       512         // a piece: at most this many frames
#define ZL_OV_NARROW_FRAMES      32          // a request whose widest column holds at most this many frames is narrow
#define ZL_OV_WAVE               64

ZL_HD inline uint32_t zl_ov_key(uint32_t b) { return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u); }
ZL_HD inline uint32_t zl_ov_unkey(uint32_t k) { return k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u); }

// the frames [*lo, *hi) of column c
ZL_HD inline void zl_ov_column(int64_t first, int64_t frames, int64_t columns, int64_t c, int64_t *lo, int64_t *hi)
{
    *lo = first + (c * frames) / columns;
    *hi = first + ((c + 1) * frames) / columns;
    if (*hi == *lo) *hi = *lo + 1;
}

// frames of the request's widest column
ZL_HD inline int64_t zl_ov_max_width(int64_t frames, int64_t columns) { return frames <= columns ? 1 : (frames + columns - 1) / columns; }

// pieces per column of a wide request; 0 = the request is narrow (one lane per column)
ZL_HD inline int32_t zl_ov_pieces_per_column(int64_t frames, int64_t columns)
{
    const int64_t w = zl_ov_max_width(frames, columns);
    return w <= ZL_OV_NARROW_FRAMES ? 0 : (int32_t)((w + ZL_OV_PIECE_FRAMES - 1) / ZL_OV_PIECE_FRAMES);
}

// items (wavefronts' worth of work) of a request
ZL_HD inline int64_t zl_ov_items(int64_t frames, int64_t columns)
{
    const int32_t ppc = zl_ov_pieces_per_column(frames, columns);
    return ppc == 0 ? (columns + ZL_OV_WAVE - 1) / ZL_OV_WAVE : columns * (int64_t)ppc;
}

// One request of a call as the kernel sees it (built by the host: no per-frame work there)
struct ZlOvRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned; built per request with 64-bit arithmetic)
    int64_t  item_base;          // the request's first item in the call
    int32_t  first, frames, columns;
    int32_t  channels;           // 1 or 2
    int32_t  col_base;           // the request's first column in the call's packed output
    int32_t  ppc;                // zl_ov_pieces_per_column
};

// item `i` (relative to the request) of a wide request: its column and the frames [*lo, *hi) of its piece
ZL_HD inline void zl_ov_piece(const ZlOvRequest &R, int64_t i, int32_t *column, int64_t *lo, int64_t *hi)
{
    const int64_t c = i / R.ppc, p = i - c * R.ppc;
    int64_t clo, chi;
    zl_ov_column(R.first, R.frames, R.columns, c, &clo, &chi);
    const int64_t w = chi - clo;                                   // >= ZL_OV_NARROW_FRAMES >= ppc: no piece is empty
    *column = (int32_t)c;
    *lo = clo + (p * w) / R.ppc;
    *hi = clo + ((p + 1) * w) / R.ppc;
}

// the 16-byte groups [*g0, *g1) that hold the floats [*f0, *f1) of the frames [lo, hi)
ZL_HD inline void zl_ov_groups(int64_t lo, int64_t hi, int channels, int64_t *f0, int64_t *f1, int64_t *g0, int64_t *g1)
{
    *f0 = lo * channels; *f1 = hi * channels;
    *g0 = *f0 >> 2; *g1 = (*f1 + 3) >> 2;
}

// does element j (0..3) of the group that lies `grel` groups behind the piece's first group belong to the piece?  head = f0 - 4 * g0
// (floats of the first group in front of the piece), count = f1 - f0.  (32-bit: a piece holds at most 2 * ZL_OV_PIECE_FRAMES + 2 floats)
ZL_HD inline bool zl_ov_valid(int32_t grel, int j, int32_t head, int32_t count) { return (uint32_t)(4 * grel + j - head) < (uint32_t)count; }

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_overview.hip; 0 or a hipError_t value).  acc: [columns][4] words, zero before the reduce launch; the finish launch
// turns them in place into the floats (minL, maxL, minR, maxR)
int zl_launch_overview_reduce(const ZlOvRequest *reqs, int32_t nreq, int64_t items, uint32_t *acc, hipStream_t s);
int zl_launch_overview_finish(uint32_t *acc, int32_t columns, hipStream_t s);
#endif
