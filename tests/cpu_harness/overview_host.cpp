// Host build of the waveform overviews' definition (libzl_amd/csrc/zl_overview.h) for the CPU tier -- TEST HARNESS ONLY.
// zlov_run walks a request the way zl_k_overview_reduce does -- item by item, a piece's 16-byte groups lane by lane with the head and
// tail masked by zl_ov_valid, a narrow request's columns lane by lane -- with the header's own arithmetic, counts the visits of every
// float of the extent and accumulates the columns exactly as the kernels do (max of key and of ~key from zero, mapped back at the end).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "zl_overview.h"

extern "C" {

uint32_t zlov_key(uint32_t b) { return zl_ov_key(b); }
uint32_t zlov_unkey(uint32_t k) { return zl_ov_unkey(k); }

void zlov_column(int64_t first, int64_t frames, int64_t columns, int64_t c, int64_t *lo, int64_t *hi) { zl_ov_column(first, frames, columns, c, lo, hi); }
int32_t zlov_pieces_per_column(int64_t frames, int64_t columns) { return zl_ov_pieces_per_column(frames, columns); }
int64_t zlov_items(int64_t frames, int64_t columns) { return zl_ov_items(frames, columns); }
int32_t zlov_piece_frames(void) { return ZL_OV_PIECE_FRAMES; }
int32_t zlov_narrow_frames(void) { return ZL_OV_NARROW_FRAMES; }

// data: the extent, (length + 8) * channels words rounded up to 4 (interleaved, the pad behind the sound included).
// visits [extent words]: += 1 for every word that enters a column; owner [extent words]: the column it entered (-1: none).
// out [columns][4] words (minL, maxL, minR, maxR).  Returns the largest word index LOADED (masked or not), -1 on a malformed piece.
int64_t zlov_run(const uint32_t *data, int32_t channels, int32_t first, int32_t frames, int32_t columns, int32_t *visits, int32_t *owner, uint32_t *out)
{
    ZlOvRequest R;
    R.src = 0; R.item_base = 0; R.first = first; R.frames = frames; R.columns = columns; R.channels = channels; R.col_base = 0;
    R.ppc = zl_ov_pieces_per_column(frames, columns);
    const int64_t items = zl_ov_items(frames, columns);
    std::vector<uint32_t> acc((size_t)columns * 4, 0u);
    int64_t top = -1;
    auto take = [&](int64_t word, int32_t column, int ch) {
        visits[word] += 1; owner[word] = column;
        const uint32_t k = zl_ov_key(data[word]);
        uint32_t *a = &acc[(size_t)column * 4 + 2 * (size_t)ch];
        a[0] = std::max(a[0], ~k); a[1] = std::max(a[1], k);
    };
    for (int64_t i = 0; i < items; ++i) {
        if (R.ppc == 0) {
            for (int lane = 0; lane < ZL_OV_WAVE; ++lane) {
                const int64_t c = i * ZL_OV_WAVE + lane;
                if (c >= columns) continue;
                int64_t lo, hi;
                zl_ov_column(first, frames, columns, c, &lo, &hi);
                for (int64_t f = lo; f < hi; ++f)
                    for (int ch = 0; ch < channels; ++ch) { take(f * channels + ch, (int32_t)c, ch); top = std::max(top, f * channels + ch); }
            }
            continue;
        }
        int32_t column; int64_t lo, hi, f0, f1, g0, g1;
        zl_ov_piece(R, i, &column, &lo, &hi);
        if (hi <= lo || hi - lo > ZL_OV_PIECE_FRAMES) return -1;
        zl_ov_groups(lo, hi, channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        for (int32_t gb = 0; gb < ngroups; gb += ZL_OV_WAVE)
            for (int lane = 0; lane < ZL_OV_WAVE; ++lane) {
                const int32_t g = gb + lane;
                if (g >= ngroups) continue;                        // (the kernel's lanes behind the piece read its last group again: no new visit)
                top = std::max(top, 4 * (g0 + g) + 3);
                for (int j = 0; j < 4; ++j)
                    if (zl_ov_valid(g, j, head, count)) take(4 * (g0 + g) + j, column, channels == 2 ? (j & 1) : 0);
            }
    }
    for (int32_t c = 0; c < columns; ++c) {
        uint32_t *a = &acc[(size_t)c * 4];
        if (channels == 1) { a[2] = a[0]; a[3] = a[1]; }
        out[4 * c + 0] = zl_ov_unkey(~a[0]); out[4 * c + 1] = zl_ov_unkey(a[1]);
        out[4 * c + 2] = zl_ov_unkey(~a[2]); out[4 * c + 3] = zl_ov_unkey(a[3]);
    }
    return top;
}

}
