// Host build of zl_resample.h for the CPU tier (tests/test_resample_cpu.py): one clip converted the way zl_k_resample walks it --
// workgroup by workgroup, the staged span masked by the header's zl_rs_in_clip, one lane per output frame, the last workgroup's zero
// floats -- with the header's own arithmetic and a count of the writes per float of the extent.  The source is read through an
// accessor that knows nothing of the mask: it checks the float's index against the buffer it was given and refuses what lies outside.
#include <stdint.h>
#include <stddef.h>
#include <vector>

#include "zl_resample.h"

namespace {
// the clip's floats as the caller handed them over; a read outside them is counted and answered with a NaN, so that it also shows in the bits
struct Source {
    const float *p; int64_t floats; int64_t refused;
    float at(int64_t index)
    {
        if (index < 0 || index >= floats) { refused += 1; return __builtin_nanf(""); }
        return p[index];
    }
};
}  // namespace

extern "C" {

// out: L, M, half, taps, row
int zl_rs_host_geometry(double fs, double ft, int32_t *out)
{
    ZlRsGeom g;
    if (zl_rs_geometry(fs, ft, &g) != 0) return -1;
    out[0] = g.L; out[1] = g.M; out[2] = g.half; out[3] = g.taps; out[4] = g.row;
    return 0;
}

int64_t zl_rs_host_out_frames(double fs, double ft, int64_t len)
{
    ZlRsGeom g;
    if (zl_rs_geometry(fs, ft, &g) != 0) return -1;
    return zl_rs_out_frames(g, len);
}

int64_t zl_rs_host_extent_floats(int64_t N, int32_t channels) { return (int64_t)zl_rs_extent_floats(N, channels); }

int32_t zl_rs_host_stage_frames(void) { return ZL_RS_STAGE_FRAMES; }

// zl_rs_position of output frame j and zl_rs_span of workgroup w for a clip of `len` source frames (int64: the two functions read the
// job's N and ratio, not its len, so a length beyond what a job record holds still walks them to the end of the range).
// out: N, i, p, first, count.  -1 on a bad ratio, -3 where zl_rs_out_frames answers 0.
int zl_rs_host_walk(double fs, double ft, int64_t len, int64_t j, int32_t w, int64_t *out)
{
    ZlRsGeom g;
    if (zl_rs_geometry(fs, ft, &g) != 0) return -1;
    const int64_t N = zl_rs_out_frames(g, len);
    if (N < 1) return -3;
    ZlRsJob J = {};
    J.len = len > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)len; J.N = (int32_t)N; J.channels = 1;
    J.L = g.L; J.M = g.M; J.half = g.half; J.taps = g.taps; J.row = g.row;
    int64_t i, first; int32_t p, count;
    zl_rs_position(J, j, &i, &p);
    zl_rs_span(J, w, &first, &count);
    out[0] = N; out[1] = i; out[2] = p; out[3] = first; out[4] = count;
    return 0;
}

// the header's own table (the tests feed the LIBRARY's, and hold this one against it)
int zl_rs_host_design(double fs, double ft, float *table)
{
    ZlRsGeom g;
    if (zl_rs_geometry(fs, ft, &g) != 0) return -1;
    zl_rs_design(g, table);
    return 0;
}

// src: src_floats floats, interleaved, of which the clip is the first len * channels; dst and writes: the extent's floats.  Returns the
// number of source reads the accessor refused, -1 on a bad ratio, -2 where a lane's taps leave the staged span.
// *verdict: 1 when an output sample is not finite.
int64_t zl_rs_host_convert(double fs, double ft, const float *table, const float *src, int64_t src_floats, int32_t len, int32_t channels,
                           float *dst, int32_t *writes, uint32_t *verdict)
{
    ZlRsGeom g;
    if (zl_rs_geometry(fs, ft, &g) != 0) return -1;
    ZlRsJob J = {};
    J.len = len; J.N = (int32_t)zl_rs_out_frames(g, len); J.channels = channels;
    J.L = g.L; J.M = g.M; J.half = g.half; J.taps = g.taps; J.row = g.row;
    Source S = { src, src_floats, 0 };
    *verdict = 0u;
    std::vector<float> stage((size_t)ZL_RS_STAGE_FRAMES * 2);
    const int32_t wgs = zl_rs_job_wgs(J.N);
    for (int32_t w = 0; w < wgs; ++w) {
        int64_t first; int32_t count;
        zl_rs_span(J, w, &first, &count);
        if (count > ZL_RS_STAGE_FRAMES) return -2;
        for (int32_t k = 0; k < count; ++k) {
            const int64_t f = first + k;
            for (int c = 0; c < channels; ++c) {
                float v = 0.0f;
                if (zl_rs_in_clip(J, f)) v = S.at(f * channels + c);
                stage[(size_t)k * channels + c] = v;
            }
        }
        for (int32_t tid = 0; tid < ZL_RS_WG; ++tid) {
            const int64_t j = (int64_t)w * ZL_RS_WG + tid;
            if (j < (int64_t)J.N) {
                int64_t i; int32_t p;
                zl_rs_position(J, j, &i, &p);
                const int64_t o = i - J.half + 1 - first;
                if (o < 0 || o + J.taps > count) return -2;
                const float *row = table + (size_t)p * (size_t)J.row;
                for (int c = 0; c < channels; ++c) {
                    float acc = 0.0f;
                    for (int32_t t = 0; t < J.taps; ++t) acc = zl_rs_tap(acc, row[t], stage[(size_t)(o + t) * channels + c]);
                    dst[j * channels + c] = acc;
                    writes[j * channels + c] += 1;
                    if (!zl_rs_finite(acc)) *verdict = 1u;
                }
            }
            if (w == wgs - 1 && tid < zl_rs_tail_floats(J)) {
                dst[(int64_t)J.N * channels + tid] = 0.0f;
                writes[(int64_t)J.N * channels + tid] += 1;
            }
        }
    }
    return S.refused;
}

}  // extern "C"
