// zl_resample.h -- clips converted to another sample rate on the device (zlhip_sound_convert_rate / _batch):
// a band-limited rational resampler, so that a bank recorded at a foreign rate (44.1 kHz in a 48 kHz session) plays as a unit-step,
// integer-position source -- K2's on-grid form -- instead of through the pitched voice path.  Shared by the HIP kernels
// (zl_resample.hip), the engine and a host build for the CPU tier (tests/cpu_harness/resample_host.cpp): the ratio, the filter, the
// number of output frames, which input frames a workgroup stages and what one lane adds up are defined HERE, once.
//
//   Ratio.   Source rate fs and target rate ft are integer-valued doubles in [1000, 768000]; g = gcd(fs, ft), L = ft / g, M = fs / g.
//   Filter.  A Kaiser-windowed sinc, polyphase, one row per phase: s = min(1, L/M), half = ceil(32 / s) input frames a side,
//            T = 2 half taps, c = 0.95 s, beta = 10.  For phase p in [0, L) and tap t in [0, T): d = (t - half + 1) - p/L,
//            h = c sinc(c d) I0(beta sqrt(1 - (d/half)^2)) / I0(beta), 0 where |d| >= half; sinc(x) = sin(pi x) / (pi x).  All in
//            double on the host; every row is divided by its own sum in double, then rounded to fp32.  I0 is the power series, summed
//            until a term is below 1e-17 of the sum.  Rows are stored padded to a multiple of 4 floats, zeros in the pad.
//   Limits.  L <= 2048, M <= 8 L (so T <= 512), L * padded T <= 262144 floats, N + 8 <= INT32_MAX.
//   Output.  N = (len L + M - 1) / M frames (int64).  Frame j: q = j M (int64), i = q / L, p = q mod L,
//            y[j] = sum over t = 0 .. T-1 of h[p][t] * x[i - half + 1 + t], x = +0 outside [0, len); per channel in fp32, acc starts
//            at +0, every tap is one rounded multiply, then one rounded add, in increasing t.  Nothing is fused.
//   Extent.  The arena's layout: interleaved or mono, ZL_RS_PAD zero frames behind, zeros up to the 16-byte boundary.
//
// The work.  A JOB is one clip of the call; a workgroup takes ZL_RS_WG consecutive output frames of one job, one per lane, and the
// workgroups are numbered over the call (wg_base).  The workgroup stages the input frames its lanes read -- zl_rs_span -- masked by
// frame index: a frame outside [0, len) is a produced +0, no address outside the clip's frames is ever formed.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <math.h>

#include "zl_types.h"

#define ZL_RS_PAD          8            // zero frames behind a clip (ZL_ST_PAD, zl_stretch.h)
#define ZL_RS_WG           256          // output frames of a workgroup, one per lane
#define ZL_RS_MIN_RATE     1000.0
#define ZL_RS_MAX_RATE     768000.0
#define ZL_RS_MAX_L        2048
#define ZL_RS_MAX_DOWN     8            // M <= 8 L
#define ZL_RS_MAX_TAPS     512
#define ZL_RS_MAX_TABLE    262144       // floats of one table
#define ZL_RS_BASE_HALF    32           // input frames a side at s = 1
#define ZL_RS_CUTOFF       0.95
#define ZL_RS_BETA         10.0
// input frames a workgroup stages at most: its lanes' first taps span at most (ZL_RS_WG - 1) * ZL_RS_MAX_DOWN frames, plus the taps
#define ZL_RS_STAGE_FRAMES ((ZL_RS_WG - 1) * ZL_RS_MAX_DOWN + ZL_RS_MAX_TAPS + 1)

struct ZlRsGeom {
    int32_t L, M;                // output frames per M input frames
    int32_t half, taps;          // taps = 2 * half
    int32_t row;                 // floats of a table row: taps rounded up to a multiple of 4
};

// 0 = valid (g filled), -1 = a rate that is no integer in [1000, 768000] or a ratio beyond the limits
inline int zl_rs_geometry(double fs, double ft, ZlRsGeom *g)
{
    if (!(fs >= ZL_RS_MIN_RATE && fs <= ZL_RS_MAX_RATE && ft >= ZL_RS_MIN_RATE && ft <= ZL_RS_MAX_RATE)) return -1;
    if (fs != floor(fs) || ft != floor(ft)) return -1;
    int64_t a = (int64_t)fs, b = (int64_t)ft;
    while (b != 0) { const int64_t r = a % b; a = b; b = r; }
    const int64_t L = (int64_t)ft / a, M = (int64_t)fs / a;
    if (L > ZL_RS_MAX_L || M > ZL_RS_MAX_DOWN * L) return -1;
    const int64_t half = L >= M ? ZL_RS_BASE_HALF : (ZL_RS_BASE_HALF * M + L - 1) / L;      // ceil(32 / s), in integers
    const int64_t taps = 2 * half, row = (taps + 3) & ~(int64_t)3;
    if (taps > ZL_RS_MAX_TAPS || L * row > ZL_RS_MAX_TABLE) return -1;
    g->L = (int32_t)L; g->M = (int32_t)M; g->half = (int32_t)half; g->taps = (int32_t)taps; g->row = (int32_t)row;
    return 0;
}

// output frames of a clip of `len` frames; 0 where N + ZL_RS_PAD does not fit an int32
inline int64_t zl_rs_out_frames(const ZlRsGeom &g, int64_t len)
{
    const int64_t N = (len * g.L + g.M - 1) / g.M;
    return N + ZL_RS_PAD <= (int64_t)INT32_MAX ? N : 0;
}

// I0 by its power series: sum of ((x/2)^k / k!)^2, until a term is below 1e-17 of the sum
inline double zl_rs_i0(double x)
{
    const double y = 0.25 * x * x;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// the table: [L][row] floats
inline void zl_rs_design(const ZlRsGeom &g, float *table)
{
    const double pi = 3.14159265358979323846;
    const double s = g.L >= g.M ? 1.0 : (double)g.L / (double)g.M;
    const double c = ZL_RS_CUTOFF * s, inv = 1.0 / zl_rs_i0(ZL_RS_BETA);
    double h[ZL_RS_MAX_TAPS];
    for (int32_t p = 0; p < g.L; ++p) {
        double sum = 0.0;
        for (int32_t t = 0; t < g.taps; ++t) {
            const double d = (double)(t - g.half + 1) - (double)p / (double)g.L;
            const double u = d / (double)g.half;
            double v = 0.0;
            if (fabs(d) < (double)g.half) {
                const double x = pi * c * d;
                const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
                v = c * sinc * zl_rs_i0(ZL_RS_BETA * sqrt(1.0 - u * u)) * inv;
            }
            h[t] = v;
            sum += v;
        }
        float *row = table + (size_t)p * (size_t)g.row;
        for (int32_t t = 0; t < g.taps; ++t) row[t] = (float)(h[t] / sum);
        for (int32_t t = g.taps; t < g.row; ++t) row[t] = 0.0f;
    }
}

// One clip of a call as the kernel sees it (built by the host)
struct ZlRsJob {
    uint64_t src, dst;           // device addresses of the source's and the converted extent (16-byte aligned)
    uint64_t table;              // device address of the job's filter table [L][row]
    int32_t  len, N;             // frames of the source, of the result
    int32_t  channels;           // 1 or 2, of both
    int32_t  L, M, half, taps, row;
    int32_t  wg_base;            // the job's first workgroup in the call
    int32_t  verdict;            // the clip's word among the call's verdicts (set when an output sample is not finite)
};

ZL_HD inline int32_t zl_rs_job_wgs(int32_t N) { return (N + ZL_RS_WG - 1) / ZL_RS_WG; }
// floats of the converted extent (zl_extent_floats, zl_arena.h)
ZL_HD inline uint64_t zl_rs_extent_floats(int64_t N, int channels) { return (((uint64_t)N + ZL_RS_PAD) * (uint64_t)channels + 3u) & ~(uint64_t)3; }

// output frame j: the input frame its tap `half - 1` sits on, and its phase
ZL_HD inline void zl_rs_position(const ZlRsJob &J, int64_t j, int64_t *i, int32_t *p)
{
    const int64_t q = j * (int64_t)J.M;
    *i = q / (int64_t)J.L;
    *p = (int32_t)(q - *i * (int64_t)J.L);
}

// the input frames workgroup w of the job stages: [*first, *first + *count), the taps of its frames [j0, j1]; frame numbers may lie
// outside [0, len).  count <= ZL_RS_STAGE_FRAMES
ZL_HD inline void zl_rs_span(const ZlRsJob &J, int32_t w, int64_t *first, int32_t *count)
{
    const int64_t j0 = (int64_t)w * ZL_RS_WG;
    const int64_t j1 = (j0 + ZL_RS_WG <= (int64_t)J.N ? j0 + ZL_RS_WG : (int64_t)J.N) - 1;
    int64_t i0, i1; int32_t p;
    zl_rs_position(J, j0, &i0, &p);
    zl_rs_position(J, j1, &i1, &p);
    *first = i0 - J.half + 1;
    *count = (int32_t)(i1 - i0) + J.taps;
}

// the mask of the staging: is input frame f one of the clip's?  (a frame that is not is staged as +0 and its address never formed)
ZL_HD inline bool zl_rs_in_clip(const ZlRsJob &J, int64_t f) { return f >= 0 && f < (int64_t)J.len; }

// one tap: a rounded multiply, then a rounded add (the build never contracts them)
ZL_HD inline float zl_rs_tap(float acc, float h, float x) { const float m = h * x; return acc + m; }

ZL_HD inline bool zl_rs_finite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// floats behind the last frame that the job's last workgroup zeroes: [N * channels, extent floats), at most 8 * 2 + 3
ZL_HD inline int32_t zl_rs_tail_floats(const ZlRsJob &J) { return (int32_t)(zl_rs_extent_floats(J.N, J.channels) - (uint64_t)J.N * (uint64_t)J.channels); }

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// One entry of the sound table a call publishes: ZL_SOUND_FINITE from the clip's verdict word
struct ZlRsPublish { ZlSound s; int32_t id, verdict; };
// launchers (zl_resample.hip; 0 or a hipError_t value)
int zl_launch_resample(const ZlRsJob *jobs, int32_t njobs, int32_t wgs, uint32_t *verdicts, hipStream_t s);
int zl_launch_resample_publish(const ZlRsPublish *recs, int32_t n, const uint32_t *verdicts, ZlSound *table, hipStream_t s);
#endif
