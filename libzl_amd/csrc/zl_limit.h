// zl_limit.h -- a clip's peaks on the device: the true-peak measurement (zlhip_sound_peak / _batch) and the
// look-ahead limiter that brings the few peaks of a clip under a ceiling and leaves everything else as it was, bit for bit, under the
// clip's own id (zlhip_sound_limit / _batch).  The reference has neither: a build-defined extension that claims no parity.  Shared by
// the HIP kernels (zl_limit.hip), the engine and a host build for the CPU tier (tests/cpu_harness/limit_host.cpp): everything is
// defined HERE, once.  All arithmetic is fp32, every operator one IEEE operation, nothing fused (the build never contracts).
//
//   Detector.  v = x gain, one rounded multiply (gain 1: v = x exactly); for the analysis a non-finite x is +0.  Sample peak of frame f,
//              channel c: |v[f][c]|.  Inter-sample peak ips[f][c], with ZL_LM_TRUE_PEAK: the oversampling factor F is 4 for a rate below
//              70000, 2 below 140000, else 1 (BS.1770-4 Annex 2); the filter is section 11's table unchanged, zl_rs_design for the
//              geometry fs = rate, ft = F rate (L = F, M = 1, 64 taps per phase), rows p = 1 .. F-1; phase p between the frames f and
//              f + 1 is y = sum over t of h[p][t] v[f - 31 + t] by zl_rs_tap in increasing t, v = +0 outside the request's region;
//              ips[f][c] = max over p of |y|, ips[-1] = 0; with F = 1 it is 0.  Frame detector p[f] = max over the channels of
//              max(|v[f]|, ips[f - 1], ips[f]) -- linked stereo; without the flag max over c of |v[f][c]|.  Maxima compare the bits of
//              |.|, so every reduction order gives the same answer.
//   Analysis.  One record per chunk of ZL_LM_CHUNK frames of the request's region: { sample_peak[2], inter_peak[2] }, maxima over the
//              chunk's own frames; a mono clip leaves index 1 zero.  The host takes the maxima; true_peak = max(sample_peak, inter_peak).
//   Limiter.   Over the slot's ORIGINAL data, the whole clip, n frames, with look-ahead L, hold H, ceiling c (zl_lm_resolve, the only
//              place the defaults and the limits are written):
//              1. g[f] = p[f] > c ? c / p[f] : 1, r[f] = 1 - g[f]: the limiter works on the REDUCTION, so that a region with nothing
//                 above the ceiling has r = 0, R = 0, G = 1 exactly and is copied bit for bit.
//              2. mr[i] = max r[j] over j in [max(i - H, 0), min(i + L, n - 1)], for i in [-L, n - 1].
//              3. R[f] = sum over k = 0 .. L of w[k] mr[f - k], from +0 in increasing k, every tap one rounded multiply, then one
//                 rounded add.  w (zl_lm_design) is parabolic and made from integers: w[k] = (double)((k + 1)(L + 1 - k)) / (double)S,
//                 S = (L + 1)(L + 2)(L + 3) / 6 in int64: one double division, rounded to fp32.  No libm.
//              4. G[f] = max(1 - R[f], 0).
//              5. y = v G[f] per channel; out = y > c ? c : (y < -c ? -c : y): comparisons, so that a NaN passes through to the
//                 verdict.  The clamp makes the guarantee exact -- no output sample exceeds c -- and moves a sample by at most
//                 |v| (L + 4) 2^-23 (w's rounding, L + 1 rounded products and L rounded adds on R, the roundings of g, r, G and y).
//              Offline: the look-ahead is taken from the data, the output is not delayed and keeps its length, channels and rate.
//   Identity.  gain == 1 and the clip's detector maximum <= c: applied = 0, no extent, no render.  gain != 1 and nothing hot:
//              applied = 1, every sample is x gain.
//   Finite.    The clip must have ZL_SOUND_FINITE (the limiter needs a finite detector); it stays set iff every written sample is
//              finite.
//
// The work.  Detecting (the analysis, and the limiter's first pass): workgroups are numbered over the call, each takes one chunk of one
// request (bisection over wg_base), reads the arena's 16-byte groups with head and tail masked by float index (zl_ov_groups,
// zl_ov_valid), with the flag stages the chunk and its taps' frames (31 before, 32 behind) in LDS and runs the F - 1 phase rows from
// there, and one lane writes the chunk's record.  Rendering: a workgroup is one TILE of ZL_LM_TILE output frames of one job, a lane
// ZL_LM_PER consecutive frames = one (mono) or two (stereo) 16-byte groups, the same groups of source and destination.  The tile reads
// the chunk records that cover its reach (zl_lm_tile_reach); none above c: the tile is COLD, a device copy with one multiply.  Else
// it recomputes r over its reach into LDS, forms mr by log-step doubling (max over [q, q + 2^k) in place, then two overlapping
// windows), stores mr transposed by 4 (zl_lm_mr_pos) so that a lane's window slides over consecutive words -- one LDS read per tap
// for four frames -- and applies.  Barriers sit outside divergent code; every trip count is the job's, uniform over the workgroup.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "zl_overview.h"
#include "zl_resample.h"
#include "zl_types.h"

#define ZL_LM_TRUE_PEAK     1
#define ZL_LM_CHUNK         1024            // frames of a detector chunk: one record, one detecting workgroup
#define ZL_LM_TILE          1024            // output frames of a render workgroup
#define ZL_LM_WG            256             // lanes of both kernels
#define ZL_LM_PER           4               // consecutive frames of a lane of a tile (ZL_LM_TILE / ZL_LM_WG)
#define ZL_LM_MAX_L         512
#define ZL_LM_MAX_H         512
#define ZL_LM_HALF          32              // the filter's frames a side (ZL_RS_BASE_HALF): tap 31 sits on frame f
#define ZL_LM_TAPS          64
#define ZL_LM_PAD           8               // zero frames behind a clip (ZL_ST_PAD, zl_stretch.h)
#define ZL_LM_CEILING       ((float)0.8912509381337456)      // -1 dBFS
#define ZL_LM_MAX_REACH     (ZL_LM_TILE + 2 * ZL_LM_MAX_L + ZL_LM_MAX_H)   // frames of r a tile needs at most
#define ZL_LM_MAX_MR        (ZL_LM_TILE + ZL_LM_MAX_L)                     // values of mr a tile needs at most
#define ZL_LM_MR_Q          400             // stride of the transposed mr: >= ZL_LM_MAX_MR / 4, and 16 modulo 64 (the four writers of a row hit four banks)
#define ZL_LM_STAGE         (ZL_LM_MAX_REACH + ZL_LM_TAPS)                 // frames of v a hot true-peak tile stages
#define ZL_LM_DET_STAGE     (ZL_LM_CHUNK + ZL_LM_TAPS - 1)                 // frames of v a detecting workgroup stages
#define ZL_LM_TABLE_FLOATS  (4 * ZL_LM_TAPS + 2 * ZL_LM_TAPS)              // the two filter tables of a call: F = 4, then F = 2
#define ZL_LM_MAX_CALL_CHUNKS 4194304       // chunk records of one call

// The requests as the header sees them (zlhip_limit_request's and zlhip_peak_request's layouts, include/zlhip.h)
struct ZlLmRequest { int32_t id, flags, lookahead_frames, hold_frames; float ceiling, gain; };
struct ZlLmPeakRequest { int32_t id, first_frame, num_frames, flags; };
struct ZlLmRecord { float sample_peak[2], inter_peak[2]; };

ZL_HD inline uint32_t zl_lm_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
ZL_HD inline float zl_lm_float(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
ZL_HD inline uint32_t zl_lm_abs_bits(float v) { return zl_lm_bits(v) & 0x7fffffffu; }
ZL_HD inline bool zl_lm_finite(float v) { return (zl_lm_bits(v) & 0x7f800000u) != 0x7f800000u; }

inline int32_t zl_lm_oversampling(double rate) { return rate < 70000.0 ? 4 : (rate < 140000.0 ? 2 : 1); }
// the table of factor F inside a call's tables (F = 4: [4][64], F = 2: [2][64]); row p at + p * ZL_LM_TAPS
ZL_HD inline int32_t zl_lm_table_at(int32_t F) { return F == 4 ? 0 : 4 * ZL_LM_TAPS; }
// is the rate one the flag can be asked at?  (section 11's limits)
inline int zl_lm_rate_ok(double rate) { ZlRsGeom g; return zl_rs_geometry(rate, rate * (double)zl_lm_oversampling(rate), &g) == 0 && g.taps == ZL_LM_TAPS && g.M == 1; }
// a call's two tables: section 11's design, unchanged (the geometry depends on F alone)
inline void zl_lm_tables(float *t)
{
    ZlRsGeom g;
    g.M = 1; g.half = ZL_LM_HALF; g.taps = ZL_LM_TAPS; g.row = ZL_LM_TAPS;
    g.L = 4; zl_rs_design(g, t + zl_lm_table_at(4));
    g.L = 2; zl_rs_design(g, t + zl_lm_table_at(2));
}

// the defaults and the limits of the limiter; the only place they are written.  0 = valid (every field filled in), -1 = not
inline int zl_lm_resolve(double rate, ZlLmRequest *q)
{
    if (q->flags & ~ZL_LM_TRUE_PEAK) return -1;
    if ((q->flags & ZL_LM_TRUE_PEAK) && !zl_lm_rate_ok(rate)) return -1;
    if (!(q->ceiling == 0.0f || (q->ceiling > 0.0f && q->ceiling <= 1.0f))) return -1;                    // (a NaN fails here)
    if (!(q->gain == 0.0f || (q->gain > 0.0f && q->gain <= 3.402823466e38f))) return -1;
    if (q->lookahead_frames < 0 || q->lookahead_frames > ZL_LM_MAX_L || q->hold_frames < 0 || q->hold_frames > ZL_LM_MAX_H) return -1;
    if (q->lookahead_frames == 0) {
        const double v = floor(rate * 0.005 + 0.5);
        q->lookahead_frames = !(v >= 1.0) ? 1 : (v > (double)ZL_LM_MAX_L ? ZL_LM_MAX_L : (int32_t)v);
    }
    if (q->ceiling == 0.0f) q->ceiling = ZL_LM_CEILING;
    if (q->gain == 0.0f) q->gain = 1.0f;
    return 0;
}
// the limits of the analysis
inline int zl_lm_peak_resolve(double rate, int32_t length, const ZlLmPeakRequest *q)
{
    if (q->flags & ~ZL_LM_TRUE_PEAK) return -1;
    if ((q->flags & ZL_LM_TRUE_PEAK) && !zl_lm_rate_ok(rate)) return -1;
    if (q->first_frame < 0 || q->num_frames < 1 || (int64_t)q->first_frame + q->num_frames > length) return -1;
    return 0;
}

// the window: L + 1 weights
inline void zl_lm_design(int32_t L, float *w)
{
    const int64_t S = ((int64_t)L + 1) * ((int64_t)L + 2) * ((int64_t)L + 3) / 6;
    for (int32_t k = 0; k <= L; ++k) w[k] = (float)((double)(((int64_t)k + 1) * ((int64_t)L + 1 - k)) / (double)S);
}

// ---- the detector ----------------------------------------------------------------------------------------------------------------
ZL_HD inline float zl_lm_v(float x, float gain, int32_t sanitize) { if (sanitize && !zl_lm_finite(x)) x = 0.0f; return x * gain; }
// |ips| of one channel as bits: win[t] = v[f - 31 + t], t in [0, 64); table: the F rows
ZL_HD inline uint32_t zl_lm_ips_bits(const float *table, int32_t F, const float *win)
{
    uint32_t m = 0u;
    for (int32_t p = 1; p < F; ++p) {
        const float *h = table + p * ZL_LM_TAPS;
        float acc = 0.0f;
        for (int32_t t = 0; t < ZL_LM_TAPS; ++t) acc = zl_rs_tap(acc, h[t], win[t]);
        const uint32_t b = zl_lm_abs_bits(acc);
        m = b > m ? b : m;
    }
    return m;
}
ZL_HD inline uint32_t zl_lm_max_bits(uint32_t a, uint32_t b) { return a > b ? a : b; }
// step 1, from the detector's bits
ZL_HD inline float zl_lm_reduction(uint32_t p_bits, float c) { const float p = zl_lm_float(p_bits); const float g = p > c ? c / p : 1.0f; return 1.0f - g; }
// step 4
ZL_HD inline float zl_lm_gain_of(float R) { const float G = 1.0f - R; return G < 0.0f ? 0.0f : G; }
// step 5
ZL_HD inline float zl_lm_apply(float v, float G, float c) { const float y = v * G; return y > c ? c : (y < -c ? -c : y); }

// One request of a detecting call as the kernel sees it (built by the host)
struct ZlLmScan {
    uint64_t src;                // device address of the extent (16-byte aligned)
    int32_t  channels, a, b;     // 1 or 2; the region
    int32_t  wg_base;            // the request's first workgroup = its first record in the call
    int32_t  F;                  // the oversampling factor; 1: no inter-sample peak
    int32_t  sanitize;           // a non-finite x is +0 (the analysis)
    float    gain;
    int32_t  pad;
};
ZL_HD inline int32_t zl_lm_chunks(int32_t frames) { return (frames + ZL_LM_CHUNK - 1) / ZL_LM_CHUNK; }
// chunk k of the region covers [*lo, *hi); with F > 1 the workgroup stages [*s0, *s1), LDS index 0 is frame *lo - 31
ZL_HD inline void zl_lm_chunk(const ZlLmScan &S, int32_t k, int32_t *lo, int32_t *hi, int32_t *s0, int32_t *s1)
{
    *lo = S.a + k * ZL_LM_CHUNK;
    *hi = S.b - *lo > ZL_LM_CHUNK ? *lo + ZL_LM_CHUNK : S.b;
    *s0 = *lo; *s1 = *hi;
    if (S.F > 1) {
        *s0 = *lo - (ZL_LM_HALF - 1) > S.a ? *lo - (ZL_LM_HALF - 1) : S.a;
        *s1 = S.b - *hi > ZL_LM_HALF ? *hi + ZL_LM_HALF : S.b;
    }
}

// ---- the render --------------------------------------------------------------------------------------------------------------------
// One applied request of a call as the render kernel sees it (built by the host)
struct ZlLmJob {
    uint64_t src, dst;           // device addresses of the original and of the new extent (16-byte aligned)
    int32_t  channels, n;        // 1 or 2; frames; of both
    int32_t  L, H, F;            // look-ahead, hold, oversampling factor (1: the detector is the sample peak)
    float    ceiling, gain;
    int32_t  wg_base;            // the job's first render workgroup in the call
    int32_t  rec_base;           // the clip's first chunk record among the call's
    int32_t  weights;            // the job's first weight among the call's
    int32_t  verdict;            // the job's word among the call's verdicts, and its ZlLmStats
    int32_t  pad;
};
struct ZlLmStats { uint32_t frames_reduced, min_gain_bits; };      // 0 and the bits of 1.0f before the launch

ZL_HD inline int64_t zl_lm_extent_floats(int64_t length, int32_t channels) { return ((length + ZL_LM_PAD) * channels + 3) & ~(int64_t)3; }
ZL_HD inline int64_t zl_lm_groups(const ZlLmJob &J) { return zl_lm_extent_floats(J.n, J.channels) >> 2; }
ZL_HD inline int32_t zl_lm_tile_groups(int32_t channels) { return ZL_LM_TILE * channels / 4; }
// tiles of a job: as many as cover every group of the extent (the last may hold the zero frames alone)
ZL_HD inline int32_t zl_lm_job_tiles(const ZlLmJob &J) { return (int32_t)((zl_lm_groups(J) + zl_lm_tile_groups(J.channels) - 1) / zl_lm_tile_groups(J.channels)); }
ZL_HD inline int32_t zl_lm_reach_frames(const ZlLmJob &J) { return ZL_LM_TILE + 2 * J.L + J.H; }          // of r; index 0 is frame t0 - L - H
ZL_HD inline int32_t zl_lm_mr_count(const ZlLmJob &J) { return ZL_LM_TILE + J.L; }                        // of mr; index 0 is frame t0 - L
ZL_HD inline int32_t zl_lm_mr_pos(int32_t m) { return (m & 3) * ZL_LM_MR_Q + (m >> 2); }
// the largest power of two <= W (W >= 1)
ZL_HD inline int32_t zl_lm_pow2(int32_t W) { int32_t P = 1; while (2 * P <= W) P *= 2; return P; }
// the frames whose detector decides anything in the tile at t0: [*lo, *hi], clipped to the clip; 0 where the tile holds no frame
ZL_HD inline int zl_lm_tile_reach(const ZlLmJob &J, int32_t t0, int32_t *lo, int32_t *hi)
{
    if (t0 >= J.n) return 0;
    const int32_t a = t0 - J.L - J.H - (J.F > 1 ? 1 : 0), b = t0 + ZL_LM_TILE - 1 + J.L;
    *lo = a > 0 ? a : 0;
    *hi = b < J.n - 1 ? b : J.n - 1;
    return 1;
}
ZL_HD inline uint32_t zl_lm_record_bits(const ZlLmRecord &r)
{
    return zl_lm_max_bits(zl_lm_max_bits(zl_lm_bits(r.sample_peak[0]), zl_lm_bits(r.sample_peak[1])), zl_lm_max_bits(zl_lm_bits(r.inter_peak[0]), zl_lm_bits(r.inter_peak[1])));
}
// is the tile cold: no record of a chunk its reach touches above c (as bits: a NaN record is above).  recs: the clip's records
ZL_HD inline bool zl_lm_tile_cold(const ZlLmJob &J, const ZlLmRecord *recs, int32_t t0)
{
    int32_t lo, hi;
    if (!zl_lm_tile_reach(J, t0, &lo, &hi)) return true;
    const uint32_t c = zl_lm_bits(J.ceiling);
    bool cold = true;
    for (int32_t k = lo / ZL_LM_CHUNK; k <= hi / ZL_LM_CHUNK; ++k) cold = cold && !(zl_lm_record_bits(recs[k]) > c);
    return cold;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_limit.hip; 0 or a hipError_t value).  tables: ZL_LM_TABLE_FLOATS floats; records [wgs of the detecting call];
// weights: the call's windows; stats, verdicts [njobs]
int zl_launch_limit_detect(const ZlLmScan *reqs, int32_t nreq, int32_t wgs, const float *tables, ZlLmRecord *records, hipStream_t s);
int zl_launch_limit_render(const ZlLmJob *jobs, int32_t njobs, int32_t wgs, const float *tables, const ZlLmRecord *records, const float *weights,
                           ZlLmStats *stats, uint32_t *verdicts, hipStream_t s);
#endif
