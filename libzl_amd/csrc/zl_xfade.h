// zl_xfade.h -- a loop crossfade baked into a clip's data on the device (zlhip_sound_loop_crossfade / _batch):
// the loop finder (zl_loop.h) only chooses among points that exist; a decaying pad or a loop placed by ear still jumps from
// x[stop - 1] to x[start] on every lap.  Here the X frames in front of the loop's stop are faded into the X frames in front of its
// start, so that the wrap stop - 1 -> start is the original's own step start - 1 -> start.  The reference has no loop crossfade: a
// build-defined extension that claims no parity.  Shared by the HIP kernels (zl_xfade.hip), the engine and a host build for the CPU
// tier (tests/cpu_harness/xfade_host.cpp): everything is defined HERE, once.
//
// A request is (sound, start_frame s, stop_frame e, fade_frames X, curve) over the slot's ORIGINAL extent of `length` frames;
// 0 <= s < e <= length, e exclusive (the voice wraps when its position reaches the stop).
//
//   Resolve.     (zl_xf_resolve, the only place the default is written) X given as 0: min(rint(0.020 rate), s, e - s, 65536); where that is
//                0 (a loop from frame 0 has no lead-in) the request resolves with applied = 0, which is no error: the clip is left
//                alone.  An explicit X: 1 <= X <= min(s, e - s, 65536).  X <= e - s keeps the regions B = [s - X, s) and A = [e - X, e)
//                disjoint.  curve: ZL_XF_AUTO (0), ZL_XF_LINEAR (rho = 1), ZL_XF_EQUAL_POWER (rho = 0).
//   Correlation. always measured, exact: m[f] = the sum over the channels of zl_st_q(v) (zl_pitch.h; NaN -> 0, |m| <= 65534);
//                Sab = the sum over i in [0, X) of m[e - X + i] m[s - X + i], Saa and Sbb likewise, in int64: at most
//                65536 * 65534^2 < 2^49, so every reduction order gives the same integers.  Finish (zl_xf_finish; host, double, built
//                without contraction): corr = (Saa == 0 || Sbb == 0) ? 0 : Sab / sqrt(Saa * Sbb); rho = min(1, max(0, corr)).  Only *, /
//                and sqrt: correctly rounded everywhere, no libm call.
//   Weights.     (zl_xf_design; host, double, the order as written, then rounded to fp32) for i in [0, X): t = (i + 1) / X, u = 1 - t,
//                d = sqrt(((u u) + (t t)) + ((2 rho) (t u))), a[i] = (float)(u / d), b[i] = (float)(t / d).  a^2 + b^2 + 2 rho a b = 1:
//                the power of material of correlation rho stays constant through the fade.  rho = 1 is the linear fade, rho = 0 the
//                equal-power fade.  At i = X - 1: a = 0 and b = 1 exactly.
//   Output.      the new extent is the old one but for A: per channel, in fp32, y[e - X + i] = (a[i] x[e - X + i]) + (b[i] x[s - X + i]):
//                two rounded multiplies, then one rounded add, nothing fused.  Every other float is copied bit for bit; the arena's
//                layout stays: ZL_XF_PAD zero frames behind the data, zeros up to the 16-byte boundary (written, not copied).
//   Finite.      ZL_SOUND_FINITE stays set iff the original had it and every written fade sample is finite (a + b reaches 1.41 under
//                the equal-power curve: samples near FLT_MAX can overflow).
//
// The work.  A JOB is one applied request of a call.  Measuring: one workgroup per job walks the fade in chunks of ZL_XF_CHUNK frames;
// the chunk's two spans are read in the arena's 16-byte groups, head and tail masked by float index (zl_ov_groups, zl_pt_group_mix), so
// that no float outside the two regions is looked at.  Rendering: one lane per 16-byte group of the DESTINATION extent, a workgroup is
// ZL_XF_WG consecutive groups of one job, and the workgroups are numbered over the call (wg_base).  A group in front of the data's end
// loads its source group; a float behind the data's end is a produced +0; a float inside A (zl_xf_fades) is mixed with the float
// (e - s) channels lower (zl_xf_b_index: never below (s - X) channels >= 0) by the weights of its frame (zl_xf_weight_index).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "zl_pitch.h"
#include "zl_types.h"

#define ZL_XF_AUTO          0
#define ZL_XF_LINEAR        1
#define ZL_XF_EQUAL_POWER   2
#define ZL_XF_FADE_SECONDS  0.020
#define ZL_XF_MAX_FADE      65536
#define ZL_XF_PAD           8            // zero frames behind a clip (ZL_ST_PAD, zl_stretch.h)
#define ZL_XF_WG            256          // 16-byte groups of a render workgroup, one per lane; lanes of the measuring workgroup
#define ZL_XF_CHUNK         1024         // frames of the fade the measuring workgroup mixes at a time (two int32 arrays of LDS)

// the default and the limits; the only place they are written.  0 = valid (*X the frames to fade, 0: nothing to fade), -1 = not
inline int zl_xf_resolve(double sample_rate, int32_t length, int32_t s, int32_t e, int32_t *X, int32_t curve)
{
    if (!(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    if (s < 0 || e <= s || e > length) return -1;
    if (curve != ZL_XF_AUTO && curve != ZL_XF_LINEAR && curve != ZL_XF_EQUAL_POWER) return -1;
    int32_t most = s < e - s ? s : e - s;
    if (most > ZL_XF_MAX_FADE) most = ZL_XF_MAX_FADE;
    if (*X == 0) {
        const double d = rint(ZL_XF_FADE_SECONDS * sample_rate);
        *X = d < (double)most ? (int32_t)d : most;
        return 0;
    }
    return *X >= 1 && *X <= most ? 0 : -1;
}

// corr and rho from the three sums (one IEEE operation per operator: build without contraction)
inline void zl_xf_finish(int64_t sab, int64_t saa, int64_t sbb, double *corr, double *rho)
{
    const double c = (saa == 0 || sbb == 0) ? 0.0 : (double)sab / sqrt((double)saa * (double)sbb);
    *corr = c;
    *rho = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
}

// the rho a curve fades with: the measured one, or the curve's own
inline double zl_xf_curve_rho(int32_t curve, double measured) { return curve == ZL_XF_LINEAR ? 1.0 : (curve == ZL_XF_EQUAL_POWER ? 0.0 : measured); }

// the table: X pairs (a, b)
inline void zl_xf_design(int32_t X, double rho, float *ab)
{
    for (int32_t i = 0; i < X; ++i) {
        const double t = (double)(i + 1) / (double)X, u = 1.0 - t;
        const double uu = u * u, tt = t * t, tu = t * u, r2 = 2.0 * rho;
        const double sq = uu + tt, cross = r2 * tu;
        const double d = sqrt(sq + cross);
        ab[2 * i] = (float)(u / d);
        ab[2 * i + 1] = (float)(t / d);
    }
}

// One applied request of a call as the kernels see it (built by the host)
struct ZlXfJob {
    uint64_t src, dst;           // device addresses of the original and of the new extent (16-byte aligned)
    int32_t  length, channels;   // frames, 1 or 2; of both
    int32_t  s, e, X;            // the loop and the frames to fade: 1 <= X <= min(s, e - s)
    int32_t  wg_base;            // the job's first render workgroup in the call
    int32_t  weights;            // the job's first (a, b) pair in the call's weight buffer
    int32_t  verdict;            // the clip's word among the call's verdicts (set when a written fade sample is not finite)
};

// what the measuring kernel leaves per job
struct ZlXfSums { int64_t sab, saa, sbb; };

// floats and groups of an extent (zl_extent_floats, zl_arena.h)
ZL_HD inline int64_t zl_xf_extent_floats(int64_t length, int32_t channels) { return ((length + ZL_XF_PAD) * channels + 3) & ~(int64_t)3; }
ZL_HD inline int64_t zl_xf_groups(const ZlXfJob &J) { return zl_xf_extent_floats(J.length, J.channels) >> 2; }
ZL_HD inline int32_t zl_xf_job_wgs(const ZlXfJob &J) { return (int32_t)((zl_xf_groups(J) + ZL_XF_WG - 1) / ZL_XF_WG); }
// the floats of the data, of the fade region A
ZL_HD inline int64_t zl_xf_data_floats(const ZlXfJob &J) { return (int64_t)J.length * J.channels; }
ZL_HD inline int64_t zl_xf_a_first(const ZlXfJob &J) { return (int64_t)(J.e - J.X) * J.channels; }
ZL_HD inline int64_t zl_xf_a_end(const ZlXfJob &J) { return (int64_t)J.e * J.channels; }
// does group g hold a float of the source's data (it is loaded), a float of A (it fades)?
ZL_HD inline bool zl_xf_group_loads(const ZlXfJob &J, int64_t g) { return 4 * g < zl_xf_data_floats(J); }
ZL_HD inline bool zl_xf_group_fades(const ZlXfJob &J, int64_t g) { return 4 * g + 4 > zl_xf_a_first(J) && 4 * g < zl_xf_a_end(J); }
// float k of the extent: is it one of A's; the float of B it is mixed with; the pair of its frame
ZL_HD inline bool zl_xf_fades(const ZlXfJob &J, int64_t k) { return k >= zl_xf_a_first(J) && k < zl_xf_a_end(J); }
ZL_HD inline int64_t zl_xf_b_index(const ZlXfJob &J, int64_t k) { return k - (int64_t)(J.e - J.s) * J.channels; }
ZL_HD inline int32_t zl_xf_weight_index(const ZlXfJob &J, int64_t k) { const int64_t d = k - zl_xf_a_first(J); return (int32_t)(J.channels == 2 ? d >> 1 : d); }
// one faded sample: two rounded multiplies, one rounded add (the build never contracts them)
ZL_HD inline float zl_xf_mix(float a, float b, float xa, float xb) { const float p = a * xa; const float q = b * xb; return p + q; }
ZL_HD inline bool zl_xf_finite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// measuring: chunk c of the fade covers its frames [*i0, *i1), i counted from the regions' first frames
ZL_HD inline int32_t zl_xf_chunks(int32_t X) { return (X + ZL_XF_CHUNK - 1) / ZL_XF_CHUNK; }
ZL_HD inline void zl_xf_chunk(int32_t X, int32_t c, int32_t *i0, int32_t *i1)
{
    *i0 = c * ZL_XF_CHUNK;
    *i1 = *i0 + ZL_XF_CHUNK < X ? *i0 + ZL_XF_CHUNK : X;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_xfade.hip; 0 or a hipError_t value).  sums [njobs] may be host memory mapped into the device; weights: the call's
// (a, b) pairs; verdicts [njobs]
int zl_launch_xfade_measure(const ZlXfJob *jobs, int32_t njobs, ZlXfSums *sums, hipStream_t s);
int zl_launch_xfade_render(const ZlXfJob *jobs, int32_t njobs, int32_t wgs, const float *weights, uint32_t *verdicts, hipStream_t s);
#endif
