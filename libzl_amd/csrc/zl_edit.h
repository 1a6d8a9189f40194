// zl_edit.h -- a clip's data edited on the device under the clip's own id (zlhip_sound_edit / _batch): crop to a
// region, trim the silence off both ends, reverse, fade the ends.  The reference has no such edit: a build-defined extension that claims
// no parity.  Shared by the HIP kernels (zl_edit.hip), the engine and a host build for the CPU tier (tests/cpu_harness/edit_host.cpp):
// everything is defined HERE, once.
//
// A request is (sound, first_frame a, num_frames, flags, pre_roll_frames, hold_frames, fade_in_frames, fade_out_frames, curve,
// threshold) over the slot's ORIGINAL extent of `length` frames.
//
//   Resolve.  (zl_ed_resolve, the only place the defaults and the limits are written) the region to keep is [a, b): num_frames 0 means
//             "to the end" (b = length, a < length), else 0 <= a, num_frames >= 1, a + num_frames <= length.  flags: ZL_ED_TRIM,
//             ZL_ED_REVERSE, no other bit.  threshold (fp32) 0: ZL_ED_THRESHOLD = 2^-10 (exact in fp32, about -60 dBFS), else finite and
//             above 0.  pre_roll_frames, hold_frames, fade_in_frames, fade_out_frames >= 0.  curve: ZL_ED_LINEAR, ZL_ED_SQRT, ZL_ED_SMOOTH.
//   Trim.     exact, no quantisation: frame f is LOUD iff for some channel !(fabsf(x[f][c]) < threshold) in fp32 (zl_ed_loud) -- NaN and
//             +-inf are loud, |x| == threshold is loud.  Over [a, b): F the smallest loud frame, Z the largest; integer min and max of
//             indices, so every reduction order gives the same answer.  No loud frame: silent = 1, applied = 0, the clip is untouched,
//             no error.  Else (zl_ed_region, int64) a' = max(a, F - pre_roll_frames), b' = min(b, Z + 1 + hold_frames).  Without
//             ZL_ED_TRIM a' = a and b' = b.  n = b' - a' >= 1.
//   Fades.    (zl_ed_fades) cut so that they never overlap: Xi = min(fade_in_frames, n / 2), Xo = min(fade_out_frames, n / 2), integer
//             division.  Weights (zl_ed_design; host, double, the order as written, then rounded to fp32): for i in [0, X): t = i / X;
//             LINEAR w = t; SQRT w = sqrt(t) (two clips faded against each other keep constant power); SMOOTH w = (t t) (3 - (2 t)).
//             Only *, /, - and sqrt: correctly rounded everywhere, no libm call, built without contraction.  w[0] = 0 exactly.
//   Output.   the new extent has n frames, the original's channels and rate.  Output frame i takes source frame b' - 1 - i with
//             ZL_ED_REVERSE and a' + i without; channels stay in place.  A frame i < Xi is multiplied by w_in[i], a frame i >= n - Xo by
//             w_out[n - 1 - i]: one rounded fp32 multiply per sample, and no frame gets both.  Every other float is copied bit for bit:
//             the fades act on the data after the reversal.  The arena's layout stays: ZL_ED_PAD zero frames behind the data, zeros up
//             to the 16-byte boundary (written, not copied).
//   Identity. (zl_ed_identity) a' = 0, n = length, no ZL_ED_REVERSE, Xi = Xo = 0: applied = 0, no extent, no launch copies it.  A trim
//             that finds nothing to cut is such a request.
//   Finite.   ZL_SOUND_FINITE stays set iff the original had it and every written FADED sample is finite.  A clip without the flag never
//             gains it, even when its non-finite samples were cropped away: the copied samples are not looked at (ZlClipSwap's rule,
//             zl_clip_calls.cpp: the verdict word of a clip whose original lacks the flag starts set).
//
// The work.  Scanning (the call's ZL_ED_TRIM requests only): workgroups cover a request's region in chunks of ZL_ED_CHUNK frames,
// numbered over the call (wg_base); a chunk's span is read in the arena's 16-byte groups, head and tail masked by float index
// (zl_ov_groups, zl_ov_valid), so that no float outside [a, b) decides anything; min and max loud frame per lane, wave, workgroup, then
// one atomic min and one atomic max into the request's two words (ZlEdFound; the host's copy starts them as INT32_MAX and -1).
// Rendering: a JOB is one applied request; one lane per 16-byte group of the DESTINATION extent, a workgroup is ZL_ED_WG consecutive
// groups of one job, numbered over the call.  A group that lies wholly inside the data (zl_ed_group_full) takes its four floats from four
// consecutive source floats that start at zl_ed_group_first -- at any dword offset of a source group -- in the order zl_ed_lane gives
// (forward as they are; reversed mono all four turned round, reversed stereo the two frames swapped as pairs).  The one group of a job
// that the data's end cuts takes its floats one by one (zl_ed_src_index); floats behind the data are produced +0.  No load touches a
// float outside [a' channels, b' channels) of the source.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "zl_overview.h"
#include "zl_types.h"

#define ZL_ED_TRIM          1
#define ZL_ED_REVERSE       2
#define ZL_ED_LINEAR        0
#define ZL_ED_SQRT          1
#define ZL_ED_SMOOTH        2
#define ZL_ED_THRESHOLD     0.0009765625f   // 2^-10
#define ZL_ED_PAD           8               // zero frames behind a clip (ZL_ST_PAD, zl_stretch.h)
#define ZL_ED_WG            256             // 16-byte groups of a render workgroup, one per lane; lanes of a scanning workgroup
#define ZL_ED_CHUNK         2048            // frames of a region one scanning workgroup reads

// The request as the header sees it (zlhip_edit_request's layout, include/zlhip.h)
struct ZlEdRequest { int32_t id, first_frame, num_frames, flags, pre_roll_frames, hold_frames, fade_in_frames, fade_out_frames, curve; float threshold; };

// the defaults and the limits; the only place they are written.  0 = valid (num_frames and threshold filled in), -1 = not
inline int zl_ed_resolve(int32_t length, ZlEdRequest *q)
{
    if (length < 1 || q->first_frame < 0 || q->num_frames < 0) return -1;
    if (q->num_frames == 0 ? q->first_frame >= length : (int64_t)q->first_frame + q->num_frames > length) return -1;
    if (q->flags & ~(ZL_ED_TRIM | ZL_ED_REVERSE)) return -1;
    if (!(q->threshold == 0.0f || (q->threshold > 0.0f && q->threshold <= 3.402823466e38f))) return -1;      // (a NaN fails here)
    if (q->pre_roll_frames < 0 || q->hold_frames < 0 || q->fade_in_frames < 0 || q->fade_out_frames < 0) return -1;
    if (q->curve != ZL_ED_LINEAR && q->curve != ZL_ED_SQRT && q->curve != ZL_ED_SMOOTH) return -1;
    if (q->num_frames == 0) q->num_frames = length - q->first_frame;
    if (q->threshold == 0.0f) q->threshold = ZL_ED_THRESHOLD;
    return 0;
}

ZL_HD inline bool zl_ed_loud(float v, float threshold) { return !(fabsf(v) < threshold); }

// the kept region [*a2, *b2) from the asked one [a, b) and the scan's F and Z (both ignored without trim).  1, or 0: no loud frame
inline int zl_ed_region(int32_t a, int32_t b, bool trim, int32_t F, int32_t Z, int32_t pre_roll, int32_t hold, int32_t *a2, int32_t *b2)
{
    *a2 = a; *b2 = b;
    if (!trim) return 1;
    if (F > Z) return 0;
    const int64_t lo = (int64_t)F - pre_roll, hi = (int64_t)Z + 1 + hold;
    *a2 = lo > a ? (int32_t)lo : a;
    *b2 = hi < b ? (int32_t)hi : b;
    return 1;
}

inline void zl_ed_fades(int32_t n, int32_t fade_in, int32_t fade_out, int32_t *Xi, int32_t *Xo)
{
    const int32_t half = n / 2;
    *Xi = fade_in < half ? fade_in : half;
    *Xo = fade_out < half ? fade_out : half;
}

inline bool zl_ed_identity(int32_t length, int32_t a2, int32_t n, bool reverse, int32_t Xi, int32_t Xo) { return a2 == 0 && n == length && !reverse && Xi == 0 && Xo == 0; }

// the table: X weights, rising from w[0] = 0 (one IEEE operation per operator: build without contraction)
inline void zl_ed_design(int32_t X, int32_t curve, float *w)
{
    for (int32_t i = 0; i < X; ++i) {
        const double t = (double)i / (double)X;
        double v = t;
        if (curve == ZL_ED_SQRT) v = sqrt(t);
        if (curve == ZL_ED_SMOOTH) { const double tt = t * t, t2 = 2.0 * t; const double r = 3.0 - t2; v = tt * r; }
        w[i] = (float)v;
    }
}

// One TRIM request of a call as the scanning kernel sees it, and the two words it leaves (built and initialised by the host)
struct ZlEdScan {
    uint64_t src;                // device address of the original extent (16-byte aligned)
    int32_t  channels, a, b;     // 1 or 2; the region to scan
    int32_t  wg_base;            // the request's first scanning workgroup in the call
    float    threshold;
    int32_t  found;              // the request's ZlEdFound among the call's
};
struct ZlEdFound { int32_t first, last; };   // INT32_MAX and -1 before the launch

ZL_HD inline int32_t zl_ed_scan_wgs(const ZlEdScan &S) { return (S.b - S.a + ZL_ED_CHUNK - 1) / ZL_ED_CHUNK; }
// chunk c of the region covers the clip's frames [*lo, *hi)
ZL_HD inline void zl_ed_chunk(const ZlEdScan &S, int32_t c, int32_t *lo, int32_t *hi)
{
    *lo = S.a + c * ZL_ED_CHUNK;
    *hi = S.b - *lo > ZL_ED_CHUNK ? *lo + ZL_ED_CHUNK : S.b;
}
// the frame of float `index` of an extent
ZL_HD inline int32_t zl_ed_frame_of(int64_t index, int32_t channels) { return (int32_t)(channels == 2 ? index >> 1 : index); }

// One applied request of a call as the render kernel sees it (built by the host)
struct ZlEdJob {
    uint64_t src, dst;           // device addresses of the original and of the new extent (16-byte aligned)
    int32_t  channels;           // 1 or 2; of both
    int32_t  a, n;               // the kept region [a, a + n) of the source = the new length
    int32_t  reverse;            // 0 or 1
    int32_t  Xi, Xo;             // frames faded in and out, each <= n / 2
    int32_t  wg_base;            // the job's first render workgroup in the call
    int32_t  w_in, w_out;        // the job's first weights in the call's weight buffer
    int32_t  verdict;            // the clip's word among the call's verdicts (set when a written faded sample is not finite)
};

// floats and groups of the new extent (zl_extent_floats, zl_arena.h)
ZL_HD inline int64_t zl_ed_extent_floats(int64_t length, int32_t channels) { return ((length + ZL_ED_PAD) * channels + 3) & ~(int64_t)3; }
ZL_HD inline int64_t zl_ed_groups(const ZlEdJob &J) { return zl_ed_extent_floats(J.n, J.channels) >> 2; }
ZL_HD inline int32_t zl_ed_job_wgs(const ZlEdJob &J) { return (int32_t)((zl_ed_groups(J) + ZL_ED_WG - 1) / ZL_ED_WG); }
ZL_HD inline int64_t zl_ed_data_floats(const ZlEdJob &J) { return (int64_t)J.n * J.channels; }
// does group g hold a float of the data; does it lie wholly inside the data (then it is one wide load)?
ZL_HD inline bool zl_ed_group_loads(const ZlEdJob &J, int64_t g) { return 4 * g < zl_ed_data_floats(J); }
ZL_HD inline bool zl_ed_group_full(const ZlEdJob &J, int64_t g) { return 4 * g + 4 <= zl_ed_data_floats(J); }
// a full group's first source float: four consecutive floats, never below a channels, never beyond (a + n) channels
ZL_HD inline int64_t zl_ed_group_first(const ZlEdJob &J, int64_t g)
{
    return J.reverse ? (int64_t)(J.a + J.n) * J.channels - 4 - 4 * g : (int64_t)J.a * J.channels + 4 * g;
}
// which of those four floats the group's float j is
ZL_HD inline int zl_ed_lane(const ZlEdJob &J, int j) { return !J.reverse ? j : (J.channels == 2 ? j ^ 2 : 3 - j); }
// the source float of the data's float k (any group)
ZL_HD inline int64_t zl_ed_src_index(const ZlEdJob &J, int64_t k)
{
    if (!J.reverse) return (int64_t)J.a * J.channels + k;
    const int64_t i = J.channels == 2 ? k >> 1 : k, c = J.channels == 2 ? (k & 1) : 0;
    return ((int64_t)(J.a + J.n) - 1 - i) * J.channels + c;
}
// does group g hold a faded float?
ZL_HD inline bool zl_ed_group_fades(const ZlEdJob &J, int64_t g)
{
    const int64_t k0 = 4 * g, data = zl_ed_data_floats(J);
    return k0 < data && (k0 < (int64_t)J.Xi * J.channels || k0 + 4 > (int64_t)(J.n - J.Xo) * J.channels);
}
// output frame i (< n): its weight in the call's buffer, or -1: it is not faded
ZL_HD inline int32_t zl_ed_weight_index(const ZlEdJob &J, int32_t i)
{
    if (i < J.Xi) return J.w_in + i;
    if (i >= J.n - J.Xo) return J.w_out + (J.n - 1 - i);
    return -1;
}
ZL_HD inline bool zl_ed_finite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_edit.hip; 0 or a hipError_t value).  found [nscan]; weights: the call's tables; verdicts [njobs]
int zl_launch_edit_scan(const ZlEdScan *reqs, int32_t nscan, int32_t wgs, ZlEdFound *found, hipStream_t s);
int zl_launch_edit_render(const ZlEdJob *jobs, int32_t njobs, int32_t wgs, const float *weights, uint32_t *verdicts, hipStream_t s);
#endif
