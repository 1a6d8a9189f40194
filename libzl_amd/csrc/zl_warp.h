// zl_warp.h -- a clip warped to the session grid on the device (zlhip_sound_warp / _batch): a time stretch that is
// cut at the clip's hits.  A request is a list of anchors (src_frame a, dst_frame d); region i plays the source frames [a_i, a_i+1) in the
// output frames [d_i, d_i+1).  Every region starts exactly at its anchor with no seek, so an attack is copied 1:1 and lands where the
// request puts it, and the seek chains of different regions do not depend on each other.  The reference has no warp: a build-defined
// extension that claims no parity.  Shared by the HIP kernels (zl_warp.hip), the engine and a host build for the CPU tier
// (tests/cpu_harness/warp_host.cpp): everything is defined HERE, once.  From section 8 (zl_stretch.h) come zl_st_q, zl_st_ref,
// zl_st_score, zl_st_better, zl_st_xfade, the ZL_ST_* constants and ZL_ST_PAD, unchanged.
//
//   Resolve.   (zl_wp_resolve, host) 2 <= count <= ZL_WP_MAX_ANCHORS; anchors[0] = (0, 0), anchors[count - 1].src = len; a and d strictly
//              increasing; N = d_last, N + ZL_ST_PAD <= INT32_MAX.  Region i: A = a_i+1 - a_i, D = d_i+1 - d_i, A <= 4 D and D <= 4 A
//              (integer compares).  Every A = D: the identity, applied = 0, no error.  O: section 8's overlap of the rate, one per clip.
//              A != D ("stretched"): tau = (double)A / (double)D; S and W from tau by section 8's two linear laws (zl_wp_sw restates
//              them); L = S - O; nseg = ceil(D / L); room = A - L - (W - 1); step = tau * (double)L, one rounded product.  It needs
//              S > O, W >= 1, W + O <= ZL_ST_MAX_WINDOW and room >= 0.  A = D ("copy"): one segment of D frames, no seek (L = D here).
//   Segments.  b_0 = a, off_0 = 0.  1 <= k < nseg: b_k = a + min(floor(k * step), room) + off_k, off_k in [0, W) the argmax of
//              zl_st_score against the weighted reference of mid[i] = q(in(b_k-1 + L + i)), i < O: section 8's seek and tie rule.
//              The clamp gives b_k + L <= a + A: no frame a region plays comes from the next one.  Segment k makes min(L, D - k L) frames.
//   Output n.  The region with d_i <= n < d_i+1; m = n - d_i, k = m / L, j = m - k L, v = in(b_k + j, c); in is 0 at or beyond len.
//              j < O and not the clip's very first segment: y = zl_st_xfade(in(pb + plen + j, c), v, j, O), (pb, plen) the base and the
//              output frames of the segment before it in output order (the same region's k - 1, else the last segment of region i - 1).
//              Else y = v.
//   Extent.    N frames in the arena's layout: interleaved, ZL_ST_PAD zero frames behind them, zeros up to the 16-byte boundary; produced.
//   Finite.    ZL_SOUND_FINITE stays set iff the original had it and every written sample is finite.
//   Plan.      (zl_wp_plan, host, double, the order as written) from hits to anchors; see there.
// Every float operation is one rounded fp32 operation (built without contraction everywhere).
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_stretch.h"

#define ZL_WP_MAX_ANCHORS    4096
#define ZL_WP_RATIO          4            // a region's A <= 4 D and D <= 4 A
#define ZL_WP_PLAN_RATIO     2            // the plan keeps A <= 2 D and D <= 2 A
#define ZL_WP_SEEK_THREADS   512          // lanes of a seek workgroup (one stretched region)
#define ZL_WP_SYNTH_THREADS  256          // lanes of a synthesis workgroup, one output frame each

struct ZlWpAnchor { int32_t src, dst; };                                                  // (zlhip_warp_anchor)
struct ZlWpSummary { int32_t applied, regions, stretched, segments, length, overlap; };  // (zlhip_warp)

// One region as the kernels see it.  A copy region has W = 0, nseg = 1 and L = D, so that k = m / L is 0 for every frame of it.
struct ZlWpRegion {
    double  step;                // tau * L (0 for a copy region)
    int32_t a, d, A, D;          // the region's first source and output frame, its source and output frames
    int32_t L, W, nseg, room;
    int32_t off_base;            // the region's first seek offset: from the clip's first (resolve), from the call's first (a job's table)
    int32_t job;                 // the region's clip among the call's jobs
};

// One applied clip of a call
struct ZlWpJob {
    uint64_t src, dst;           // device addresses of the original and of the new extent (16-byte aligned)
    int32_t  len, channels;      // source frames; 1 or 2
    int32_t  N, O;               // output frames, the clip's overlap
    int32_t  region_base, nregions;   // the clip's regions in the call's table
    int32_t  wg_base;            // the clip's first synthesis workgroup in the call
    int32_t  verdict;            // the clip's word among the call's verdicts (set when a written sample is not finite)
};

// ---- geometry (host) ----------------------------------------------------------------------------------------------------------------
// section 8's overlap of a rate (zl_st_geometry's O lines)
inline int32_t zl_wp_overlap(double sr)
{
    int64_t O = (int64_t)floor(sr * ZL_ST_OVERLAP_SEC);
    O = O < ZL_ST_OVERLAP_MIN ? ZL_ST_OVERLAP_MIN : (O > ZL_ST_OVERLAP_MAX ? ZL_ST_OVERLAP_MAX : O);
    return (int32_t)(O & ~(int64_t)7);
}

// section 8's two linear laws (zl_st_geometry's S and W lines)
inline void zl_wp_sw(double sr, double tau, int32_t *S, int32_t *W)
{
    const double seq_ms = zl_st_clamp(ZL_ST_SEQ_MS_AT_LO + (ZL_ST_SEQ_MS_AT_HI - ZL_ST_SEQ_MS_AT_LO) / ZL_ST_TAU_SPAN * (tau - ZL_ST_TAU_LO),
                                      ZL_ST_SEQ_MS_AT_HI, ZL_ST_SEQ_MS_AT_LO);
    const double seek_ms = zl_st_clamp(ZL_ST_SEEK_MS_AT_LO + (ZL_ST_SEEK_MS_AT_HI - ZL_ST_SEEK_MS_AT_LO) / ZL_ST_TAU_SPAN * (tau - ZL_ST_TAU_LO),
                                       ZL_ST_SEEK_MS_AT_HI, ZL_ST_SEEK_MS_AT_LO);
    const double s = floor(sr * seq_ms / 1000.0), w = floor(sr * seek_ms / 1000.0);
    *S = s < 2e9 ? (int32_t)s : 2000000000;
    *W = w < 2e9 ? (int32_t)w : 2000000000;
}

// One region's rules with the ratio limit `ratio`; 0 = acceptable (*R filled but for off_base and job), -1 = not
inline int zl_wp_region(double sr, int32_t O, int64_t a, int64_t d, int64_t A, int64_t D, int ratio, ZlWpRegion *R)
{
    if (A < 1 || D < 1 || A > 0x7fffffff || D > 0x7fffffff || A > ratio * D || D > ratio * A) return -1;
    R->a = (int32_t)a; R->d = (int32_t)d; R->A = (int32_t)A; R->D = (int32_t)D; R->off_base = 0; R->job = 0;
    if (A == D) { R->step = 0.0; R->L = (int32_t)D; R->W = 0; R->nseg = 1; R->room = 0; return 0; }
    const double tau = (double)A / (double)D;
    int32_t S, W;
    zl_wp_sw(sr, tau, &S, &W);
    if (S <= O || W < 1 || (int64_t)W + O > ZL_ST_MAX_WINDOW) return -1;
    const int64_t L = S - O, room = A - L - ((int64_t)W - 1);
    if (room < 0) return -1;
    R->L = (int32_t)L; R->W = W; R->nseg = (int32_t)((D + L - 1) / L); R->room = (int32_t)room;
    R->step = tau * (double)L;
    return 0;
}

// 0 = the request resolves (*sum filled; regs, if given: count - 1 records with off_base counted from the clip's first offset), -1 = not
inline int zl_wp_resolve(double sr, int64_t len, const ZlWpAnchor *an, int32_t count, ZlWpSummary *sum, ZlWpRegion *regs)
{
    if (!(sr > 0.0 && sr < 1e9) || len < 1 || len > 0x7fffffff || !an || count < 2 || count > ZL_WP_MAX_ANCHORS) return -1;
    if (an[0].src != 0 || an[0].dst != 0 || (int64_t)an[count - 1].src != len) return -1;
    for (int32_t i = 0; i + 1 < count; ++i)
        if (an[i + 1].src <= an[i].src || an[i + 1].dst <= an[i].dst) return -1;
    const int64_t N = an[count - 1].dst;
    if (N + ZL_ST_PAD > 0x7fffffff) return -1;
    const int32_t O = zl_wp_overlap(sr);
    int64_t segments = 0; int32_t stretched = 0;
    for (int32_t i = 0; i + 1 < count; ++i) {
        ZlWpRegion R;
        if (zl_wp_region(sr, O, an[i].src, an[i].dst, (int64_t)an[i + 1].src - an[i].src, (int64_t)an[i + 1].dst - an[i].dst, ZL_WP_RATIO, &R) != 0) return -1;
        R.off_base = (int32_t)segments;
        segments += R.nseg;
        stretched += R.W > 0 ? 1 : 0;
        if (regs) regs[i] = R;
    }
    if (segments > 0x7fffffff) return -1;
    sum->applied = stretched > 0 ? 1 : 0; sum->regions = count - 1; sum->stretched = stretched; sum->segments = (int32_t)segments;
    sum->length = (int32_t)N; sum->overlap = O;
    return 0;
}

// the piecewise-linear image of a source frame (floor, int64 arithmetic); frames in front of the clip map to 0, behind it to d_last
inline int64_t zl_wp_map(const ZlWpAnchor *an, int32_t count, int64_t src)
{
    if (src <= an[0].src) return an[0].dst;
    if (src >= an[count - 1].src) return an[count - 1].dst;
    int32_t lo = 0, hi = count - 2;                                // the last i with a_i <= src
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (an[mid].src <= src) lo = mid; else hi = mid - 1; }
    const int64_t A = (int64_t)an[lo + 1].src - an[lo].src, D = (int64_t)an[lo + 1].dst - an[lo].dst;
    return (int64_t)an[lo].dst + ((src - an[lo].src) * D) / A;
}

// ---- the plan: from hits to anchors (host; double, the order as written) ---------------------------------------------------------------
//   scale = src_bpm / dst_bpm; g = (rate * 60) / (src_bpm * steps_per_beat); P = preroll (-1: the rate's O).  Every onset t, ascending:
//   q = rint((t - origin) / g) (ties to even), target = origin + q g, moved = t + strength (target - t), the candidate anchor is
//   (t - P, rint(moved * scale) - P); candidates with src <= 0 are skipped.  Start (0, 0), end (length, max(1, rint(length * scale))).
//   Greedy, left to right: a candidate is kept iff the region from the last kept anchor to it and the region from it to the end anchor
//   are both acceptable (zl_wp_region with ZL_WP_PLAN_RATIO), so the result always resolves; *dropped counts the candidates not kept.
// 0 = planned, -1 = a parameter outside its range or the single region start -> end not acceptable, -2 = capacity below the count
inline int zl_wp_plan(double sr, int64_t len, const int32_t *onsets, int32_t n, double src_bpm, double dst_bpm, int32_t steps_per_beat, double strength,
                      int64_t origin, int32_t preroll, ZlWpAnchor *out, int32_t capacity, int32_t *count, int32_t *dropped)
{
    if (!(sr > 0.0 && sr < 1e9) || len < 1 || len > 0x7fffffff || n < 0 || (n > 0 && !onsets) || !out || !count || !dropped) return -1;
    if (!(src_bpm > 0.0) || !(dst_bpm > 0.0) || !isfinite(src_bpm) || !isfinite(dst_bpm) || steps_per_beat < 1 || steps_per_beat > 64) return -1;
    if (!(strength >= 0.0 && strength <= 1.0) || origin < 0 || origin >= len || preroll < -1) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (onsets[i] < 0 || (int64_t)onsets[i] > len || (i > 0 && onsets[i] < onsets[i - 1])) return -1;
    const int32_t O = zl_wp_overlap(sr);
    const int64_t P = preroll < 0 ? O : preroll;
    const double scale = src_bpm / dst_bpm;
    const double g = (sr * 60.0) / (src_bpm * (double)steps_per_beat);
    const double endd = rint((double)len * scale);
    if (!(endd + ZL_ST_PAD <= 2147483647.0)) return -1;
    const int64_t endDst = endd < 1.0 ? 1 : (int64_t)endd;
    ZlWpRegion R;
    if (zl_wp_region(sr, O, 0, 0, len, endDst, ZL_WP_PLAN_RATIO, &R) != 0) return -1;
    int32_t kept = 1, lost = 0;
    int64_t la = 0, ld = 0;
    if (capacity < 2) return -2;
    out[0].src = 0; out[0].dst = 0;
    for (int32_t i = 0; i < n; ++i) {
        const double t = (double)onsets[i];
        const double q = rint((t - (double)origin) / g);
        const double target = (double)origin + q * g;
        const double moved = t + strength * (target - t);
        const int64_t ca = (int64_t)onsets[i] - P;
        if (ca <= 0) continue;
        const double cdd = rint(moved * scale) - (double)P;
        bool ok = cdd > (double)ld && cdd < (double)endDst && ca > la && ca < len;
        const int64_t cd = ok ? (int64_t)cdd : 0;
        ok = ok && zl_wp_region(sr, O, la, ld, ca - la, cd - ld, ZL_WP_PLAN_RATIO, &R) == 0
                && zl_wp_region(sr, O, ca, cd, len - ca, endDst - cd, ZL_WP_PLAN_RATIO, &R) == 0;
        if (!ok) { ++lost; continue; }
        if (kept + 2 > capacity) return -2;
        out[kept].src = (int32_t)ca; out[kept].dst = (int32_t)cd; ++kept;
        la = ca; ld = cd;
    }
    if (kept + 1 > capacity) return -2;
    out[kept].src = (int32_t)len; out[kept].dst = (int32_t)endDst; ++kept;
    *count = kept; *dropped = lost;
    return 0;
}

// ---- what the kernels and the harness walk ---------------------------------------------------------------------------------------------
ZL_HD inline int64_t zl_wp_extent_floats(int64_t N, int32_t channels) { return ((N + ZL_ST_PAD) * channels + 3) & ~(int64_t)3; }
// the synthesis' lanes of a clip: one per frame of the extent, the zero frames and the floats up to the 16-byte boundary included
// (the extent's floats are a multiple of 4, so of the channels)
ZL_HD inline int64_t zl_wp_lanes(const ZlWpJob &J) { return zl_wp_extent_floats(J.N, J.channels) / J.channels; }
ZL_HD inline int32_t zl_wp_job_wgs(const ZlWpJob &J) { return (int32_t)((zl_wp_lanes(J) + ZL_WP_SYNTH_THREADS - 1) / ZL_WP_SYNTH_THREADS); }
ZL_HD inline bool zl_wp_finite(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// segment k >= 1 of a stretched region: where its seek window starts; any segment: its base given the offsets, its output frames
ZL_HD inline int64_t zl_wp_nominal(const ZlWpRegion &R, int32_t k)
{
    const int64_t f = (int64_t)floor((double)k * R.step);
    return (int64_t)R.a + (f < (int64_t)R.room ? f : (int64_t)R.room);
}
ZL_HD inline int64_t zl_wp_base(const ZlWpRegion &R, const int32_t *off, int32_t k) { return k == 0 ? (int64_t)R.a : zl_wp_nominal(R, k) + off[R.off_base + k]; }
ZL_HD inline int32_t zl_wp_seg_frames(const ZlWpRegion &R, int32_t k)
{
    const int64_t rest = (int64_t)R.D - (int64_t)k * R.L;
    return (int32_t)(rest < (int64_t)R.L ? rest : (int64_t)R.L);
}

// the clip's region of output frame n < N: the last one whose d is <= n (regs: the clip's own records, d increasing, regs[0].d = 0)
ZL_HD inline int32_t zl_wp_find_region(const ZlWpRegion *regs, int32_t nregions, int32_t n)
{
    int32_t lo = 0, hi = nregions - 1;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (regs[mid].d <= n) lo = mid; else hi = mid - 1; }
    return lo;
}

// Output frame n of a clip, in its region i: the source frame it plays, and, where it lies in a join, the frame it is faded from
struct ZlWpTap { int64_t v, p; int32_t j, fade; };
ZL_HD inline ZlWpTap zl_wp_tap(const ZlWpRegion *regs, int32_t i, const int32_t *off, int32_t O, int32_t n)
{
    const ZlWpRegion &R = regs[i];
    const int32_t m = n - R.d, k = m / R.L, j = m - k * R.L;
    ZlWpTap t;
    t.v = zl_wp_base(R, off, k) + j; t.p = 0; t.j = j; t.fade = 0;
    if (j >= O || (i == 0 && k == 0)) return t;
    t.fade = 1;
    if (k > 0) {
        t.p = zl_wp_base(R, off, k - 1) + R.L + j;
    } else {
        const ZlWpRegion &Q = regs[i - 1];
        const int32_t pk = Q.nseg - 1;
        t.p = zl_wp_base(Q, off, pk) + zl_wp_seg_frames(Q, pk) + j;
    }
    return t;
}
// the sample from the frame it plays (v) and, in a join, the frame it is faded from (p; not looked at elsewhere)
ZL_HD inline float zl_wp_join(const ZlWpTap &t, int32_t O, float p, float v) { return t.fade ? zl_st_xfade(p, v, t.j, O) : v; }
template <class In>
ZL_HD inline float zl_wp_sample(const ZlWpTap &t, int32_t O, int c, const In &in)
{
    const float v = in(t.v, c);
    return zl_wp_join(t, O, t.fade ? in(t.p, c) : 0.0f, v);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_warp.hip; 0 or a hipError_t value).  seek_regions: the call's regions with nseg > 1; offsets: the call's seek offsets,
// zeroed by the caller; verdicts [njobs]
int zl_launch_warp_seek(const ZlWpJob *jobs, const ZlWpRegion *regions, const int32_t *seek_regions, int32_t nseek, int32_t *offsets, hipStream_t s);
int zl_launch_warp_synth(const ZlWpJob *jobs, int32_t njobs, int32_t wgs, const ZlWpRegion *regions, const int32_t *offsets, uint32_t *verdicts, hipStream_t s);
#endif
