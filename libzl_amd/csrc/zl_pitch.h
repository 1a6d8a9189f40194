// zl_pitch.h -- a clip's pitch, detected on the device (zlhip_sound_pitch / _batch): what note a one-shot is, so
// that a sampler can set its root note (ClipAudioSource_setRootNote takes a note the caller must already know).  The reference has no
// pitch detection, so this is a build-defined extension and claims no parity.  Shared by the HIP kernels (zl_pitch.hip), the engine
// and a host build for the CPU tier (tests/cpu_harness/pitch_host.cpp): everything is defined HERE, once.  It is YIN's difference
// function, cumulative-mean normalisation and absolute threshold, made exact by section 8's 16-bit quantisation: everything behind
// zl_st_q is integer arithmetic, so every reduction order gives the same bits.
//
// A request is (sound, first_frame, num_frames, window, max_frames, f_min, f_max, threshold, gate) over the sound's current playback data.
//
//   Lags.       t_min = max(2, ceil(rate / f_max)), t_max = floor(rate / f_min), one double division each (zl_pt_lags).
//   Window.     W = window; given as 0: min(4096, roundup(2 t_max, 64)).  A frame needs L = W + t_max + 1 samples.
//   Frames.     num_frames < L: no frames ("no pitch", not an error).  Otherwise hop = W, K = (num_frames - L) / hop + 1; K > max_frames:
//               K = max_frames and hop = (num_frames - L) / (max_frames - 1) (max_frames 1: K = 1).  Frame k starts at
//               s_k = first_frame + k hop: the frames spread over the whole region (zl_pt_frames).
//   Mono mix.   m[f] = the sum over the channels of zl_st_q(v), |m| <= 65534; NaN -> 0.
//   Gate.       e_k = the sum over j < W of m[s_k + j]^2 as uint64 (< 2^46); e_k < W channels gate^2: the frame is SILENT.
//   Shift.      sh_k = max(0, bitlength(max over j < L of |m[s_k + j]|) - 12); x[j] = m[s_k + j] >> sh_k (arithmetic), -2^12 <= x < 2^12.
//               Everything behind this is a ratio, so the shift changes no decision; it only bounds the sums.
//   Difference. d[t] = the sum over j < W of (x[j] - x[j + t])^2 for t in [1, t_max + 1]; a term is below 2^26, d < 2^38.
//   Cumulative. C[t] = d[1] + ... + d[t] < 2^49.
//   Threshold.  t0 = the smallest t in [t_min, t_max] with d[t] t 1024 < threshold C[t] in uint64 (both sides below 2^60); none: the
//               frame is UNVOICED (a constant signal has C = 0).
//   Descend.    t_k = the first t >= t0 with t = t_max or d[t + 1] >= d[t]: the local minimum of d itself.
//   Clarity.    c_k = L(C[t_k] + 1) - L(d[t_k] t_k + 1), L = zl_on_level (a log2 in 1/64 octaves).
//   Record.     per frame (t_k, c_k, sh_k, flag, d[t_k - 1], d[t_k], d[t_k + 1], C[t_k]); silent and unvoiced frames: t_k = 0 and
//               every field 0 except sh_k and the flag that says which.
//   Vote.       V = the voiced frames; t_med = their lower median (index (V - 1) / 2 of the sorted lags); a frame is CONSISTENT if
//               |t_k - t_med| <= t_med >> 5 (about half a semitone); the representative is the consistent frame with the largest c_k,
//               equal values go to the smaller k.  The device writes integers only (ZlPtResult).
//   No pitch.   no frames or V = 0: every field 0 except frames.  Not an error.
//   Finish.     host, double (zl_pt_finish): the parabola through d[t - 1], d[t], d[t + 1], hz, note, root_note, cents, confidence.
//
// The difference function is evaluated in work items (request, frame, tile of ZL_PT_TILE lags), numbered over the call; the tiles of
// a frame are neighbours (they share the frame's samples).  zl_pt_item_of and zl_pt_lane_lag say what a lane of an item sums.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_onset.h"
#include "zl_types.h"

#define ZL_PT_F_MIN_DEFAULT      55.0f
#define ZL_PT_F_MAX_DEFAULT      1760.0f
#define ZL_PT_THRESHOLD_DEFAULT  154         // 0.15 in 1/1024
#define ZL_PT_GATE_DEFAULT       8
#define ZL_PT_FRAMES_DEFAULT     64
#define ZL_PT_F_LO               20.0f
#define ZL_PT_WINDOW_MIN         256
#define ZL_PT_WINDOW_MAX         4096
#define ZL_PT_MAX_LAGS           2048        // t_max + 1 at most
#define ZL_PT_THRESHOLD_MAX      1024
#define ZL_PT_GATE_MAX           32767
#define ZL_PT_MAX_FRAMES         256         // per request: one lane each in the vote
#define ZL_PT_MAX_CALL_FRAMES    65536       // per call
#define ZL_PT_TILE               256         // lags of a work item: one lane each
#define ZL_PT_MAX_SPAN           (ZL_PT_WINDOW_MAX + ZL_PT_MAX_LAGS)      // the largest L
#define ZL_PT_BITS               12          // |x| <= 2^12
#define ZL_PT_CHUNK              32          // terms whose sum stays in 32 bits: 32 (2^13 - 1)^2 < 2^32

#define ZL_PT_VOICED             0
#define ZL_PT_SILENT             1
#define ZL_PT_UNVOICED           2

// t_min and t_max (host): the only place the two divisions are written
inline void zl_pt_lags(double sample_rate, float f_min, float f_max, double *tmin, double *tmax)
{
    const double a = ceil(sample_rate / (double)f_max);
    *tmin = a < 2.0 ? 2.0 : a;
    *tmax = floor(sample_rate / (double)f_min);
}

// the defaults of the fields given as 0 and the limits that need no sound; the only place they are written.  0 = valid, -1 = not
inline int zl_pt_resolve(double sample_rate, int32_t *window, int32_t *max_frames, float *f_min, float *f_max, int32_t *threshold, int32_t *gate)
{
    if (!(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    if (*f_min == 0.0f) *f_min = ZL_PT_F_MIN_DEFAULT;
    if (*f_max == 0.0f) *f_max = ZL_PT_F_MAX_DEFAULT;
    if (*threshold == 0) *threshold = ZL_PT_THRESHOLD_DEFAULT;
    if (*gate == 0) *gate = ZL_PT_GATE_DEFAULT;
    if (*max_frames == 0) *max_frames = ZL_PT_FRAMES_DEFAULT;
    if (!(*f_min >= ZL_PT_F_LO && *f_min < *f_max && (double)*f_max < sample_rate / 2.0)) return -1;          // (NaN and inf fail here)
    double tmin, tmax;
    zl_pt_lags(sample_rate, *f_min, *f_max, &tmin, &tmax);
    if (tmax + 1.0 > (double)ZL_PT_MAX_LAGS) return -1;
    if (*window == 0) {
        const int32_t w = (2 * (int32_t)tmax + 63) / 64 * 64;
        *window = w < ZL_PT_WINDOW_MAX ? w : ZL_PT_WINDOW_MAX;
    }
    if (*window < ZL_PT_WINDOW_MIN || *window > ZL_PT_WINDOW_MAX || (*window & 63) != 0) return -1;
    if (tmax + 1.0 > (double)*window) return -1;
    if (*threshold < 1 || *threshold > ZL_PT_THRESHOLD_MAX || *gate < 1 || *gate > ZL_PT_GATE_MAX) return -1;
    if (*max_frames < 1 || *max_frames > ZL_PT_MAX_FRAMES) return -1;
    return 0;
}

// K and hop of a region of num_frames frames
ZL_HD inline void zl_pt_frames(int64_t num_frames, int32_t window, int32_t tmax, int32_t max_frames, int32_t *K, int32_t *hop)
{
    const int64_t L = (int64_t)window + tmax + 1;
    *hop = window;
    if (num_frames < L) { *K = 0; return; }
    const int64_t k = (num_frames - L) / window + 1;
    if (k <= max_frames) { *K = (int32_t)k; return; }
    *K = max_frames;
    if (max_frames > 1) *hop = (int32_t)((num_frames - L) / (max_frames - 1));
}

// One request of a call as the kernels see it (built by the host)
struct ZlPtRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned)
    uint64_t floor_;             // W channels gate^2: a frame with less energy is silent
    int64_t  d_base;             // the request's first word in the call's d array: frame k's d[t] is word d_base + k (t_max + 1) + t - 1
    int32_t  first, hop, frames, channels;       // frames: K
    int32_t  window, tmin, tmax, threshold;
    int32_t  frame_base;         // the request's first frame in the call's per-frame arrays
    int32_t  item_base;          // the request's first work item of the call
};

// what the diff kernel leaves per frame for the pick kernel
struct ZlPtStat { uint64_t energy; int32_t shift, silent; };

// a frame's record (zlhip_pitch_frame's layout)
struct ZlPtFrame { int32_t lag, clarity, shift, flag; uint64_t d_lo, d_mid, d_hi, cum; };

// the result as the device writes it: the layout of zlhip_pitch (the floats and root_note are the host's)
struct ZlPtResult {
    float hz, note, cents, confidence;
    int32_t root_note, frames, voiced, consistent, frame, lag, shift, clarity;
    uint64_t d_lo, d_mid, d_hi, cum;
};

ZL_HD inline int32_t zl_pt_span(const ZlPtRequest &R) { return R.window + R.tmax + 1; }
ZL_HD inline int32_t zl_pt_nd(const ZlPtRequest &R) { return R.tmax + 1; }
ZL_HD inline int32_t zl_pt_tiles(const ZlPtRequest &R) { return (zl_pt_nd(R) + ZL_PT_TILE - 1) / ZL_PT_TILE; }
ZL_HD inline int32_t zl_pt_items(const ZlPtRequest &R) { return R.frames * zl_pt_tiles(R); }
ZL_HD inline int64_t zl_pt_frame_start(const ZlPtRequest &R, int32_t k) { return (int64_t)R.first + (int64_t)k * R.hop; }

// item i of a request: its frame and its tile of lags
ZL_HD inline void zl_pt_item_of(const ZlPtRequest &R, int32_t i, int32_t *frame, int32_t *tile)
{
    const int32_t tiles = zl_pt_tiles(R);
    *frame = i / tiles;
    *tile = i - *frame * tiles;
}

// the lag of lane `lane` of a tile, and whether the lane owns it: the lanes behind t_max + 1 sum the last lag again and store nothing,
// so no lane reads behind the frame's L samples
ZL_HD inline bool zl_pt_lane_live(const ZlPtRequest &R, int32_t tile, int32_t lane) { return tile * ZL_PT_TILE + lane + 1 <= zl_pt_nd(R); }
ZL_HD inline int32_t zl_pt_lane_lag(const ZlPtRequest &R, int32_t tile, int32_t lane)
{
    const int32_t t = tile * ZL_PT_TILE + lane + 1;
    return t <= zl_pt_nd(R) ? t : zl_pt_nd(R);
}

ZL_HD inline int32_t zl_pt_bitlength(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return x ? 32 - __clz((int)x) : 0;
#else
    return x ? 32 - __builtin_clz(x) : 0;
#endif
}

ZL_HD inline int32_t zl_pt_shift(uint32_t maxabs) { const int32_t b = zl_pt_bitlength(maxabs) - ZL_PT_BITS; return b > 0 ? b : 0; }

// The mix of one 16-byte group of the arena's layout (stereo [L0 R0 L1 R1], mono [x0 x1 x2 x3]).  grel: the group counted from the
// frame span's first group; head, count: zl_ov_groups' (floats of the first group in front of the span, floats of the span).  Slot s in
// [0, 4) is a mixed sample m[s] of the span's sample idx[s], or idx[s] = -1: nothing (an element outside the span, or a stereo
// frame's second slot).  The elements outside the span are never looked at.
ZL_HD inline void zl_pt_group_mix(float v0, float v1, float v2, float v3, int32_t grel, int32_t head, int32_t count, int32_t channels, int32_t *m, int32_t *idx)
{
    const int32_t rel = 4 * grel - head;
    if (channels == 2) {                                           // head and count are even: a frame never straddles two groups
        const bool a = zl_ov_valid(grel, 0, head, count), b = zl_ov_valid(grel, 2, head, count);
        m[0] = a ? zl_st_q(v0) + zl_st_q(v1) : 0; idx[0] = a ? rel >> 1 : -1;
        m[1] = b ? zl_st_q(v2) + zl_st_q(v3) : 0; idx[1] = b ? (rel + 2) >> 1 : -1;
        m[2] = 0; idx[2] = -1; m[3] = 0; idx[3] = -1;
    } else {
        const float v[4] = {v0, v1, v2, v3};
        for (int j = 0; j < 4; ++j) {
            const bool a = zl_ov_valid(grel, j, head, count);
            m[j] = a ? zl_st_q(v[j]) : 0; idx[j] = a ? rel + j : -1;
        }
    }
}

// the threshold: is lag t below it?  d = d[t], C = C[t]
ZL_HD inline bool zl_pt_below(uint64_t d, int32_t t, int32_t threshold, uint64_t C) { return d * (uint64_t)t * 1024u < (uint64_t)threshold * C; }

// the descent stops at t: d = d[t], dnext = d[t + 1]
ZL_HD inline bool zl_pt_stops(uint64_t d, uint64_t dnext, int32_t t, int32_t tmax) { return t == tmax || dnext >= d; }

ZL_HD inline int32_t zl_pt_clarity(uint64_t C, uint64_t d, int32_t t) { return zl_on_level(C + 1) - zl_on_level(d * (uint64_t)t + 1); }

// a frame's record from its lag (0: none), C[lag] and d (d[t] is d[t - 1] here: the array starts at lag 1)
ZL_HD inline void zl_pt_frame_record(const ZlPtStat &st, const uint64_t *d, uint64_t C, int32_t lag, ZlPtFrame *out)
{
    ZlPtFrame o;
    o.lag = 0; o.clarity = 0; o.shift = st.shift; o.flag = st.silent ? ZL_PT_SILENT : ZL_PT_UNVOICED;
    o.d_lo = 0; o.d_mid = 0; o.d_hi = 0; o.cum = 0;
    if (!st.silent && lag > 0) {
        o.lag = lag; o.flag = ZL_PT_VOICED;
        o.d_lo = d[lag - 2]; o.d_mid = d[lag - 1]; o.d_hi = d[lag]; o.cum = C;         // (lag >= t_min >= 2, lag + 1 <= t_max + 1)
        o.clarity = zl_pt_clarity(C, o.d_mid, lag);
    }
    *out = o;
}

ZL_HD inline bool zl_pt_consistent(int32_t lag, int32_t med) { const int32_t a = lag > med ? lag - med : med - lag; return a <= (med >> 5); }

// the representative's order as one signed word: the larger clarity first, then the smaller frame index
ZL_HD inline int64_t zl_pt_key(int32_t clarity, int32_t k) { return (int64_t)clarity * 65536 + (65535 - k); }
#define ZL_PT_NO_KEY INT64_MIN

// the integer result from the vote's outcome: K frames, V voiced, `consistent` of them consistent, the representative rep (-1: no pitch)
ZL_HD inline void zl_pt_result(int32_t K, int32_t V, int32_t consistent, int32_t rep, const ZlPtFrame *frames, ZlPtResult *out)
{
    ZlPtResult o;
    o.hz = 0.0f; o.note = 0.0f; o.cents = 0.0f; o.confidence = 0.0f;
    o.root_note = 0; o.frames = K; o.voiced = 0; o.consistent = 0; o.frame = 0; o.lag = 0; o.shift = 0; o.clarity = 0;
    o.d_lo = 0; o.d_mid = 0; o.d_hi = 0; o.cum = 0;
    if (V > 0 && rep >= 0) {
        const ZlPtFrame f = frames[rep];
        o.voiced = V; o.consistent = consistent; o.frame = rep; o.lag = f.lag; o.shift = f.shift; o.clarity = f.clarity;
        o.d_lo = f.d_lo; o.d_mid = f.d_mid; o.d_hi = f.d_hi; o.cum = f.cum;
    }
    *out = o;
}

// pick and vote by one thread, straight from the definition (the host route of scripts/pitch_bench.py and the harness's second opinion)
inline void zl_pt_pick_serial(const ZlPtRequest &R, const ZlPtStat &st, const uint64_t *d, ZlPtFrame *out)
{
    int32_t lag = 0; uint64_t C = 0, Clag = 0;
    for (int32_t t = 1; t <= R.tmax && !st.silent; ++t) {
        C += d[t - 1];
        if (lag == 0 && t >= R.tmin && zl_pt_below(d[t - 1], t, R.threshold, C)) lag = t;            // t0; the descent goes on from it
        if (lag != 0) { lag = t; Clag = C; if (zl_pt_stops(d[t - 1], d[t], t, R.tmax)) break; }
    }
    zl_pt_frame_record(st, d, Clag, lag, out);
}

inline void zl_pt_vote_serial(const ZlPtFrame *frames, int32_t K, ZlPtResult *out)
{
    int32_t hist[ZL_PT_MAX_LAGS] = {0}, V = 0;
    for (int32_t k = 0; k < K; ++k) if (frames[k].lag > 0) { ++hist[frames[k].lag]; ++V; }
    int32_t med = 0;
    for (int32_t t = 0, seen = 0; V > 0 && t < ZL_PT_MAX_LAGS; ++t) { seen += hist[t]; if (seen > (V - 1) / 2) { med = t; break; } }
    int32_t consistent = 0, rep = -1; int64_t best = ZL_PT_NO_KEY;
    for (int32_t k = 0; k < K; ++k) {
        if (frames[k].lag == 0 || !zl_pt_consistent(frames[k].lag, med)) continue;
        ++consistent;
        if (zl_pt_key(frames[k].clarity, k) > best) { best = zl_pt_key(frames[k].clarity, k); rep = k; }
    }
    zl_pt_result(K, V, consistent, rep, frames, out);
}

// hz, note, root_note, cents and confidence from the integer record (host, double, one IEEE operation per operator: build without
// contraction)
inline void zl_pt_finish(double sample_rate, ZlPtResult *r)
{
    r->hz = 0.0f; r->note = 0.0f; r->cents = 0.0f; r->confidence = 0.0f; r->root_note = 0;
    if (r->lag == 0) return;
    const double lo = (double)r->d_lo, mid = (double)r->d_mid, hi = (double)r->d_hi;
    const double den = (lo - 2.0 * mid) + hi;
    double delta = den > 0.0 ? (lo - hi) / (2.0 * den) : 0.0;
    delta = delta > 0.5 ? 0.5 : (delta < -0.5 ? -0.5 : delta);
    const double hz = sample_rate / ((double)r->lag + delta);
    const double note = 69.0 + 12.0 * log2(hz / 440.0);
    double root = rint(note);
    root = root < 0.0 ? 0.0 : (root > 127.0 ? 127.0 : root);
    r->hz = (float)hz;
    r->note = (float)note;
    r->root_note = (int32_t)root;
    r->cents = (float)(100.0 * (note - root));
    r->confidence = (float)((double)r->consistent / (double)r->frames);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_pitch.hip; 0 or a hipError_t value).  D [call d words] uint64, stat [call frames], frames [call frames]; out [nreq] may be
// host memory mapped into the device: only the records are written
int zl_launch_pitch_diff(const ZlPtRequest *reqs, int32_t nreq, int64_t items, uint64_t *D, ZlPtStat *stat, hipStream_t s);
int zl_launch_pitch_pick(const ZlPtRequest *reqs, int32_t nreq, int64_t frames, const uint64_t *D, const ZlPtStat *stat, ZlPtFrame *out, hipStream_t s);
int zl_launch_pitch_vote(const ZlPtRequest *reqs, int32_t nreq, const ZlPtFrame *frames, ZlPtResult *out, hipStream_t s);
#endif
