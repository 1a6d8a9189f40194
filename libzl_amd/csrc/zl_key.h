// zl_key.h -- a clip's musical key, detected on the device (zlhip_sound_key / _batch): the answer a loop browser
// shows next to bpm, and what libzl_hotpath_clip_match_key transposes a loop by.  The reference has no key detection, so this is a
// build-defined extension and claims no parity.  Shared by the HIP kernels (zl_key.hip), the engine and a host build for the CPU tier
// (tests/cpu_harness/key_host.cpp): everything is defined HERE, once.  It is a constant-Q bank of correlators, one per semitone, folded
// into a chroma vector and matched against the Krumhansl-Kessler profiles.  Behind section 8's 16-bit quantisation (zl_st_q) everything
// the device does is integer arithmetic, so every reduction order and every split of the work gives the same bits.
//
// A request is (sound, first_frame, num_frames, hop, max_frames, a4_hz, note_lo, note_hi, q, gate) over the sound's current playback data.
//
//   Table.      host, double (zl_ky_design), the only floating point in front of the device.  Bin b is MIDI note n = note_lo + b:
//               f = a4 2^((n - 69) / 12); N = rint(q rate / f), plus 1 if odd, at most 32768; step = rint(f / rate 2^32) < 2^31 (f is
//               below rate / 2); wstep = floor(2^32 / N) <= 2^27 (N >= 32).  T[i] = rint(32767 cos(2 pi i / 4096)), int16, 4096
//               entries: the only trigonometric table.
//   Frames.     L = the largest N (bin 0's: the lowest note).  num_frames < L: no frames ("no key", not an error).  Otherwise
//               K = (num_frames - L) / hop + 1; K > max_frames: K = max_frames and hop = (num_frames - L) / (max_frames - 1) (max_frames
//               1: K = 1) -- zl_pt_frames' rule (zl_ky_frames).  Frame k spans [s_k, s_k + L), s_k = first_frame + k hop, centred at
//               c_k = s_k + L / 2; bin b reads [c_k - N / 2, c_k + N / 2) = [s_k + off, s_k + off + N), off = (L - N) / 2 (every N is even).
//   Mono mix.   m[f] = the sum over the channels of zl_st_q(v), |m| <= 65534; NaN -> 0.
//   Gate.       e_k = the sum over the span of m^2 as uint64 (< 2^32 2^15 = 2^47); e_k < L channels gate^2: the frame is SILENT and
//               contributes nothing; its re and im read 0.
//   Correlator. j counts from the bin's window start, so frames are independent.  All products are modulo 2^32 where it says so:
//                 w  = (32767 - T[(j wstep mod 2^32) >> 20]) >> 1        0 <= w <= 32767 (j wstep < N wstep <= 2^32: it never wraps)
//                 v  = (m w) >> 15 (arithmetic)                          |m w| <= 65534 * 32767 < 2^31: int32; |v| <= 65534
//                 ph = j step mod 2^32;  c = T[ph >> 20];  s = T[((ph - 2^30) mod 2^32) >> 20] = T[((ph >> 20) - 1024) mod 4096]
//                 re = the sum of v c, im = the sum of v s                |v c| <= 65534 * 32767 = 2147352578 < 2^31: a term is an
//               int32, and two full-scale terms are not: no chunk of more than ONE term provably fits 32 bits, so every term is
//               widened as it is added (a data-dependent chunk would change nothing in the sums and is not worth its branch: the
//               loop is bound by the LDS gathers, see zl_key.hip).  |re|, |im| <= N 2^31 <= 2^46: int64.
//   Energy.     a = (re / N) >> 8, b = (im / N) >> 8 (the division truncates toward zero, the shift is arithmetic), |a|, |b| <= 2^23;
//               e = a^2 + b^2 < 2^47.  The division by N makes bins of different lengths comparable.
//   Bin gate.   A pure tone of amplitude A gives e = 1024 A^2 against a span energy of L A^2 / 2.  A bin COUNTS in a frame if
//               e L >= e_k (< 2^47 2^15 = 2^62: uint64): it holds at least 1 / 2048 (-33 dB) of what a tone of the whole frame's power
//               would give.  What lies under it is the window's leakage and the tables' rounding -- all that a constant (DC) leaves.
//   Totals.     B[b] = the sum of the counting e over the sounding frames < 2^47 2^8 = 2^55 (K <= 256); C[p] = the sum of B[b] over
//               the bins with n mod 12 = p < 2^55 2^7 = 2^62 (at most 96 bins): uint64.  The device writes integers only: C, frames,
//               sounding, B.
//   Finish.     host, double, serial loops in one written order (zl_ky_finish): Pearson's r of C with the 24 rotations of the
//               Krumhansl-Kessler profiles, 12 majors by tonic, then 12 minors; the best and the runner-up, equal values to the smaller
//               index.  No frames, no sounding frame or a constant chroma: "no key", tonic = -1 and every other field 0 except frames.
//
// The correlate launch's work items are (request, frame, group of ZL_KY_ITEM_BINS bins), numbered over the call; within an item
// ZL_KY_BIN_LANES lanes share a bin and stride j (zl_ky_lane_range): the sums are order-free.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_pitch.h"
#include "zl_types.h"

#define ZL_KY_A4_DEFAULT         440.0f
#define ZL_KY_A4_MIN             220.0f
#define ZL_KY_A4_MAX             880.0f
#define ZL_KY_NOTE_LO_DEFAULT    36          // C2
#define ZL_KY_NOTE_HI_DEFAULT    95          // B6
#define ZL_KY_NOTE_MAX           127
#define ZL_KY_Q_DEFAULT          34          // a Hann main lobe of 4 / N cycles per sample = f 4 / q: narrower than a semitone's 0.1189 f
#define ZL_KY_Q_MAX              256
#define ZL_KY_HOP_DEFAULT        8192
#define ZL_KY_HOP_MAX            (1 << 24)
#define ZL_KY_GATE_DEFAULT       ZL_PT_GATE_DEFAULT
#define ZL_KY_GATE_MAX           ZL_PT_GATE_MAX
#define ZL_KY_FRAMES_DEFAULT     256
#define ZL_KY_MAX_FRAMES         256         // per request: B < 2^55
#define ZL_KY_MAX_CALL_FRAMES    65536       // per call
#define ZL_KY_MAX_BINS           96          // C < 2^62
#define ZL_KY_SPAN_MAX           32768       // the largest N: j < 2^15
#define ZL_KY_SPAN_MIN           32          // the smallest: wstep <= 2^27, and a lane each of a bin's ZL_KY_BIN_LANES has a term
#define ZL_KY_TABLE              4096
#define ZL_KY_ITEM_BINS          8           // bins of a work item
#define ZL_KY_BIN_LANES          32          // lanes that share a bin
#define ZL_KY_CHUNK              2048        // samples staged at a time

// zlhip_key_bin's layout
struct ZlKyBin { int32_t note, n; uint32_t step, wstep; };

// the defaults of the fields given as 0 and the limits that need no sound; the only place they are written.  0 = valid, -1 = not
inline int zl_ky_resolve(double sample_rate, int32_t *hop, int32_t *max_frames, float *a4, int32_t *note_lo, int32_t *note_hi, int32_t *q, int32_t *gate)
{
    if (!(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    if (*a4 == 0.0f) *a4 = ZL_KY_A4_DEFAULT;
    if (*note_lo == 0) *note_lo = ZL_KY_NOTE_LO_DEFAULT;
    if (*note_hi == 0) *note_hi = ZL_KY_NOTE_HI_DEFAULT;
    if (*q == 0) *q = ZL_KY_Q_DEFAULT;
    if (*hop == 0) *hop = ZL_KY_HOP_DEFAULT;
    if (*max_frames == 0) *max_frames = ZL_KY_FRAMES_DEFAULT;
    if (*gate == 0) *gate = ZL_KY_GATE_DEFAULT;
    if (!(*a4 >= ZL_KY_A4_MIN && *a4 <= ZL_KY_A4_MAX)) return -1;                                          // (NaN and inf fail here)
    if (*note_lo < 1 || *note_hi > ZL_KY_NOTE_MAX || *note_lo > *note_hi || *note_hi - *note_lo + 1 > ZL_KY_MAX_BINS) return -1;
    if (*q < 1 || *q > ZL_KY_Q_MAX || *hop < 1 || *hop > ZL_KY_HOP_MAX || *gate < 1 || *gate > ZL_KY_GATE_MAX) return -1;
    if (*max_frames < 1 || *max_frames > ZL_KY_MAX_FRAMES) return -1;
    const double top = (double)*a4 * exp2(((double)*note_hi - 69.0) / 12.0);
    if (!(top < sample_rate / 2.0)) return -1;
    if (rint((double)*q * sample_rate / top) < (double)ZL_KY_SPAN_MIN) return -1;
    return 0;
}

// the table of a resolved request: bins [note_hi - note_lo + 1], T [ZL_KY_TABLE] (either may be null).  Host, double
inline void zl_ky_design(double sample_rate, float a4, int32_t note_lo, int32_t note_hi, int32_t q, ZlKyBin *bins, int16_t *T)
{
    for (int32_t n = note_lo; bins && n <= note_hi; ++n) {
        const double f = (double)a4 * exp2(((double)n - 69.0) / 12.0);
        int64_t N = (int64_t)rint((double)q * sample_rate / f);
        N += N & 1;
        if (N > ZL_KY_SPAN_MAX) N = ZL_KY_SPAN_MAX;
        ZlKyBin &b = bins[n - note_lo];
        b.note = n; b.n = (int32_t)N;
        b.step = (uint32_t)(int64_t)rint(f / sample_rate * 4294967296.0);
        b.wstep = (uint32_t)(((uint64_t)1 << 32) / (uint64_t)N);
    }
    for (int32_t i = 0; T && i < ZL_KY_TABLE; ++i) T[i] = (int16_t)rint(32767.0 * cos(2.0 * 3.14159265358979323846 * (double)i / (double)ZL_KY_TABLE));
}

// K and hop of a region of num_frames frames: zl_pt_frames' rule over a span of L samples
ZL_HD inline void zl_ky_frames(int64_t num_frames, int32_t L, int32_t hop_in, int32_t max_frames, int32_t *K, int32_t *hop)
{
    *hop = hop_in;
    if (num_frames < L) { *K = 0; return; }
    const int64_t k = (num_frames - L) / hop_in + 1;
    if (k <= max_frames) { *K = (int32_t)k; return; }
    *K = max_frames;
    if (max_frames > 1) *hop = (int32_t)((num_frames - L) / (max_frames - 1));
}

// One request of a call as the kernels see it (built by the host)
struct ZlKyRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned)
    uint64_t floor_;             // L channels gate^2: a frame with less energy is silent
    int64_t  acc_base;           // the request's first word pair in the call's accumulator array: frame k's bin b is pair acc_base + k nbins + b
    int32_t  first, hop, frames, channels;       // frames: K
    int32_t  span, nbins;        // L; the bins
    int32_t  bin_base;           // the request's first bin in the call's bin table and per-bin totals
    int32_t  frame_base;         // the request's first frame in the call's per-frame array
    int32_t  item_base;          // the request's first work item of the call
    int32_t  reserved;
};

// what the gate kernel leaves per frame
struct ZlKyStat { uint64_t energy; int32_t silent, reserved; };

// what the correlate kernel leaves per frame and bin
struct ZlKyAcc { int64_t re, im; };

// the result: zlhip_key's layout.  The device writes frames, sounding and chroma and zeroes the rest; the other fields are the host's
struct ZlKyResult {
    int32_t tonic, mode, second_tonic, second_mode, frames, sounding;
    double confidence, second_confidence;
    uint64_t chroma[12];
};

ZL_HD inline int32_t zl_ky_groups(const ZlKyRequest &R) { return (R.nbins + ZL_KY_ITEM_BINS - 1) / ZL_KY_ITEM_BINS; }
ZL_HD inline int32_t zl_ky_items(const ZlKyRequest &R) { return R.frames * zl_ky_groups(R); }
ZL_HD inline int64_t zl_ky_frame_start(const ZlKyRequest &R, int32_t k) { return (int64_t)R.first + (int64_t)k * R.hop; }
ZL_HD inline int32_t zl_ky_bin_off(const ZlKyRequest &R, const ZlKyBin &b) { return (R.span - b.n) >> 1; }

// item i of a request: its frame and its group of bins
ZL_HD inline void zl_ky_item_of(const ZlKyRequest &R, int32_t i, int32_t *frame, int32_t *group)
{
    const int32_t groups = zl_ky_groups(R);
    *frame = i / groups;
    *group = i - *frame * groups;
}

// What lane `lane` (0 .. ZL_KY_BIN_LANES - 1) of a bin whose window is [off, off + n) of the span sums out of the staged samples
// [c0, c1) of the span: j = *j0, *j0 + ZL_KY_BIN_LANES, ... below *j1 (nothing where *j0 >= *j1).  j mod ZL_KY_BIN_LANES == lane.
ZL_HD inline void zl_ky_lane_range(int32_t off, int32_t n, int32_t c0, int32_t c1, int32_t lane, int32_t *j0, int32_t *j1)
{
    const int32_t lo = (c0 > off ? c0 : off) - off, hi = (c1 < off + n ? c1 : off + n) - off;
    *j0 = lo + ((lane - lo) & (ZL_KY_BIN_LANES - 1));
    *j1 = hi;
}

// the table as the correlate kernel holds it: entry i is T[i] in the low half and T[(i - 1024) mod 4096] in the high half, so that one
// load gives the cosine and the sine of a phase
ZL_HD inline uint32_t zl_ky_pair(const int16_t *T, int32_t i) { return (uint32_t)(uint16_t)T[i] | (uint32_t)(uint16_t)T[(i - 1024) & (ZL_KY_TABLE - 1)] << 16; }
ZL_HD inline int32_t zl_ky_pair_cos(uint32_t p) { return (int32_t)(int16_t)(p & 0xffffu); }
ZL_HD inline int32_t zl_ky_pair_sin(uint32_t p) { return (int32_t)(int16_t)(p >> 16); }

ZL_HD inline uint32_t zl_ky_index(uint32_t step, int32_t j) { return ((uint32_t)j * step) >> 20; }           // (the product modulo 2^32)
ZL_HD inline int32_t zl_ky_window(int32_t t) { return (32767 - t) >> 1; }                                    // t = T[window index]
ZL_HD inline int32_t zl_ky_windowed(int32_t m, int32_t w) { return (m * w) >> 15; }

// one term: sample m at index j of bin b, added to the accumulator.  P: the paired table
ZL_HD inline void zl_ky_term(const uint32_t *P, const ZlKyBin &b, int32_t j, int32_t m, int64_t *re, int64_t *im)
{
    const int32_t v = zl_ky_windowed(m, zl_ky_window(zl_ky_pair_cos(P[zl_ky_index(b.wstep, j)])));
    const uint32_t p = P[zl_ky_index(b.step, j)];
    *re += (int64_t)(v * zl_ky_pair_cos(p));
    *im += (int64_t)(v * zl_ky_pair_sin(p));
}

ZL_HD inline uint64_t zl_ky_energy(int64_t re, int64_t im, int32_t n)
{
    const int64_t a = (re / n) >> 8, b = (im / n) >> 8;
    return (uint64_t)(a * a) + (uint64_t)(b * b);
}

// what a bin adds to its total in a frame of span energy `energy`: e, or nothing under the bin gate
ZL_HD inline uint64_t zl_ky_counted(int64_t re, int64_t im, int32_t n, int32_t span, uint64_t energy)
{
    const uint64_t e = zl_ky_energy(re, im, n);
    return e * (uint64_t)span >= energy ? e : 0;
}

// a frame's bin straight from the definition, by one thread over T itself (the harness's second opinion; m: the span's L mixed samples)
inline void zl_ky_bin_serial(const int16_t *T, const ZlKyBin &b, const int32_t *m, int32_t off, int64_t *re, int64_t *im)
{
    int64_t r = 0, i = 0;
    for (int32_t j = 0; j < b.n; ++j) {
        const int32_t w = (32767 - (int32_t)T[((uint32_t)j * b.wstep) >> 20]) >> 1;
        const int32_t v = (m[off + j] * w) >> 15;
        const uint32_t ph = (uint32_t)j * b.step;
        r += (int64_t)v * (int64_t)T[ph >> 20];
        i += (int64_t)v * (int64_t)T[(ph - 0x40000000u) >> 20];
    }
    *re = r; *im = i;
}

// the fold of one request by one thread: the per-bin totals B [nbins] and the integer result
inline void zl_ky_fold_serial(const ZlKyRequest &R, const ZlKyBin *bins, const ZlKyStat *stat, const ZlKyAcc *acc, uint64_t *B, ZlKyResult *out)
{
    ZlKyResult o;
    o.tonic = 0; o.mode = 0; o.second_tonic = 0; o.second_mode = 0; o.frames = R.frames; o.sounding = 0; o.confidence = 0.0; o.second_confidence = 0.0;
    for (int p = 0; p < 12; ++p) o.chroma[p] = 0;
    for (int32_t k = 0; k < R.frames; ++k) o.sounding += stat[k].silent ? 0 : 1;
    for (int32_t b = 0; b < R.nbins; ++b) {
        uint64_t t = 0;
        for (int32_t k = 0; k < R.frames; ++k)
            if (!stat[k].silent) t += zl_ky_counted(acc[(int64_t)k * R.nbins + b].re, acc[(int64_t)k * R.nbins + b].im, bins[b].n, R.span, stat[k].energy);
        B[b] = t;
        o.chroma[bins[b].note % 12] += t;
    }
    *out = o;
}

// Krumhansl and Kessler's probe-tone profiles
static const double kZlKyMajor[12] = {6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88};
static const double kZlKyMinor[12] = {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17};

// Pearson's r of the chroma with candidate i (0 .. 11: major with tonic i; 12 .. 23: minor with tonic i - 12); mx, sxx: the chroma's mean
// and its sum of squared deviations.  Serial, in index order (host, double, one IEEE operation per operator: build without contraction)
inline double zl_ky_correlation(const double *x, double mx, double sxx, int32_t i)
{
    const double *prof = i < 12 ? kZlKyMajor : kZlKyMinor;
    const int32_t tonic = i % 12;
    double y[12], my = 0.0, sxy = 0.0, syy = 0.0;
    for (int p = 0; p < 12; ++p) { y[p] = prof[(p - tonic + 12) % 12]; my += y[p]; }
    my /= 12.0;
    for (int p = 0; p < 12; ++p) { sxy += (x[p] - mx) * (y[p] - my); syy += (y[p] - my) * (y[p] - my); }
    return sxy / sqrt(sxx * syy);
}

// tonic, mode, confidence and the runner-up from the integer record
inline void zl_ky_finish(ZlKyResult *r)
{
    r->tonic = -1; r->mode = 0; r->second_tonic = 0; r->second_mode = 0; r->confidence = 0.0; r->second_confidence = 0.0;
    double x[12], mx = 0.0, sxx = 0.0;
    for (int p = 0; p < 12; ++p) { x[p] = (double)r->chroma[p]; mx += x[p]; }
    mx /= 12.0;
    for (int p = 0; p < 12; ++p) sxx += (x[p] - mx) * (x[p] - mx);
    if (r->frames == 0 || r->sounding == 0 || !(sxx > 0.0)) {
        r->sounding = 0;
        for (int p = 0; p < 12; ++p) r->chroma[p] = 0;
        return;
    }
    double rr[24];
    int32_t best = 0, second = -1;
    for (int32_t i = 0; i < 24; ++i) { rr[i] = zl_ky_correlation(x, mx, sxx, i); if (rr[i] > rr[best]) best = i; }
    for (int32_t i = 0; i < 24; ++i) if (i != best && (second < 0 || rr[i] > rr[second])) second = i;
    r->tonic = best % 12; r->mode = best / 12; r->confidence = rr[best];
    r->second_tonic = second % 12; r->second_mode = second / 12; r->second_confidence = rr[second];
}

// How many semitones to move a clip in (clip_tonic, clip_mode) so that it sits in (tonic, mode): where the modes differ the clip is
// compared through its relative key (major: tonic + 9, minor: tonic + 3).  Always in [-6, 5]
ZL_HD inline int32_t zl_ky_match_shift(int32_t clip_tonic, int32_t clip_mode, int32_t tonic, int32_t mode)
{
    const int32_t from = clip_mode == mode ? clip_tonic : (clip_tonic + (clip_mode == 0 ? 9 : 3)) % 12;
    return ((tonic - from + 6 + 12) % 12) - 6;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_key.hip; 0 or a hipError_t value).  bins [call bins], P [ZL_KY_TABLE] the paired table (zl_ky_pair), stat [call frames], acc [call frames x bins],
// totals [call bins]; out [nreq] may be host memory mapped into the device: only the records are written
int zl_launch_key_gate(const ZlKyRequest *reqs, int32_t nreq, int64_t frames, ZlKyStat *stat, hipStream_t s);
int zl_launch_key_correlate(const ZlKyRequest *reqs, int32_t nreq, int64_t items, const ZlKyBin *bins, const uint32_t *P, const ZlKyStat *stat, ZlKyAcc *acc, hipStream_t s);
int zl_launch_key_fold(const ZlKyRequest *reqs, int32_t nreq, const ZlKyBin *bins, const ZlKyStat *stat, const ZlKyAcc *acc, uint64_t *totals, ZlKyResult *out, hipStream_t s);
#endif
