// zl_tempo.h -- a clip's tempo, estimated on the device (zlhip_sound_tempo / _batch): how fast a loop is, so that
// a sampler can fit it to the session (ClipAudioSource_setLength(beat, bpm) and _setSpeedRatio both take a tempo the caller must know).
// The reference has no tempo estimate, so this is a build-defined extension and claims no parity.  Shared by the HIP kernels
// (zl_tempo.hip), the engine and a host build for the CPU tier (tests/cpu_harness/tempo_host.cpp): everything is defined HERE, once,
// and everything behind section 12's quantisation is integer arithmetic, so every reduction order gives the same bits.
//
// A request is (sound, first_frame, num_frames, hop, bpm_min, bpm_max) over the sound's current playback data.
//
//   Energy.     E[h] is section 12's (zl_onset.h): the sum of zl_st_q(v)^2 over the hop's frames and channels as uint64.
//   Flux.       R[h] = floor(sqrt(E[h])) exactly (zl_tp_isqrt), R[-1] = 0; s = max(0, bitlength(max R) - 16);
//               W[h] = max(0, R[h] - R[h-1]) >> s < 2^16; S = sum of W.  (The amplitude domain on purpose: section 12's log level
//               weighs a hi-hat almost like a kick.)
//   Lags.       l_min = max(1, ceil(60 rate / (hop bpm_max))), l_max = floor(60 rate / (hop bpm_min)), one double division each
//               (zl_tp_lags); cap = (hops - 1) / 2; l_max = min(l_max, cap).
//   Acf.        A[l] = sum over h in [l, hops) of W[h] W[h-l] as uint64, for l = 0 and l in [max(1, l_min - 1), min(8 l_max + 8, cap + 1)];
//               A[l] <= (hops - l) (2^16 - 1)^2.
//   Order.      lag a beats lag b iff A[a] (hops - b) > A[b] (hops - a) in uint64 (the unbiased estimates A / (hops - l) compared
//               without a division; both products stay below 2^64); equal goes to the smaller lag (zl_tp_beats).
//   Coarse.     l* = the best lag in [l_min, l_max].
//   Doublings.  m = l*, K = 0; while K < 3 and 2m + 1 <= cap: m = the best of {2m-1, 2m, 2m+1}, K += 1.
//   No tempo.   l_min > l_max (the clip is too short for the range) or A[0] == 0 (silence): every field 0 except hops, shift, sum and
//               acf_zero.  Not an error.
//   Result.     the device writes integers only (ZlTpResult); the host derives bpm and confidence in double (zl_tp_finish).
//
// The acf is evaluated in work items (request, tile of ZL_TP_TILE lags, segment of at most ZL_TP_SEG hops), numbered over the call:
// zl_tp_item_of, zl_tp_h_index and zl_tp_l_index say which hops an item stages; an index outside [0, hops) is a produced zero.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_onset.h"
#include "zl_types.h"

#define ZL_TP_BPM_MIN_DEFAULT    75.0f
#define ZL_TP_BPM_MAX_DEFAULT    150.0f
#define ZL_TP_BPM_LO             20.0f
#define ZL_TP_BPM_HI             400.0f
#define ZL_TP_MAX_LAG            1024        // l_max before the cut to cap
#define ZL_TP_MAX_DOUBLINGS      3
#define ZL_TP_MAX_LAGS           (8 * ZL_TP_MAX_LAG + 8)   // the largest lag evaluated
#define ZL_TP_MAX_HOPS           ZL_ON_MAX_HOPS
#define ZL_TP_MAX_CALL_HOPS      ZL_ON_MAX_CALL_HOPS
#define ZL_TP_TILE               256         // lags of a work item: one lane each
#define ZL_TP_SEG                4096        // hops of a work item

// floor(sqrt(x)), exact for x < 2^62: the double root, then steps of one until r^2 <= x < (r + 1)^2
ZL_HD inline uint64_t zl_tp_isqrt(uint64_t x)
{
    uint64_t r = (uint64_t)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

ZL_HD inline int32_t zl_tp_bitlength(uint64_t x) { return x ? 64 - zl_on_clz64(x) : 0; }

ZL_HD inline int32_t zl_tp_shift(uint64_t rmax) { const int32_t b = zl_tp_bitlength(rmax) - 16; return b > 0 ? b : 0; }

// W[h] from R[h], R[h-1] (0 for h == 0) and s
ZL_HD inline uint32_t zl_tp_flux(uint64_t r, uint64_t rprev, int32_t shift) { return r > rprev ? (uint32_t)((r - rprev) >> shift) : 0u; }

// l_min and l_max before the cut to cap (host): the only place the two divisions are written
inline void zl_tp_lags(double sample_rate, int32_t hop, float bpm_min, float bpm_max, double *lmin, double *lmax)
{
    const double a = ceil((60.0 * sample_rate) / ((double)hop * (double)bpm_max));
    *lmin = a < 1.0 ? 1.0 : a;
    *lmax = floor((60.0 * sample_rate) / ((double)hop * (double)bpm_min));
}

// the defaults of the fields given as 0 and the limits that need no sound; the only place they are written.  0 = valid, -1 = not
inline int zl_tp_resolve(double sample_rate, int32_t *hop, float *bpm_min, float *bpm_max)
{
    if (!(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    int32_t gate = 1, threshold = 1, min_gap = 1, max_onsets = 1;
    if (zl_on_resolve(sample_rate, hop, &gate, &threshold, &min_gap, &max_onsets) != 0) return -1;
    if (*bpm_min == 0.0f) *bpm_min = ZL_TP_BPM_MIN_DEFAULT;
    if (*bpm_max == 0.0f) *bpm_max = ZL_TP_BPM_MAX_DEFAULT;
    if (!(*bpm_min >= ZL_TP_BPM_LO && *bpm_min < *bpm_max && *bpm_max <= ZL_TP_BPM_HI)) return -1;        // (NaN and inf fail here)
    double lmin, lmax;
    zl_tp_lags(sample_rate, *hop, *bpm_min, *bpm_max, &lmin, &lmax);
    if (lmax > (double)ZL_TP_MAX_LAG) return -1;
    return 0;
}

// One request of a call as the flux, acf and pick kernels see it (built by the host; the energy pass takes a ZlOnRequest)
struct ZlTpRequest {
    int32_t hops;
    int32_t hop_base;            // the request's first hop in the call's E / W arrays
    int32_t lmin, lmax, cap;     // l_max already cut to cap; l_min > l_max: no tempo
    int32_t first_lag, nlags;    // the lags besides 0 that are evaluated: [first_lag, first_lag + nlags), nlags 0 where there is no tempo
    int32_t acf_base;            // the request's A[first_lag] in the call's A array
    int32_t item_base;           // the request's first work item of the call
    int32_t nsegs;               // its segments of ZL_TP_SEG hops; items = ceil(nlags / ZL_TP_TILE) * nsegs
};

// what the flux kernel leaves per request for the pick kernel
struct ZlTpStat { uint64_t acf_zero, sum; int32_t shift, pad; };

// the result as the device writes it: the layout of zlhip_tempo (bpm and confidence are the host's)
struct ZlTpResult {
    float bpm, confidence;
    int32_t lag_coarse, lag_fine, doublings, shift, hops, reserved;
    uint64_t acf_lo, acf_mid, acf_hi, acf_zero, sum;
};

// the geometry of a request from its hops and the resolved lags (host)
inline void zl_tp_geometry(ZlTpRequest *R, int32_t hops, double lmin, double lmax)
{
    R->hops = hops;
    R->cap = (hops - 1) / 2;
    R->lmin = (int32_t)(lmin > 1e6 ? 1e6 : lmin);
    R->lmax = lmax < (double)R->cap ? (int32_t)lmax : R->cap;
    R->first_lag = R->lmin - 1 > 1 ? R->lmin - 1 : 1;
    const int32_t last = 8 * R->lmax + 8 < R->cap + 1 ? 8 * R->lmax + 8 : R->cap + 1;
    R->nlags = R->lmin > R->lmax || last < R->first_lag ? 0 : last - R->first_lag + 1;
    R->nsegs = (hops + ZL_TP_SEG - 1) / ZL_TP_SEG;
}

ZL_HD inline int32_t zl_tp_tiles(const ZlTpRequest &R) { return (R.nlags + ZL_TP_TILE - 1) / ZL_TP_TILE; }
ZL_HD inline int32_t zl_tp_items(const ZlTpRequest &R) { return zl_tp_tiles(R) * R.nsegs; }

// item i of a request: its tile of lags and its segment of hops (the tiles of one segment are neighbours: they share W[h])
ZL_HD inline void zl_tp_item_of(const ZlTpRequest &R, int32_t i, int32_t *tile, int32_t *seg)
{
    const int32_t tiles = zl_tp_tiles(R);
    *seg = i / tiles;
    *tile = i - *seg * tiles;
}

// the first lag of a tile and the first hop of a segment
ZL_HD inline int32_t zl_tp_tile_lag(const ZlTpRequest &R, int32_t tile) { return R.first_lag + tile * ZL_TP_TILE; }
ZL_HD inline int32_t zl_tp_seg_hop(int32_t seg) { return seg * ZL_TP_SEG; }

// an item none of whose products has h >= l contributes nothing and stages nothing
ZL_HD inline bool zl_tp_item_live(const ZlTpRequest &R, int32_t tile, int32_t seg)
{
    const int32_t h1 = zl_tp_seg_hop(seg) + ZL_TP_SEG < R.hops ? zl_tp_seg_hop(seg) + ZL_TP_SEG : R.hops;
    return h1 - 1 >= zl_tp_tile_lag(R, tile);
}

// the hop staged at word i of the segment's W[h] (i in [0, ZL_TP_SEG)) and at word j of the lagged window (j in [0, ZL_TP_SEG +
// ZL_TP_TILE)): lane `lane` (lag zl_tp_tile_lag + lane) multiplies word i by window word i + ZL_TP_TILE - 1 - lane.  -1: a produced
// zero (before hop 0, or at or behind `hops`); no address is formed for it.
ZL_HD inline int32_t zl_tp_h_index(const ZlTpRequest &R, int32_t seg, int32_t i)
{
    const int32_t h = zl_tp_seg_hop(seg) + i;
    return h < R.hops ? h : -1;
}
ZL_HD inline int32_t zl_tp_l_index(const ZlTpRequest &R, int32_t tile, int32_t seg, int32_t j)
{
    const int32_t h = zl_tp_seg_hop(seg) - zl_tp_tile_lag(R, tile) - (ZL_TP_TILE - 1) + j;
    return h >= 0 && h < R.hops ? h : -1;
}
ZL_HD inline int32_t zl_tp_window_word(int32_t i, int32_t lane) { return i + ZL_TP_TILE - 1 - lane; }

// the order: lag a strictly before lag b (Aa = A[a], Ab = A[b])
ZL_HD inline bool zl_tp_beats(uint64_t Aa, int32_t a, uint64_t Ab, int32_t b, int32_t hops)
{
    const uint64_t x = Aa * (uint64_t)(hops - b), y = Ab * (uint64_t)(hops - a);
    return x > y || (x == y && a < b);
}

// the doublings from the coarse lag on; A: the request's A[first_lag ...].  One lane's work: at most nine comparisons
ZL_HD inline void zl_tp_doublings(const ZlTpRequest &R, const uint64_t *A, int32_t coarse, int32_t *fine, int32_t *K)
{
    int32_t m = coarse, k = 0;
    while (k < ZL_TP_MAX_DOUBLINGS && 2 * m + 1 <= R.cap) {
        int32_t b = 2 * m - 1;
        for (int32_t c = 2 * m; c <= 2 * m + 1; ++c)
            if (zl_tp_beats(A[c - R.first_lag], c, A[b - R.first_lag], b, R.hops)) b = c;
        m = b; ++k;
    }
    *fine = m; *K = k;
}

// the integer record of a request from its statistics, A and the coarse lag (0: none was looked for)
ZL_HD inline void zl_tp_record(const ZlTpRequest &R, const ZlTpStat &st, const uint64_t *A, int32_t coarse, ZlTpResult *out)
{
    ZlTpResult o;
    o.bpm = 0.0f; o.confidence = 0.0f;
    o.lag_coarse = 0; o.lag_fine = 0; o.doublings = 0; o.shift = st.shift; o.hops = R.hops; o.reserved = 0;
    o.acf_lo = 0; o.acf_mid = 0; o.acf_hi = 0; o.acf_zero = st.acf_zero; o.sum = st.sum;
    if (R.lmin <= R.lmax && st.acf_zero != 0) {
        zl_tp_doublings(R, A, coarse, &o.lag_fine, &o.doublings);
        const int32_t m = o.lag_fine;
        o.lag_coarse = coarse;
        o.acf_lo = m - 1 == 0 ? st.acf_zero : A[m - 1 - R.first_lag];
        o.acf_mid = A[m - R.first_lag];
        o.acf_hi = A[m + 1 - R.first_lag];
    }
    *out = o;
}

// bpm and confidence from the integer record (host, double, one IEEE operation per operator: build without contraction)
inline void zl_tp_finish(double sample_rate, int32_t hop, ZlTpResult *r)
{
    r->bpm = 0.0f; r->confidence = 0.0f;
    if (r->lag_fine == 0) return;
    const double m = (double)r->lag_fine, hops = (double)r->hops;
    const double ym = (double)r->acf_lo / (hops - m + 1.0), y0 = (double)r->acf_mid / (hops - m), yp = (double)r->acf_hi / (hops - m - 1.0);
    const double den = (ym - 2.0 * y0) + yp;
    double d = den < 0.0 ? (ym - yp) / (2.0 * den) : 0.0;
    d = d > 0.5 ? 0.5 : (d < -0.5 ? -0.5 : d);
    const double period = (m + d) / (double)(1 << r->doublings);
    const double mu = (double)r->sum / hops, mu2 = mu * mu;
    const double cden = (double)r->acf_zero / hops - mu2;
    r->bpm = (float)((60.0 * sample_rate) / ((double)hop * period));
    r->confidence = cden > 0.0 ? (float)((y0 - mu2) / cden) : 0.0f;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_tempo.hip; 0 or a hipError_t value).  E [call hops] is zl_launch_onset_energy's; W [call hops] uint16; A [call lags];
// stat [nreq]; out [nreq] may be host memory mapped into the device: only the records are written
int zl_launch_tempo_flux(const ZlTpRequest *reqs, int32_t nreq, const uint64_t *E, uint16_t *W, uint64_t *A, ZlTpStat *stat, hipStream_t s);
int zl_launch_tempo_acf(const ZlTpRequest *reqs, int32_t nreq, int64_t items, const uint16_t *W, uint64_t *A, hipStream_t s);
int zl_launch_tempo_pick(const ZlTpRequest *reqs, int32_t nreq, const uint64_t *A, const ZlTpStat *stat, ZlTpResult *out, hipStream_t s);
#endif
