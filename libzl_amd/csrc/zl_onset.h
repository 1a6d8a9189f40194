// zl_onset.h -- a clip's transients, found on the device (zlhip_sound_onsets / _batch): the frames at which a
// sampler slices a loop so that the cuts fall on the hits, not through them.  The reference has no transient detection (its only slice
// table is an even division, lib/ClipAudioSource.cpp:495-528), so this is a build-defined extension and claims no parity.  Shared by the
// HIP kernels (zl_onset.hip), the engine and a host build for the CPU tier (tests/cpu_harness/onset_host.cpp): everything is defined
// HERE, once, and everything behind the quantisation is integer arithmetic, so every reduction order gives the same bits.
//
// A request is (sound, first_frame, num_frames, hop, gate, threshold, min_gap, max_onsets) over the sound's current playback data.
//
//   Quantise.   q = zl_st_q(v) (zl_stretch.h: clamp(rint(4096 v), +-32767), NaN -> 0); per frame e[f] = sum over the channels of q^2.
//   Hops.       hops = ceil(num_frames / hop); hop h covers [first + h*hop, min(first + (h+1)*hop, first + num_frames)); E[h] is the sum
//               of e over it as uint64 (hop <= 4096: below 2^44); E[-1] = 0.
//   Floor.      F = hop * channels * gate^2: silence and noise below the gate read as the level L(F) and cannot trigger.
//   Level.      L(x), x >= 1: a piecewise-linear log2 in 1/64 octaves, p = 63 - clz(x), L = 64 p + floor((x - 2^p) * 64 / 2^p)
//               (zl_on_level: a shift either way, no division).
//   Novelty.    N[h] = max(0, L(E[h] + F) - L(E[h-1] + F)).
//   Candidate.  hop h with N[h] >= threshold, N[h] > N[j] for j in [h - min_gap, h), N[h] >= N[j] for j in (h, h + min_gap], the ranges
//               cut to [0, hops).  Two candidates are therefore always more than min_gap hops apart.
//   Select.     more than max_onsets candidates: the max_onsets with the largest N stay, equal N goes to the smaller h.
//   Refine.     per kept hop h: S = hop / 16, Ep = E[h-1] + F; sub-blocks of S frames from a0 = max(first, first + (h-1)*hop) up to
//               first + (h+1)*hop, cut to the request's end; the onset is the start of the first sub-block whose energy e_s has
//               4 e_s > Ep, else first + h*hop.
//   Output.     (frame, strength = N[h]) in ascending frame order, and the count; frame counts from the sound's first frame.
//
// The windows are evaluated in linear time (zl_on_window): per aligned block of min_gap hops the running maximum from the block's
// start (prefix) and from its end (suffix) are stored; a range of at most min_gap hops is the suffix of one block and the prefix of
// the next.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_overview.h"
#include "zl_stretch.h"
#include "zl_types.h"

#define ZL_ON_HOP_MIN            64
#define ZL_ON_HOP_MAX            4096
#define ZL_ON_GATE_MAX           32767
#define ZL_ON_THRESHOLD_MAX      4096
#define ZL_ON_MIN_GAP_MAX        1024
#define ZL_ON_MAX_ONSETS         1024        // per request
#define ZL_ON_MAX_HOPS           65536       // per request
#define ZL_ON_MAX_CALL_HOPS      (4 << 20)   // per call
#define ZL_ON_SUBBLOCKS          16          // sub-blocks of the refinement per hop
#define ZL_ON_REFINE_FACTOR      4           // (16-frame sub-blocks of a low sine swing to twice their mean energy: 2 is too eager)
#define ZL_ON_LEVELS             (64 * 44)   // every level, hence every N, is below this (E + F < 2^44)
#define ZL_ON_WAVE               64

// the defaults of the fields given as 0 and the limits of all five; the only place they are written.  0 = valid, -1 = not
inline int zl_on_resolve(double sample_rate, int32_t *hop, int32_t *gate, int32_t *threshold, int32_t *min_gap, int32_t *max_onsets)
{
    if ((*hop == 0 || *min_gap == 0) && !(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    if (*hop == 0) {
        double k = rint(sample_rate / 3000.0);
        k = k < 4.0 ? 4.0 : (k > 256.0 ? 256.0 : k);
        *hop = 16 * (int32_t)k;
    }
    if (*hop < ZL_ON_HOP_MIN || *hop > ZL_ON_HOP_MAX || (*hop & 15) != 0) return -1;
    if (*gate == 0) *gate = 8;
    if (*threshold == 0) *threshold = 128;
    if (*min_gap == 0) {
        const double g = ceil(sample_rate / (20.0 * (double)*hop));          // 0.05 * sample_rate / hop
        *min_gap = g < 1.0 ? 1 : (g > 1e6 ? 1000000 : (int32_t)g);
    }
    if (*max_onsets == 0) *max_onsets = 128;
    if (*gate < 1 || *gate > ZL_ON_GATE_MAX || *threshold < 1 || *threshold > ZL_ON_THRESHOLD_MAX) return -1;
    if (*min_gap < 1 || *min_gap > ZL_ON_MIN_GAP_MAX || *max_onsets < 1 || *max_onsets > ZL_ON_MAX_ONSETS) return -1;
    return 0;
}

ZL_HD inline int64_t zl_on_hops(int64_t frames, int64_t hop) { return (frames + hop - 1) / hop; }

ZL_HD inline uint64_t zl_on_floor(int32_t hop, int32_t channels, int32_t gate) { return (uint64_t)hop * (uint64_t)channels * (uint64_t)gate * (uint64_t)gate; }

ZL_HD inline int zl_on_clz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// L(x) for x >= 1
ZL_HD inline int32_t zl_on_level(uint64_t x)
{
    const int p = 63 - zl_on_clz64(x);
    const uint64_t m = x - ((uint64_t)1 << p);
    return (int32_t)(64 * p) + (int32_t)(p >= 6 ? m >> (p - 6) : m << (6 - p));
}

// N[h] from E[h], E[h-1] (0 for h == 0) and F
ZL_HD inline int32_t zl_on_novelty(uint64_t e, uint64_t eprev, uint64_t floor_)
{
    const int32_t d = zl_on_level(e + floor_) - zl_on_level(eprev + floor_);
    return d > 0 ? d : 0;
}

// the energy of one sample
ZL_HD inline uint32_t zl_on_sq(float v) { const int32_t q = zl_st_q(v); return (uint32_t)(q * q); }

// the frames [*lo, *hi) of hop h
ZL_HD inline void zl_on_hop_range(int64_t first, int64_t frames, int64_t hop, int64_t h, int64_t *lo, int64_t *hi)
{
    *lo = first + h * hop;
    *hi = *lo + hop < first + frames ? *lo + hop : first + frames;
}

// (a hop's 16-byte groups and the mask of their elements are the overview's: zl_ov_groups, zl_ov_valid -- what lies outside the hop belongs
// to the neighbouring hop, to the frames around the request or to the zero frames behind the extent)

// ---- windows in linear time --------------------------------------------------------------------------------------------------------
// ps[h] = prefix | suffix << 16: the maximum of N over [block start, h] and over [h, block end], blocks of `gap` hops from hop 0, the
// last one cut at `hops` (N < 2^12).  One block: the work of one thread.
ZL_HD inline void zl_on_scan_block(const int32_t *N, uint32_t *ps, int32_t hops, int32_t gap, int32_t block)
{
    const int32_t b0 = block * gap, b1 = b0 + gap < hops ? b0 + gap : hops;
    int32_t m = 0;
    for (int32_t h = b0; h < b1; ++h) { m = N[h] > m ? N[h] : m; ps[h] = (uint32_t)m; }
    m = 0;
    for (int32_t h = b1 - 1; h >= b0; --h) { m = N[h] > m ? N[h] : m; ps[h] |= (uint32_t)m << 16; }
}

// the maximum of N over [a, b], 0 <= a <= b < hops, where the range holds `gap` hops or fewer and, if fewer, starts at 0 or ends at hops - 1
ZL_HD inline int32_t zl_on_window(const uint32_t *ps, int32_t gap, int32_t a, int32_t b)
{
    const int32_t suffix = (int32_t)(ps[a] >> 16), prefix = (int32_t)(ps[b] & 0xffffu);
    if (a / gap != b / gap) return suffix > prefix ? suffix : prefix;
    return a % gap == 0 ? prefix : suffix;             // inside one block: the range starts with the block or ends with it
}

ZL_HD inline bool zl_on_candidate(const int32_t *N, const uint32_t *ps, int32_t hops, int32_t gap, int32_t threshold, int32_t h)
{
    const int32_t n = N[h];
    if (n < threshold) return false;
    if (h > 0 && !(n > zl_on_window(ps, gap, h - gap > 0 ? h - gap : 0, h - 1))) return false;
    if (h + 1 < hops && !(n >= zl_on_window(ps, gap, h + 1, h + gap < hops - 1 ? h + gap : hops - 1))) return false;
    return true;
}

// ---- select ------------------------------------------------------------------------------------------------------------------------
// hist[s]: candidates of strength s.  The cut-off strength s* of the top max_onsets and how many of strength s* stay (the earliest);
// everything above s* stays.  Fewer candidates than max_onsets: s* = 0 (no candidate has N = 0: threshold >= 1).
ZL_HD inline void zl_on_cutoff(const uint32_t *hist, int32_t max_onsets, int32_t *cut, int32_t *quota)
{
    uint32_t above = 0;
    for (int32_t s = ZL_ON_LEVELS - 1; s >= 1; --s) {
        if (above + hist[s] >= (uint32_t)max_onsets) { *cut = s; *quota = max_onsets - (int32_t)above; return; }
        above += hist[s];
    }
    *cut = 0; *quota = 0;
}

// ---- refine ------------------------------------------------------------------------------------------------------------------------
// sub-block s of kept hop h: the frames [*lo, *hi), empty (false) behind the walk's or the request's end
ZL_HD inline bool zl_on_subblock(int64_t first, int64_t frames, int32_t hop, int32_t h, int32_t s, int64_t *lo, int64_t *hi)
{
    const int64_t S = hop / ZL_ON_SUBBLOCKS, end = first + frames;
    const int64_t a0 = h > 0 ? first + (int64_t)(h - 1) * hop : first, stop = first + (int64_t)(h + 1) * hop;
    *lo = a0 + s * S;
    *hi = *lo + S < end ? *lo + S : end;
    return *lo < stop && *lo < end;
}

ZL_HD inline bool zl_on_hit(uint64_t es, uint64_t eprev_plus_floor) { return ZL_ON_REFINE_FACTOR * es > eprev_plus_floor; }

// One request of a call as the kernels see it (built by the host)
struct ZlOnRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned)
    uint64_t floor_;             // F
    int32_t  first, frames, hop, channels;
    int32_t  hops;
    int32_t  hop_base;           // the request's first hop in the call's E / N / ps arrays
    int32_t  threshold, min_gap, max_onsets;
    int32_t  out_base;           // the request's first onset in the call's packed output (the sum of the max_onsets before it)
};

struct ZlOnOnset { int32_t frame, strength; };

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_onset.hip; 0 or a hipError_t value).  E [call hops] uint64, N [call hops], ps [call hops]; counts [nreq] and
// out [sum of max_onsets] may be host memory mapped into the device: only a request's count and its onsets are written
int zl_launch_onset_energy(const ZlOnRequest *reqs, int32_t nreq, int64_t hops, uint64_t *E, hipStream_t s);
int zl_launch_onset_pick(const ZlOnRequest *reqs, int32_t nreq, const uint64_t *E, int32_t *N, uint32_t *ps, int32_t *counts, ZlOnOnset *out, hipStream_t s);
#endif
