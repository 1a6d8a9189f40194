// zl_loop.h -- a clip's seamless loop points, found on the device (zlhip_sound_loop / _batch): where a sampler's
// sustain loop can wrap from its stop to its start without a click (ClipCommand.looping; ClipAudioSource_setStartPosition / _setLength
// take seconds and beats the caller must already know).  The reference has no loop finder, so this is a build-defined extension and
// claims no parity.  Shared by the HIP kernels (zl_loop.hip), the engine and a host build for the CPU tier
// (tests/cpu_harness/loop_host.cpp): everything is defined HERE, once.  Behind section 8's 16-bit quantisation everything is integer
// arithmetic and the order of two pairs is total, so every reduction order gives the same pair.
//
// A request is (sound, start_frame s0, stop_frame e0, start_search Rs, stop_search Re, window W, min_length) over the sound's current
// playback data of `length` frames; the nominal loop is [s0, e0), 0 <= s0 < e0 <= length.
//
//   Defaults.   (zl_lp_resolve, the only place they are written) Rs, Re given as 0: min(2047, rint(0.010 rate)); -1: "this point stays",
//               the range is the nominal point alone; at most 2047.  W given as 0: 256; a multiple of 16 in [16, 1024]; H = W / 2.
//               min_length given as 0: W; at least 1.
//   Candidates. starts s in [max(s0 - Rs, H), min(s0 + Rs, length - H)], ends e in [max(e0 - Re, H), min(e0 + Re, length - H)]: the
//               window [p - H, p + H) of a candidate lies inside the data.  ns, ne: how many.  A pair (s, e) is ADMISSIBLE if
//               e - s >= min_length.  An empty range or no admissible pair: found = 0 and every other field 0, not an error.
//               (A loop over the whole file has its points inside H of the data's ends, so its candidates begin H frames in: the
//               service is meant for sustain loops inside a sound, not for beat loops that trust the file's edges.)
//   Mono mix.   m[f] = the sum over the channels of zl_st_q(v), as in zl_pitch.h; NaN -> 0.
//   Shift.      one per request: maxabs = the largest |m| over the two strips [smin - H, smax + H) and [emin - H, emax + H);
//               sh = max(0, bitlength(maxabs) - 10); x = m >> sh (arithmetic), |x| <= 2^10.
//   Cost.       cost(s, e) = the sum over j in [-H, H) of (x[s + j] - x[e + j])^2: the frames behind the jump should be what would
//               have followed e, the frames in front of s what preceded e.  A term is below 2^22 and W <= 2^10: cost < 2^32 (uint32).
//               E(p) = the sum of x[p + j]^2 over the window (<= 2^30); den(s, e) = E(s) + E(e) + 1 <= 2^31 + 1.
//   Order.      pair a is better than pair b under the first rule that differs: cost_a den_b < cost_b den_a (exact in uint64); the
//               smaller |s - s0| + |e - e0|; the smaller s; the smaller e (zl_lp_better).
//   Result.     integers only from the device (ZlLpResult): found, start_frame, stop_frame, shift, starts, ends, pairs (the admissible
//               pairs), cost, den, nominal_valid (1 when (s0, e0) is itself an admissible candidate pair), nominal_cost, nominal_den.
//   Finish.     host, double (zl_lp_finish): seam_db = -120 where cost == 0, else max(-120, 10 log10(cost / den)); nominal_db the same
//               way; improvement_db = nominal_db - seam_db, or 0 without a nominal.
//   Seconds.    zl_lp_seconds: the float seconds from which the voice derives exactly these frames.
//
// The costs are evaluated in work items (request, tile of ZL_LP_TILE starts x ZL_LP_TILE ends), numbered over the call; zl_lp_item_of
// says which.  A strip of a request is stored as int16 from its first frame p_min - H on: candidate c (counted from p_min) has its
// window at the strip's elements [c, c + W).
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_pitch.h"
#include "zl_types.h"

#define ZL_LP_SEARCH_SECONDS     0.010
#define ZL_LP_SEARCH_MAX         2047
#define ZL_LP_WINDOW_DEFAULT     256
#define ZL_LP_WINDOW_MIN         16
#define ZL_LP_WINDOW_MAX         1024
#define ZL_LP_BITS               10          // |x| <= 2^10
#define ZL_LP_TILE               64          // starts and ends of a work item
#define ZL_LP_LANE               4           // starts and ends of a lane's register tile
#define ZL_LP_MAX_CALL_ITEMS     65536       // per call
#define ZL_LP_MAX_CALL_STRIP     4194304     // strip frames per call (each strip rounded up to ZL_LP_STRIP_ALIGN)
#define ZL_LP_STRIP_ALIGN        8
#define ZL_LP_MAX_COST_PAIRS     1048576     // a call with at most this many candidate pairs also stores every cost (debug)
#define ZL_LP_STAGE              (ZL_LP_TILE + ZL_LP_WINDOW_MAX)           // int16 of a staged strip tile: 64 + W at most
#define ZL_LP_DB_FLOOR           (-120.0)

// the defaults of the fields given as 0 and the limits that need no sound; the only place they are written.  0 = valid, -1 = not
inline int zl_lp_resolve(double sample_rate, int32_t *rs, int32_t *re, int32_t *window, int32_t *min_length)
{
    if (!(sample_rate > 0.0 && sample_rate < 1e9)) return -1;
    const double d = rint(ZL_LP_SEARCH_SECONDS * sample_rate);
    const int32_t def = d > (double)ZL_LP_SEARCH_MAX ? ZL_LP_SEARCH_MAX : (d < 1.0 ? 1 : (int32_t)d);
    if (*rs == 0) *rs = def;
    if (*re == 0) *re = def;
    if (*window == 0) *window = ZL_LP_WINDOW_DEFAULT;
    if (*rs < -1 || *rs > ZL_LP_SEARCH_MAX || *re < -1 || *re > ZL_LP_SEARCH_MAX) return -1;
    if (*window < ZL_LP_WINDOW_MIN || *window > ZL_LP_WINDOW_MAX || (*window & 15) != 0) return -1;
    if (*min_length == 0) *min_length = *window;
    if (*min_length < 1) return -1;
    return 0;
}

// the candidates of one point: [*lo, *lo + *n) around the nominal p0 with search radius r (-1: the nominal alone)
ZL_HD inline void zl_lp_range(int32_t p0, int32_t r, int32_t H, int32_t length, int32_t *lo, int32_t *n)
{
    const int64_t rr = r < 0 ? 0 : r;
    int64_t a = (int64_t)p0 - rr, b = (int64_t)p0 + rr;
    if (a < H) a = H;
    if (b > (int64_t)length - H) b = (int64_t)length - H;
    *lo = (int32_t)a;
    *n = b >= a ? (int32_t)(b - a + 1) : 0;
}

// One request of a call as the kernels see it (built by the host)
struct ZlLpRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned)
    int64_t  cost_base;          // the request's first word in the call's cost matrix [ns][ne] (debug; where the call stores one)
    int32_t  s0, e0;             // the nominal loop
    int32_t  smin, ns, emin, ne; // the candidates
    int32_t  window, min_length, channels;
    int32_t  xs_base, xe_base;   // the strips' first elements in the call's int16 array (multiples of ZL_LP_STRIP_ALIGN)
    int32_t  es_base, ee_base;   // the candidates' first words in the call's E array
    int32_t  item_base;          // the request's first work item of the call
};

// a pair with its cost; s < 0: none
struct ZlLpPair { int32_t s, e; uint32_t cost, den; };

// what the pairs kernel leaves per item (zlhip_loop_item's layout): the item's best admissible pair (none: start = stop = -1, cost = den = 0)
struct ZlLpItem { int32_t start, stop; uint32_t cost, den; uint64_t pairs; };

// the result as the device writes it: the layout of zlhip_loop (the three doubles are the host's)
struct ZlLpResult {
    int32_t found, start_frame, stop_frame, shift, starts, ends, nominal_valid, reserved;
    uint64_t pairs;
    uint32_t cost, den, nominal_cost, nominal_den;
    double seam_db, nominal_db, improvement_db;
};

ZL_HD inline int32_t zl_lp_strip_len(int32_t n, int32_t window) { return n > 0 ? n - 1 + window : 0; }
ZL_HD inline int32_t zl_lp_strip_room(int32_t n, int32_t window) { return (zl_lp_strip_len(n, window) + ZL_LP_STRIP_ALIGN - 1) / ZL_LP_STRIP_ALIGN * ZL_LP_STRIP_ALIGN; }
ZL_HD inline int32_t zl_lp_tiles(int32_t n) { return (n + ZL_LP_TILE - 1) / ZL_LP_TILE; }
ZL_HD inline int32_t zl_lp_items(const ZlLpRequest &R) { return zl_lp_tiles(R.ns) * zl_lp_tiles(R.ne); }

// item i of a request: its tile of starts and its tile of ends (the tiles of one start tile are neighbours)
ZL_HD inline void zl_lp_item_of(const ZlLpRequest &R, int32_t i, int32_t *ts, int32_t *te)
{
    const int32_t tiles = zl_lp_tiles(R.ne);
    *ts = i / tiles;
    *te = i - *ts * tiles;
}

// lane `lane` of a 256-lane item owns the starts 4 (lane & 15) .. + 3 and the ends 4 (lane >> 4) .. + 3 of the tile
ZL_HD inline int32_t zl_lp_lane_start(int32_t lane) { return ZL_LP_LANE * (lane & 15); }
ZL_HD inline int32_t zl_lp_lane_end(int32_t lane) { return ZL_LP_LANE * (lane >> 4); }

ZL_HD inline int32_t zl_lp_shift(uint32_t maxabs) { const int32_t b = zl_pt_bitlength(maxabs) - ZL_LP_BITS; return b > 0 ? b : 0; }

ZL_HD inline uint32_t zl_lp_term(int32_t a, int32_t b) { const int32_t d = a - b; return (uint32_t)(d * d); }
// the same cost from the cross term X (what the pairs kernel sums: one dot2 per two terms) = the sum of x[s + j] x[e + j] (|X| <= 2^30): E(s) + E(e) - 2 X, exact modulo 2^32 and the cost is below 2^32
ZL_HD inline uint32_t zl_lp_cost_from_dot(uint32_t es, uint32_t ee, int32_t X) { return es + ee - 2u * (uint32_t)X; }
ZL_HD inline uint32_t zl_lp_den(uint32_t es, uint32_t ee) { return es + ee + 1u; }
ZL_HD inline bool zl_lp_admissible(int32_t s, int32_t e, int32_t min_length) { return (int64_t)e - (int64_t)s >= (int64_t)min_length; }

// cost and energy straight from the strips (cs, ce: candidates counted from smin, emin)
ZL_HD inline uint32_t zl_lp_cost(const int16_t *xs, const int16_t *xe, int32_t cs, int32_t ce, int32_t window)
{
    uint32_t acc = 0;
    for (int32_t j = 0; j < window; ++j) acc += zl_lp_term((int32_t)xs[cs + j], (int32_t)xe[ce + j]);
    return acc;
}
ZL_HD inline uint32_t zl_lp_energy(const int16_t *x, int32_t c, int32_t window)
{
    uint32_t acc = 0;
    for (int32_t j = 0; j < window; ++j) acc += (uint32_t)((int32_t)x[c + j] * (int32_t)x[c + j]);
    return acc;
}

ZL_HD inline int32_t zl_lp_abs(int32_t v) { return v < 0 ? -v : v; }

// THE order: is pair a better than pair b?  Total (no two different pairs are equal), so every reduction order gives the same pair
ZL_HD inline bool zl_lp_better(const ZlLpPair &a, const ZlLpPair &b, int32_t s0, int32_t e0)
{
    if (a.s < 0) return false;
    if (b.s < 0) return true;
    const uint64_t l = (uint64_t)a.cost * (uint64_t)b.den, r = (uint64_t)b.cost * (uint64_t)a.den;       // both below 2^64
    if (l != r) return l < r;
    const int32_t da = zl_lp_abs(a.s - s0) + zl_lp_abs(a.e - e0), db = zl_lp_abs(b.s - s0) + zl_lp_abs(b.e - e0);
    if (da != db) return da < db;
    if (a.s != b.s) return a.s < b.s;
    return a.e < b.e;
}

ZL_HD inline ZlLpPair zl_lp_no_pair() { ZlLpPair p; p.s = -1; p.e = -1; p.cost = 0; p.den = 0; return p; }

ZL_HD inline ZlLpItem zl_lp_item_record(const ZlLpPair &best, uint64_t pairs)
{
    ZlLpItem o;
    o.start = best.s < 0 ? -1 : best.s; o.stop = best.s < 0 ? -1 : best.e;
    o.cost = best.s < 0 ? 0u : best.cost; o.den = best.s < 0 ? 0u : best.den; o.pairs = pairs;
    return o;
}

// is the nominal pair itself an admissible candidate pair?
ZL_HD inline bool zl_lp_nominal_valid(const ZlLpRequest &R)
{
    return R.ns > 0 && R.ne > 0 && R.s0 >= R.smin && R.s0 < R.smin + R.ns && R.e0 >= R.emin && R.e0 < R.emin + R.ne && zl_lp_admissible(R.s0, R.e0, R.min_length);
}

// the integer result from the reduction's outcome
ZL_HD inline void zl_lp_result(const ZlLpRequest &R, const ZlLpPair &best, uint64_t pairs, int32_t shift, bool nominal, uint32_t ncost, uint32_t nden, ZlLpResult *out)
{
    ZlLpResult o;
    o.found = 0; o.start_frame = 0; o.stop_frame = 0; o.shift = 0; o.starts = 0; o.ends = 0; o.nominal_valid = 0; o.reserved = 0;
    o.pairs = 0; o.cost = 0; o.den = 0; o.nominal_cost = 0; o.nominal_den = 0;
    o.seam_db = 0.0; o.nominal_db = 0.0; o.improvement_db = 0.0;
    if (best.s >= 0 && pairs > 0) {
        o.found = 1; o.start_frame = best.s; o.stop_frame = best.e; o.shift = shift; o.starts = R.ns; o.ends = R.ne;
        o.pairs = pairs; o.cost = best.cost; o.den = best.den;
        if (nominal) { o.nominal_valid = 1; o.nominal_cost = ncost; o.nominal_den = nden; }
    }
    *out = o;
}

// a whole request by one thread, straight from the definition, over its two strips and its E arrays (the host route of
// scripts/loop_bench.py and the harness's second opinion).  The starts [c0, c1) only: a thread's share; shares merge with zl_lp_better
inline void zl_lp_search_serial(const ZlLpRequest &R, const int16_t *xs, const int16_t *xe, const uint32_t *Es, const uint32_t *Ee, int32_t c0, int32_t c1,
                                ZlLpPair *best, uint64_t *pairs)
{
    ZlLpPair b = zl_lp_no_pair(); uint64_t n = 0;
    for (int32_t cs = c0; cs < c1; ++cs)
        for (int32_t ce = 0; ce < R.ne; ++ce) {
            const int32_t s = R.smin + cs, e = R.emin + ce;
            if (!zl_lp_admissible(s, e, R.min_length)) continue;
            ZlLpPair p; p.s = s; p.e = e; p.cost = zl_lp_cost(xs, xe, cs, ce, R.window); p.den = zl_lp_den(Es[cs], Ee[ce]);
            ++n;
            if (zl_lp_better(p, b, R.s0, R.e0)) b = p;
        }
    *best = b; *pairs = n;
}

// seam_db, nominal_db, improvement_db from the integer record (host, double, one IEEE operation per operator: build without contraction)
inline double zl_lp_db(uint32_t cost, uint32_t den)
{
    if (cost == 0) return ZL_LP_DB_FLOOR;
    const double v = 10.0 * log10((double)cost / (double)den);
    return v < ZL_LP_DB_FLOOR ? ZL_LP_DB_FLOOR : v;
}
inline void zl_lp_finish(ZlLpResult *r)
{
    r->seam_db = 0.0; r->nominal_db = 0.0; r->improvement_db = 0.0;
    if (!r->found) return;
    r->seam_db = zl_lp_db(r->cost, r->den);
    if (r->nominal_valid) { r->nominal_db = zl_lp_db(r->nominal_cost, r->nominal_den); r->improvement_db = r->nominal_db - r->seam_db; }
}

// The voice derives its loop from float seconds: start = (int)(start_s * rate), stop = (int)((float)(start_s + length_s) * rate)
// (zl_clip_start / zl_clip_stop and K1's casts, zl_plan.h).  These two are those formulas; zl_lp_seconds inverts them.
inline int64_t zl_lp_frame_of(float seconds, double rate) { return (int64_t)((double)seconds * rate); }
inline int64_t zl_lp_stop_of(float start_s, float length_s, double rate) { const float sum = start_s + length_s; return (int64_t)((double)sum * rate); }

// start_s and length_s that map to (start, stop): the middle of the frame, nudged by single floats (at most 8 each) until it maps;
// 0, or -1: not representable (a float has 24 bits: from about 2^23 frames on some pairs are not)
inline int zl_lp_seconds(double rate, int64_t start, int64_t stop, float *start_s, float *length_s)
{
    if (!(rate > 0.0) || start < 0 || stop <= start) return -1;
    float a = (float)(((double)start + 0.5) / rate);
    for (int n = 0; ; ++n) {
        const int64_t m = zl_lp_frame_of(a, rate);
        if (m == start) break;
        if (n == 8) return -1;
        a = nextafterf(a, m < start ? INFINITY : -INFINITY);
    }
    float t = (float)(((double)stop + 0.5) / rate), len = t - a;
    for (int n = 0; ; ++n) {
        len = t - a;
        const int64_t m = zl_lp_stop_of(a, len, rate);
        if (m == stop) break;
        if (n == 8) return -1;
        t = nextafterf(t, m < stop ? INFINITY : -INFINITY);         // (the sum's target moves: a nudge of the length alone can be lost in the sum)
    }
    *start_s = a; *length_s = len;
    return 0;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_loop.hip; 0 or a hipError_t value).  X [call strip elements] int16, E [call candidates] uint32, shifts [nreq],
// items [call items], costs: the call's cost matrix or null; out [nreq] may be host memory mapped into the device
int zl_launch_loop_prep(const ZlLpRequest *reqs, int32_t nreq, int16_t *X, uint32_t *E, int32_t *shifts, hipStream_t s);
int zl_launch_loop_pairs(const ZlLpRequest *reqs, int32_t nreq, int64_t items, const int16_t *X, const uint32_t *E, ZlLpItem *out, uint32_t *costs, hipStream_t s);
int zl_launch_loop_pick(const ZlLpRequest *reqs, int32_t nreq, const int16_t *X, const uint32_t *E, const int32_t *shifts, const ZlLpItem *items, ZlLpResult *out, hipStream_t s);
#endif
