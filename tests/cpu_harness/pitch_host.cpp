// Host build of the pitch detection's definition (libzl_amd/csrc/zl_pitch.h) for the CPU tier -- TEST HARNESS ONLY.
// zlpt_call walks a call the way the kernels do, with the header's own arithmetic: the difference function work item by work item (the
// request by bisection over item_base, the frame's 16-byte groups of the arena's layout masked by float index, the mix, the shift, the
// staged int16 samples, a lane per lag with 32-bit partial sums), the pick with a lane's eight consecutive lags and min-reductions merged
// in another order, the vote with a lane per frame and a histogram scanned in lane-sized pieces.  It counts how often every (j, t)
// term enters and every float of the sounds is used, and refuses -- and counts -- any float outside a request's frames.  The walks are
// held to the header's one-thread forms (zl_pt_pick_serial, zl_pt_vote_serial).  zlpt_pick_vote runs pick and vote on hand-made d
// arrays.  zlpt_run_planar is a whole request over planar data, straight from the definition's sums: the host side of
// scripts/pitch_bench.py.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "zl_pitch.h"
#include "zlhip.h"

namespace {

const int kThreads = ZL_PT_TILE;
const int kPerLane = ZL_PT_MAX_LAGS / kThreads;

struct Walk { int64_t terms = 0, refused = 0, staged_wrong = 0, disagree = 0; };

int32_t find(const ZlPtRequest *reqs, int32_t nreq, int32_t at, bool items)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((items ? reqs[mid].item_base : reqs[mid].frame_base) <= at) lo = mid; else hi = mid - 1;
    }
}

// the geometry of a request: 0, or -1 where a limit is broken.  first + num_frames <= length is the caller's to keep
int geometry(const zlhip_pitch_request &q0, double rate, int32_t channels, const float *src, ZlPtRequest *R)
{
    zlhip_pitch_request q = q0;
    if (q.first_frame < 0 || q.num_frames < 1) return -1;
    if (zl_pt_resolve(rate, &q.window, &q.max_frames, &q.f_min, &q.f_max, &q.threshold, &q.gate) != 0) return -1;
    double tmin, tmax;
    zl_pt_lags(rate, q.f_min, q.f_max, &tmin, &tmax);
    R->src = (uint64_t)(uintptr_t)src;
    R->floor_ = (uint64_t)q.window * (uint64_t)channels * (uint64_t)q.gate * (uint64_t)q.gate;
    R->first = q.first_frame; R->channels = channels;
    R->window = q.window; R->tmin = (int32_t)tmin; R->tmax = (int32_t)tmax; R->threshold = q.threshold;
    zl_pt_frames(q.num_frames, R->window, R->tmax, q.max_frames, &R->frames, &R->hop);
    return 0;
}

// one work item of the difference function.  lo, hi: the floats [lo, hi) of the sound that belong to the request's frames;
// touched: per float of the sound, how often it was used (or null); counts: [K][nd][W] bytes (or null)
void diff_item(const ZlPtRequest *reqs, int32_t nreq, int32_t item, uint64_t *Dall, ZlPtStat *stat, const int64_t *lo, const int64_t *hi, uint8_t *const *touched,
               uint8_t *const *counts, Walk &w)
{
    const int32_t r = find(reqs, nreq, item, true);
    const ZlPtRequest &R = reqs[r];
    int32_t frame, tile;
    zl_pt_item_of(R, item - R.item_base, &frame, &tile);
    const int32_t L = zl_pt_span(R), W = R.window, nd = zl_pt_nd(R);
    const int64_t s0 = zl_pt_frame_start(R, frame);
    int64_t f0, f1, g0, g1;
    zl_ov_groups(s0, s0 + L, R.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const float *src = (const float *)(uintptr_t)R.src + 4 * g0;
    std::vector<int32_t> mixed((size_t)L, 0);
    std::vector<int16_t> sX((size_t)L, (int16_t)0x7fff);
    std::vector<uint8_t> written((size_t)L, 0);
    uint32_t amax = 0; uint64_t energy = 0;
    for (int32_t g = ngroups - 1; g >= 0; --g) {                   // (any order: integer maximum and sum)
        // the elements the mask lets through are the only ones looked at: copy those, leave the others a NaN pattern
        float v[4];
        for (int j = 0; j < 4; ++j) {
            const uint32_t nan = 0x7fc00000u;
            std::memcpy(&v[j], &nan, 4);
            if (!zl_ov_valid(g, j, head, count)) continue;
            const int64_t at = 4 * (g0 + g) + j;
            if (at < lo[r] || at >= hi[r]) { ++w.refused; continue; }                 // a float outside the request's frames: never used
            v[j] = src[4 * g + j];
            if (touched && touched[r] && tile == 0) touched[r][at] += 1;
        }
        int32_t m[4], idx[4];
        zl_pt_group_mix(v[0], v[1], v[2], v[3], g, head, count, R.channels, m, idx);
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = (uint32_t)(m[j] < 0 ? -m[j] : m[j]);
            amax = std::max(amax, a);
            if (idx[j] < 0) continue;
            if (idx[j] >= L) { ++w.refused; continue; }
            if (idx[j] < W) energy += (uint64_t)a * a;
            mixed[(size_t)idx[j]] = m[j];
            written[(size_t)idx[j]] += 1;
        }
    }
    const int32_t shift = zl_pt_shift(amax);
    if (tile == 0) { ZlPtStat st; st.energy = energy; st.shift = shift; st.silent = energy < R.floor_ ? 1 : 0; stat[R.frame_base + frame] = st; }
    for (int32_t i = 0; i < L; ++i) {
        if (written[(size_t)i] != 1) ++w.staged_wrong;             // every sample of the span is staged exactly once
        const int32_t x = mixed[(size_t)i] >> shift;
        if (x < -(1 << ZL_PT_BITS) || x >= (1 << ZL_PT_BITS)) ++w.staged_wrong;
        sX[(size_t)i] = (int16_t)x;
    }
    for (int lane = kThreads - 1; lane >= 0; --lane) {
        const int32_t t = zl_pt_lane_lag(R, tile, lane);
        const bool live = zl_pt_lane_live(R, tile, lane);
        uint64_t acc = 0;
        for (int32_t j0 = 0; j0 < W; j0 += ZL_PT_CHUNK) {
            uint32_t part = 0;
            for (int32_t j = j0; j < j0 + ZL_PT_CHUNK; ++j) {
                if (j + t >= L) { ++w.refused; continue; }         // behind the staged samples
                const int32_t df = (int32_t)sX[(size_t)j] - (int32_t)sX[(size_t)(j + t)];
                part += (uint32_t)(df * df);
                if (live) { ++w.terms; if (counts && counts[r]) counts[r][((size_t)frame * (size_t)nd + (size_t)(t - 1)) * (size_t)W + (size_t)j] += 1; }
            }
            acc += part;
        }
        if (live) Dall[R.d_base + (int64_t)frame * nd + (t - 1)] = acc;
    }
}

// the pick of one frame the way the workgroup does it: lane `tid` owns the lags 8 tid + 1 .. 8 tid + 8
void pick_walk(const ZlPtRequest &R, const ZlPtStat &st, const uint64_t *d, ZlPtFrame *out, Walk &w)
{
    const int32_t nd = zl_pt_nd(R);
    std::vector<uint64_t> own((size_t)kThreads, 0), C((size_t)ZL_PT_MAX_LAGS, 0);
    for (int t = 0; t < kThreads; ++t)
        for (int k = 0; k < kPerLane; ++k) { const int32_t i = t * kPerLane + k; if (i < nd) own[(size_t)t] += d[i]; }
    std::vector<uint64_t> base((size_t)kThreads, 0);
    for (int t = 1; t < kThreads; ++t) base[(size_t)t] = base[(size_t)(t - 1)] + own[(size_t)(t - 1)];
    const int32_t none = ZL_PT_MAX_LAGS;
    int32_t t0 = none;
    for (int t = kThreads - 1; t >= 0; --t) {
        uint64_t run = base[(size_t)t];
        int32_t first = none;
        for (int k = 0; k < kPerLane; ++k) {
            const int32_t i = t * kPerLane + k, lag = i + 1;
            if (i >= nd) continue;
            run += d[i];
            C[(size_t)i] = run;
            if (first == none && lag >= R.tmin && lag <= R.tmax && zl_pt_below(d[i], lag, R.threshold, run)) first = lag;
        }
        t0 = std::min(t0, first);
    }
    int32_t stop = none;
    for (int t = kThreads - 1; t >= 0 && t0 < none; --t)
        for (int k = 0; k < kPerLane; ++k) {
            const int32_t lag = t * kPerLane + k + 1;
            if (lag >= t0 && lag <= R.tmax && zl_pt_stops(d[lag - 1], d[lag], lag, R.tmax)) { stop = std::min(stop, lag); break; }
        }
    const int32_t tk = st.silent || stop >= none ? 0 : stop;
    zl_pt_frame_record(st, d, tk > 0 ? C[(size_t)(tk - 1)] : 0, tk, out);
    ZlPtFrame serial;
    zl_pt_pick_serial(R, st, d, &serial);
    if (std::memcmp(&serial, out, sizeof(serial)) != 0) ++w.disagree;
}

// the vote of one request the way the workgroup does it: lane k owns frame k and the histogram bins 8 k .. 8 k + 7
void vote_walk(const ZlPtFrame *F, int32_t K, ZlPtResult *out, Walk &w)
{
    std::vector<uint32_t> hist((size_t)ZL_PT_MAX_LAGS, 0);
    int32_t V = 0;
    for (int32_t k = K - 1; k >= 0; --k) if (F[k].lag > 0) { hist[(size_t)F[k].lag] += 1; ++V; }
    std::vector<uint64_t> own((size_t)kThreads, 0), base((size_t)kThreads, 0);
    for (int t = 0; t < kThreads; ++t) for (int k = 0; k < kPerLane; ++k) own[(size_t)t] += hist[(size_t)(t * kPerLane + k)];
    for (int t = 1; t < kThreads; ++t) base[(size_t)t] = base[(size_t)(t - 1)] + own[(size_t)(t - 1)];
    const uint64_t rank = (uint64_t)((V > 0 ? V - 1 : 0) / 2);
    int32_t med = ZL_PT_MAX_LAGS;
    for (int t = kThreads - 1; t >= 0; --t) {
        uint64_t run = base[(size_t)t];
        for (int k = 0; k < kPerLane; ++k) {
            run += hist[(size_t)(t * kPerLane + k)];
            if (V > 0 && run > rank) { med = std::min(med, t * kPerLane + k); break; }
        }
    }
    int32_t consistent = 0, rep = -1; int64_t best = ZL_PT_NO_KEY;
    for (int32_t k = K - 1; k >= 0; --k) {
        if (F[k].lag == 0 || !zl_pt_consistent(F[k].lag, med)) continue;
        ++consistent;
        if (zl_pt_key(F[k].clarity, k) > best) { best = zl_pt_key(F[k].clarity, k); rep = k; }
    }
    zl_pt_result(K, V, consistent, rep, F, out);
    ZlPtResult serial;
    zl_pt_vote_serial(F, K, &serial);
    if (std::memcmp(&serial, out, sizeof(serial)) != 0) ++w.disagree;
}

}  // namespace

extern "C" {

int32_t zlpt_resolve(double sr, int32_t *window, int32_t *max_frames, float *f_min, float *f_max, int32_t *threshold, int32_t *gate)
{
    return zl_pt_resolve(sr, window, max_frames, f_min, f_max, threshold, gate);
}
void zlpt_sizes(int32_t *out) { out[0] = (int32_t)sizeof(ZlPtResult); out[1] = (int32_t)sizeof(ZlPtFrame); out[2] = (int32_t)sizeof(ZlPtRequest); }

// A call of nreq requests.  reqs[i].id is ignored: request i reads data[i], the sound in the arena's layout ([L0 R0 L1 R1] / [x0 x1 ..],
// length[i] frames, padded with zeros to a whole 16-byte group), channels[i], rate[i].  D [d_capacity] words, frames [frame_capacity]
// records, geom [nreq][8] = (t_min, t_max, window, K, hop, items, frame_base, tiles), d_base [nreq], out [nreq] results (finished),
// touched [nreq] pointers (each null or [length * channels] zeroed bytes), counts [nreq] pointers (each null or [K][t_max + 1][W] zeroed
// bytes), walk [4] = (terms entered, floats or samples refused, samples not staged exactly once or out of range, walks that disagree
// with the one-thread forms).  Returns the d words used; -1: a capacity is too small; -2: a request is outside its limits.
int64_t zlpt_call(int32_t nreq, const zlhip_pitch_request *reqs, const float *const *data, const int32_t *length, const int32_t *channels, const double *rate, uint64_t *D,
                  int64_t d_capacity, ZlPtFrame *frames, int64_t frame_capacity, int32_t *geom, int64_t *d_base, ZlPtResult *out, uint8_t *const *touched,
                  uint8_t *const *counts, int64_t *walk)
{
    std::vector<ZlPtRequest> R((size_t)nreq);
    std::vector<int64_t> lo((size_t)nreq), hi((size_t)nreq);
    int64_t nf = 0, words = 0, items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlPtRequest &T = R[(size_t)i];
        if (geometry(reqs[i], rate[i], channels[i], data[i], &T) != 0) return -2;
        if ((int64_t)reqs[i].first_frame + reqs[i].num_frames > length[i]) return -2;
        T.d_base = words; T.frame_base = (int32_t)nf; T.item_base = (int32_t)items;
        lo[(size_t)i] = (int64_t)reqs[i].first_frame * channels[i];
        hi[(size_t)i] = ((int64_t)reqs[i].first_frame + reqs[i].num_frames) * channels[i];
        const int32_t g[8] = {T.tmin, T.tmax, T.window, T.frames, T.hop, zl_pt_items(T), T.frame_base, zl_pt_tiles(T)};
        std::memcpy(geom + 8 * i, g, sizeof(g));
        d_base[i] = words;
        nf += T.frames; words += (int64_t)T.frames * zl_pt_nd(T); items += zl_pt_items(T);
    }
    if (words > d_capacity || nf > frame_capacity || nf > ZL_PT_MAX_CALL_FRAMES) return -1;
    std::vector<ZlPtStat> stat((size_t)nf);
    Walk w;
    for (int64_t it = items - 1; it >= 0; --it) diff_item(R.data(), nreq, (int32_t)it, D, stat.data(), lo.data(), hi.data(), touched, counts, w);
    for (int64_t f = nf - 1; f >= 0; --f) {
        const ZlPtRequest &T = R[(size_t)find(R.data(), nreq, (int32_t)f, false)];
        pick_walk(T, stat[(size_t)f], D + T.d_base + (f - T.frame_base) * zl_pt_nd(T), &frames[f], w);
    }
    for (int32_t i = 0; i < nreq; ++i) {
        vote_walk(frames + R[(size_t)i].frame_base, R[(size_t)i].frames, &out[i], w);
        zl_pt_finish(rate[i], &out[i]);
    }
    walk[0] = w.terms; walk[1] = w.refused; walk[2] = w.staged_wrong; walk[3] = w.disagree;
    return words;
}

// pick and vote on hand-made d arrays: K frames of nd = t_max + 1 words each, silent [K], shift [K].  frames [K], out: the finished
// result.  Returns how many walks disagree with the one-thread forms
int32_t zlpt_pick_vote(int32_t K, int32_t tmin, int32_t tmax, int32_t threshold, const uint64_t *d, const int32_t *silent, const int32_t *shift, double rate,
                       ZlPtFrame *frames, ZlPtResult *out)
{
    ZlPtRequest R;
    std::memset(&R, 0, sizeof(R));
    R.tmin = tmin; R.tmax = tmax; R.threshold = threshold; R.frames = K; R.window = ZL_PT_WINDOW_MAX;
    Walk w;
    for (int32_t k = 0; k < K; ++k) {
        ZlPtStat st; st.energy = 0; st.shift = shift[k]; st.silent = silent[k];
        pick_walk(R, st, d + (size_t)k * (size_t)(tmax + 1), &frames[k], w);
    }
    vote_walk(frames, K, out, w);
    zl_pt_finish(rate, out);
    return (int32_t)w.disagree;
}

// the whole request over planar data (right: null for a mono clip), straight sums, the frames on `threads` threads; 0, or -1 where a
// limit is broken.  frames_out: null or [max_frames] records
int32_t zlpt_run_planar(const float *left, const float *right, const zlhip_pitch_request *q, double rate, int32_t threads, ZlPtFrame *frames_out, ZlPtResult *out)
{
    ZlPtRequest R;
    if (geometry(*q, rate, right ? 2 : 1, left, &R) != 0) return -1;
    const int32_t L = zl_pt_span(R), W = R.window, nd = zl_pt_nd(R), K = R.frames;
    std::vector<ZlPtFrame> F((size_t)std::max(K, 1));
    auto work = [&](int32_t th) {
        std::vector<int32_t> m((size_t)L);
        std::vector<int16_t> x((size_t)L);
        std::vector<uint64_t> d((size_t)nd);
        for (int32_t k = (int32_t)((int64_t)K * th / threads); k < (int32_t)((int64_t)K * (th + 1) / threads); ++k) {
            const int64_t s0 = zl_pt_frame_start(R, k);
            uint32_t amax = 0; uint64_t e = 0;
            for (int32_t j = 0; j < L; ++j) {
                const int32_t v = zl_st_q(left[s0 + j]) + (right ? zl_st_q(right[s0 + j]) : 0);
                const uint32_t a = (uint32_t)(v < 0 ? -v : v);
                m[(size_t)j] = v; amax = std::max(amax, a);
                if (j < W) e += (uint64_t)a * a;
            }
            ZlPtStat st; st.energy = e; st.shift = zl_pt_shift(amax); st.silent = e < R.floor_ ? 1 : 0;
            for (int32_t j = 0; j < L; ++j) x[(size_t)j] = (int16_t)(m[(size_t)j] >> st.shift);
            for (int32_t t = 1; t <= nd; ++t) {
                uint64_t acc = 0;
                for (int32_t j0 = 0; j0 < W; j0 += ZL_PT_CHUNK) {
                    uint32_t part = 0;
                    for (int32_t j = j0; j < j0 + ZL_PT_CHUNK; ++j) { const int32_t df = (int32_t)x[(size_t)j] - (int32_t)x[(size_t)(j + t)]; part += (uint32_t)(df * df); }
                    acc += part;
                }
                d[(size_t)(t - 1)] = acc;
            }
            zl_pt_pick_serial(R, st, d.data(), &F[(size_t)k]);
        }
    };
    std::vector<std::thread> pool;
    for (int32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    zl_pt_vote_serial(F.data(), K, out);
    zl_pt_finish(rate, out);
    if (frames_out) std::memcpy(frames_out, F.data(), (size_t)K * sizeof(ZlPtFrame));
    return 0;
}

}
