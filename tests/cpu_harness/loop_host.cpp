// Host build of the loop finder's definition (libzl_amd/csrc/zl_loop.h) for the CPU tier -- TEST HARNESS ONLY.
// zllp_call walks a call the way the kernels do, with the header's own arithmetic: the prep request by request (the two strips' 16-byte
// groups of the arena's layout masked by float index, the mix, the one shift, the int16 strips, E per candidate by a lane's run of
// sliding windows), the pairs work item by work item (the request by bisection over item_base, the two staged strip tiles with their
// zero fill, lane tile by lane tile four samples per side at a time, in either form, the lanes outside a partial tile contributing
// nothing, the item's best pair merged in another order than the device's), the pick over the items and the nominal pair.  It counts
// the terms that enter, every float of the sounds that is used, and refuses -- and counts -- any float outside a request's strips and
// any staged element read behind a tile.  The walk is held to the header's one-thread form (zl_lp_search_serial).  zllp_run_planar is a
// whole request over planar data on `threads` threads, straight from the definition's sums: the host side of scripts/loop_bench.py.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "zl_loop.h"
#include "zlhip.h"

namespace {

const int kThreads = 256;
enum { kFormDiff = 0, kFormDot = 1 };          // what the walk sums per pair: the squared differences, or the cross term (the kernel's)

struct Walk { int64_t terms = 0, refused = 0, staged_wrong = 0, disagree = 0; };

int32_t find(const ZlLpRequest *reqs, int32_t nreq, int32_t at)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= at) lo = mid; else hi = mid - 1;
    }
}

// the geometry of a request: 0, or -1 where a limit is broken
int geometry(const zlhip_loop_request &q0, double rate, int32_t channels, int32_t length, const float *src, ZlLpRequest *R)
{
    zlhip_loop_request q = q0;
    if (q.start_frame < 0 || q.stop_frame <= q.start_frame || q.stop_frame > length) return -1;
    if (zl_lp_resolve(rate, &q.start_search, &q.stop_search, &q.window, &q.min_length) != 0) return -1;
    std::memset(R, 0, sizeof(*R));
    R->src = (uint64_t)(uintptr_t)src;
    R->s0 = q.start_frame; R->e0 = q.stop_frame; R->window = q.window; R->min_length = q.min_length; R->channels = channels;
    zl_lp_range(q.start_frame, q.start_search, q.window >> 1, length, &R->smin, &R->ns);
    zl_lp_range(q.stop_frame, q.stop_search, q.window >> 1, length, &R->emin, &R->ne);
    if (R->ns == 0 || R->ne == 0) { R->ns = 0; R->ne = 0; }
    return 0;
}

// the prep of one request: the strips into X, E per candidate, the shift.  touched: per float of the sound how often it was used (or null)
void prep_walk(const ZlLpRequest &R, int32_t length, int16_t *X, uint32_t *E, int32_t *shift_out, uint8_t *touched, Walk &w)
{
    *shift_out = 0;
    if (R.ns <= 0 || R.ne <= 0) return;
    const int32_t W = R.window, H = W >> 1;
    const int32_t lo[2] = {R.smin - H, R.emin - H}, len[2] = {zl_lp_strip_len(R.ns, W), zl_lp_strip_len(R.ne, W)}, base[2] = {R.xs_base, R.xe_base};
    std::vector<int32_t> mixed[2];
    std::vector<uint8_t> written[2];
    uint32_t amax = 0;
    for (int k = 1; k >= 0; --k) {
        mixed[k].assign((size_t)len[k], 0); written[k].assign((size_t)len[k], 0);
        int64_t f0, f1, g0, g1;
        zl_ov_groups(lo[k], (int64_t)lo[k] + len[k], R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const float *src = (const float *)(uintptr_t)R.src + 4 * g0;
        for (int32_t g = ngroups - 1; g >= 0; --g) {
            // the elements the mask lets through are the only ones looked at: copy those, leave the others a NaN pattern
            float v[4];
            for (int j = 0; j < 4; ++j) {
                const uint32_t nan = 0x7fc00000u;
                std::memcpy(&v[j], &nan, 4);
                if (!zl_ov_valid(g, j, head, count)) continue;
                const int64_t at = 4 * (g0 + g) + j;
                if (at < (int64_t)lo[k] * R.channels || at >= ((int64_t)lo[k] + len[k]) * R.channels || at < 0 || at >= (int64_t)length * R.channels) { ++w.refused; continue; }
                v[j] = src[4 * g + j];
                if (touched) touched[at] |= (uint8_t)(1 << k);
            }
            int32_t m[4], idx[4];
            zl_pt_group_mix(v[0], v[1], v[2], v[3], g, head, count, R.channels, m, idx);
            for (int j = 0; j < 4; ++j) {
                const uint32_t a = (uint32_t)(m[j] < 0 ? -m[j] : m[j]);
                amax = std::max(amax, a);
                if (idx[j] < 0) continue;
                if (idx[j] >= len[k]) { ++w.refused; continue; }
                mixed[k][(size_t)idx[j]] = m[j];
                written[k][(size_t)idx[j]] += 1;
            }
        }
    }
    const int32_t shift = zl_lp_shift(amax);
    *shift_out = shift;
    for (int k = 0; k < 2; ++k)
        for (int32_t i = 0; i < len[k]; ++i) {
            if (written[k][(size_t)i] != 1) ++w.staged_wrong;       // every sample of a strip is written exactly once
            const int32_t x = mixed[k][(size_t)i] >> shift;
            if (x < -(1 << ZL_LP_BITS) || x >= (1 << ZL_LP_BITS)) ++w.staged_wrong;
            X[base[k] + i] = (int16_t)x;
        }
    // E: lane `tid` owns a run of consecutive candidates, the first by the window's sum, the others by sliding
    for (int k = 0; k < 2; ++k) {
        const int32_t n = k == 0 ? R.ns : R.ne, per = (n + kThreads - 1) / kThreads;
        const int16_t *x = X + base[k];
        uint32_t *out = E + (k == 0 ? R.es_base : R.ee_base);
        for (int tid = kThreads - 1; tid >= 0; --tid) {
            const int32_t c0 = tid * per, c1 = std::min(c0 + per, n);
            if (c0 >= c1) continue;
            uint32_t e = zl_lp_energy(x, c0, W);
            out[c0] = e;
            for (int32_t c = c0 + 1; c < c1; ++c) {
                if (c + W - 1 >= len[k]) { ++w.refused; continue; }
                const int32_t a = x[c - 1], b = x[c + W - 1];
                e = e - (uint32_t)(a * a) + (uint32_t)(b * b);
                out[c] = e;
                if (e != zl_lp_energy(x, c, W)) ++w.disagree;
            }
        }
    }
}

// one work item of the pairs pass
void pairs_item(const ZlLpRequest *reqs, int32_t nreq, int32_t item, const int16_t *X, const uint32_t *E, ZlLpItem *out, uint32_t *costs, int form, Walk &w)
{
    const ZlLpRequest &R = reqs[find(reqs, nreq, item)];
    int32_t ts, te;
    zl_lp_item_of(R, item - R.item_base, &ts, &te);
    const int32_t W = R.window, cs0 = ts * ZL_LP_TILE, ce0 = te * ZL_LP_TILE;
    const int32_t ncs = std::min(R.ns - cs0, (int32_t)ZL_LP_TILE), nce = std::min(R.ne - ce0, (int32_t)ZL_LP_TILE);
    const int32_t lenS = zl_lp_strip_len(R.ns, W), lenE = zl_lp_strip_len(R.ne, W), stage = ZL_LP_TILE + W;
    std::vector<int16_t> sS((size_t)stage), sE((size_t)stage);
    for (int32_t i = 0; i < stage; ++i) {
        sS[(size_t)i] = cs0 + i < lenS ? X[R.xs_base + cs0 + i] : (int16_t)0;
        sE[(size_t)i] = ce0 + i < lenE ? X[R.xe_base + ce0 + i] : (int16_t)0;
    }
    ZlLpPair best = zl_lp_no_pair();
    uint64_t pairs = 0;
    for (int lane = kThreads - 1; lane >= 0; --lane) {
        const int32_t a4 = zl_lp_lane_start(lane), b4 = zl_lp_lane_end(lane);
        uint32_t diff[ZL_LP_LANE][ZL_LP_LANE] = {};
        int32_t dot[ZL_LP_LANE][ZL_LP_LANE] = {};
        for (int32_t jb = 0; jb < W; jb += 4) {
            // the eight samples per side the lane holds in this step: its current word and the next one
            if (a4 + jb + 7 >= stage || b4 + jb + 7 >= stage) { ++w.refused; continue; }
            for (int jj = 0; jj < 4; ++jj)
                for (int i = 0; i < ZL_LP_LANE; ++i)
                    for (int k = 0; k < ZL_LP_LANE; ++k) {
                        const int32_t a = sS[(size_t)(a4 + jb + i + jj)], b = sE[(size_t)(b4 + jb + k + jj)];
                        diff[i][k] += zl_lp_term(a, b);
                        dot[i][k] += a * b;
                    }
        }
        for (int i = 0; i < ZL_LP_LANE; ++i)
            for (int k = 0; k < ZL_LP_LANE; ++k) {
                if (a4 + i >= ncs || b4 + k >= nce) continue;
                const int32_t cs = cs0 + a4 + i, ce = ce0 + b4 + k;
                const uint32_t es = E[R.es_base + cs], ee = E[R.ee_base + ce];
                ZlLpPair p;
                p.s = R.smin + cs; p.e = R.emin + ce;
                p.cost = form == kFormDiff ? diff[i][k] : zl_lp_cost_from_dot(es, ee, dot[i][k]);
                if (diff[i][k] != zl_lp_cost_from_dot(es, ee, dot[i][k])) ++w.disagree;            // the two forms
                p.den = zl_lp_den(es, ee);
                w.terms += W;
                if (costs) costs[R.cost_base + (int64_t)cs * R.ne + ce] = p.cost;
                if (!zl_lp_admissible(p.s, p.e, R.min_length)) continue;
                ++pairs;
                if (zl_lp_better(p, best, R.s0, R.e0)) best = p;
            }
    }
    out[item] = zl_lp_item_record(best, pairs);
}

void pick_walk(const ZlLpRequest &R, const int16_t *X, const uint32_t *E, int32_t shift, const ZlLpItem *items, ZlLpResult *out, Walk &w)
{
    const int32_t n = zl_lp_items(R);
    ZlLpPair best = zl_lp_no_pair();
    uint64_t pairs = 0;
    for (int32_t i = n - 1; i >= 0; --i) {
        const ZlLpItem &it = items[R.item_base + i];
        ZlLpPair p; p.s = it.start; p.e = it.stop; p.cost = it.cost; p.den = it.den;
        pairs += it.pairs;
        if (zl_lp_better(p, best, R.s0, R.e0)) best = p;
    }
    const bool nominal = zl_lp_nominal_valid(R);
    uint32_t ncost = 0, nden = 0;
    if (nominal) {
        const int32_t cs = R.s0 - R.smin, ce = R.e0 - R.emin;
        ncost = zl_lp_cost(X + R.xs_base, X + R.xe_base, cs, ce, R.window);
        nden = zl_lp_den(E[R.es_base + cs], E[R.ee_base + ce]);
    }
    zl_lp_result(R, best, pairs, shift, nominal, ncost, nden, out);
    // the second opinion: one thread, straight from the definition
    ZlLpPair sb = zl_lp_no_pair(); uint64_t sp = 0;
    if (R.ns > 0) zl_lp_search_serial(R, X + R.xs_base, X + R.xe_base, E + R.es_base, E + R.ee_base, 0, R.ns, &sb, &sp);
    if (sp != pairs || sb.s != best.s || sb.e != best.e || sb.cost != best.cost || sb.den != best.den) ++w.disagree;
}

}  // namespace

extern "C" {

int32_t zllp_resolve(double sr, int32_t *rs, int32_t *re, int32_t *window, int32_t *min_length) { return zl_lp_resolve(sr, rs, re, window, min_length); }
void zllp_sizes(int32_t *out) { out[0] = (int32_t)sizeof(ZlLpResult); out[1] = (int32_t)sizeof(ZlLpItem); out[2] = (int32_t)sizeof(ZlLpRequest); }
int32_t zllp_seconds(double rate, int64_t start, int64_t stop, float *start_s, float *length_s) { return zl_lp_seconds(rate, start, stop, start_s, length_s); }
int64_t zllp_frame_of(float seconds, double rate) { return zl_lp_frame_of(seconds, rate); }
int64_t zllp_stop_of(float start_s, float length_s, double rate) { return zl_lp_stop_of(start_s, length_s, rate); }
// is pair a = (s, e, cost, den) better than pair b around the nominal (s0, e0)?
int32_t zllp_better(const int64_t *a, const int64_t *b, int32_t s0, int32_t e0)
{
    ZlLpPair pa, pb;
    pa.s = (int32_t)a[0]; pa.e = (int32_t)a[1]; pa.cost = (uint32_t)a[2]; pa.den = (uint32_t)a[3];
    pb.s = (int32_t)b[0]; pb.e = (int32_t)b[1]; pb.cost = (uint32_t)b[2]; pb.den = (uint32_t)b[3];
    return zl_lp_better(pa, pb, s0, e0) ? 1 : 0;
}

// A call of nreq requests.  reqs[i].id is ignored: request i reads data[i], the sound in the arena's layout ([L0 R0 L1 R1] / [x0 x1 ..],
// length[i] frames, padded with zeros to a whole 16-byte group), channels[i], rate[i].  costs [cost_capacity] words (every candidate
// pair's cost, [ns][ne] per request from cost_base[i] on), items [item_capacity] records, geom [nreq][8] = (smin, ns, emin, ne, window,
// min_length, items, item_base), out [nreq] results (finished), touched [nreq] pointers (each null or [length * channels] zeroed bytes:
// bit 0 the start strip, bit 1 the end strip), walk [4] = (terms entered, floats or staged elements refused, strip samples not written
// exactly once or out of range, walks that disagree with the one-thread forms or the other form).  form: 0 sums the squared differences,
// 1 the cross term as the kernel does.  Returns the cost
// words used; -1: a capacity is too small or a per-call limit is broken; -2: a request is outside its limits.
int64_t zllp_call(int32_t nreq, const zlhip_loop_request *reqs, const float *const *data, const int32_t *length, const int32_t *channels, const double *rate,
                  uint32_t *costs, int64_t cost_capacity, ZlLpItem *items, int64_t item_capacity, int32_t *geom, int64_t *cost_base, ZlLpResult *out,
                  uint8_t *const *touched, int64_t *walk, int32_t form)
{
    std::vector<ZlLpRequest> R((size_t)nreq);
    int64_t nitems = 0, strip = 0, cands = 0, words = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlLpRequest &T = R[(size_t)i];
        if (geometry(reqs[i], rate[i], channels[i], length[i], data[i], &T) != 0) return -2;
        T.cost_base = words; T.item_base = (int32_t)nitems;
        T.xs_base = (int32_t)strip; T.xe_base = T.xs_base + zl_lp_strip_room(T.ns, T.window);
        T.es_base = (int32_t)cands; T.ee_base = T.es_base + T.ns;
        const int32_t g[8] = {T.smin, T.ns, T.emin, T.ne, T.window, T.min_length, zl_lp_items(T), T.item_base};
        std::memcpy(geom + 8 * i, g, sizeof(g));
        cost_base[i] = words;
        nitems += zl_lp_items(T); strip += zl_lp_strip_room(T.ns, T.window) + zl_lp_strip_room(T.ne, T.window);
        cands += T.ns + T.ne; words += (int64_t)T.ns * T.ne;
    }
    if (words > cost_capacity || nitems > item_capacity || nitems > ZL_LP_MAX_CALL_ITEMS || strip > ZL_LP_MAX_CALL_STRIP) return -1;
    std::vector<int16_t> X((size_t)strip, (int16_t)0x7fff);
    std::vector<uint32_t> E((size_t)cands);
    std::vector<int32_t> shift((size_t)nreq);
    Walk w;
    for (int32_t i = nreq - 1; i >= 0; --i) prep_walk(R[(size_t)i], length[i], X.data(), E.data(), &shift[(size_t)i], touched ? touched[i] : nullptr, w);
    for (int64_t it = nitems - 1; it >= 0; --it) pairs_item(R.data(), nreq, (int32_t)it, X.data(), E.data(), items, costs, form, w);
    for (int32_t i = 0; i < nreq; ++i) {
        pick_walk(R[(size_t)i], X.data(), E.data(), shift[(size_t)i], items, &out[i], w);
        zl_lp_finish(&out[i]);
    }
    walk[0] = w.terms; walk[1] = w.refused; walk[2] = w.staged_wrong; walk[3] = w.disagree;
    return words;
}

// the whole request over planar data (right: null for a mono clip), straight sums, the starts on `threads` threads; 0, or -1 where a
// limit is broken
int32_t zllp_run_planar(const float *left, const float *right, int32_t length, const zlhip_loop_request *q, double rate, int32_t threads, ZlLpResult *out)
{
    ZlLpRequest R;
    if (geometry(*q, rate, right ? 2 : 1, length, left, &R) != 0 || threads < 1) return -1;
    const int32_t W = R.window, H = W >> 1, lenS = zl_lp_strip_len(R.ns, W), lenE = zl_lp_strip_len(R.ne, W);
    std::vector<int32_t> ms((size_t)lenS), me((size_t)lenE);
    uint32_t amax = 0;
    auto mix = [&](int32_t lo, std::vector<int32_t> &m) {
        for (size_t j = 0; j < m.size(); ++j) {
            const int32_t v = zl_st_q(left[lo + (int64_t)j]) + (right ? zl_st_q(right[lo + (int64_t)j]) : 0);
            m[j] = v; amax = std::max(amax, (uint32_t)(v < 0 ? -v : v));
        }
    };
    if (R.ns > 0) { mix(R.smin - H, ms); mix(R.emin - H, me); }
    const int32_t shift = zl_lp_shift(amax);
    std::vector<int16_t> xs((size_t)lenS), xe((size_t)lenE);
    for (size_t j = 0; j < xs.size(); ++j) xs[j] = (int16_t)(ms[j] >> shift);
    for (size_t j = 0; j < xe.size(); ++j) xe[j] = (int16_t)(me[j] >> shift);
    std::vector<uint32_t> Es((size_t)R.ns), Ee((size_t)R.ne);
    for (int32_t c = 0; c < R.ns; ++c) Es[(size_t)c] = zl_lp_energy(xs.data(), c, W);
    for (int32_t c = 0; c < R.ne; ++c) Ee[(size_t)c] = zl_lp_energy(xe.data(), c, W);
    std::vector<ZlLpPair> best((size_t)threads, zl_lp_no_pair());
    std::vector<uint64_t> pairs((size_t)threads, 0);
    auto work = [&](int32_t th) {
        const int32_t c0 = (int32_t)((int64_t)R.ns * th / threads), c1 = (int32_t)((int64_t)R.ns * (th + 1) / threads);
        zl_lp_search_serial(R, xs.data(), xe.data(), Es.data(), Ee.data(), c0, c1, &best[(size_t)th], &pairs[(size_t)th]);
    };
    std::vector<std::thread> pool;
    for (int32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    ZlLpPair b = zl_lp_no_pair(); uint64_t n = 0;
    for (int32_t t = 0; t < threads; ++t) { n += pairs[(size_t)t]; if (zl_lp_better(best[(size_t)t], b, R.s0, R.e0)) b = best[(size_t)t]; }
    const bool nominal = zl_lp_nominal_valid(R);
    uint32_t ncost = 0, nden = 0;
    if (nominal) {
        const int32_t cs = R.s0 - R.smin, ce = R.e0 - R.emin;
        ncost = zl_lp_cost(xs.data(), xe.data(), cs, ce, W);
        nden = zl_lp_den(Es[(size_t)cs], Ee[(size_t)ce]);
    }
    zl_lp_result(R, b, n, shift, nominal, ncost, nden, out);
    zl_lp_finish(out);
    return 0;
}

}
