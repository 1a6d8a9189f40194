// Host build of the tempo estimate's definition (libzl_amd/csrc/zl_tempo.h) for the CPU tier -- TEST HARNESS ONLY.
// zltp_call walks a call the way the kernels do, with the header's own arithmetic: the flux per request with thread-strided partial
// maxima and sums, the autocorrelation work item by work item (the request by bisection over item_base, the two staged arrays through
// zl_tp_h_index / zl_tp_l_index, a lane per lag), the pick with per-thread bests merged in another order, the record and the finish.
// It counts how often every (h, l) product enters, and refuses -- and counts -- any index outside a request's W.  zltp_run_planar is a
// whole request over planar data, straight from the definition's sums: the host side of scripts/tempo_bench.py.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "zl_tempo.h"

namespace {

const int kThreads = ZL_TP_TILE;

struct Walk { int64_t products = 0, refused = 0, mismatched = 0; };

uint16_t load_w(const uint16_t *W, const ZlTpRequest &R, int32_t h, Walk &w)
{
    if (h < 0 || h >= R.hops) { ++w.refused; return 0; }            // an address outside the request's W: never formed
    return W[h];
}

void flux(const ZlTpRequest &R, const uint64_t *E, uint16_t *W, uint64_t *A, ZlTpStat *st)
{
    for (int32_t l = 0; l < R.nlags; ++l) A[l] = 0;
    uint64_t part[kThreads] = {0};
    for (int t = 0; t < kThreads; ++t)
        for (int32_t h = t; h < R.hops; h += kThreads) part[t] = std::max(part[t], zl_tp_isqrt(E[h]));
    uint64_t rmax = 0;
    for (int t = kThreads - 1; t >= 0; --t) rmax = std::max(rmax, part[t]);
    const int32_t shift = zl_tp_shift(rmax);
    uint64_t sum = 0, sq = 0;
    for (int t = kThreads - 1; t >= 0; --t)
        for (int32_t h = t; h < R.hops; h += kThreads) {
            const uint32_t w = zl_tp_flux(zl_tp_isqrt(E[h]), h > 0 ? zl_tp_isqrt(E[h - 1]) : 0, shift);
            W[h] = (uint16_t)w;
            sum += w; sq += (uint64_t)w * w;
        }
    st->acf_zero = sq; st->sum = sum; st->shift = shift; st->pad = 0;
}

void acf_item(const ZlTpRequest *reqs, int32_t nreq, int32_t item, const uint16_t *Wall, uint64_t *Aall, uint8_t *const *counts, Walk &w)
{
    int32_t r = 0;
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= item) lo = mid; else hi = mid - 1;
    }
    const ZlTpRequest &R = reqs[r];
    int32_t tile, seg;
    zl_tp_item_of(R, item - R.item_base, &tile, &seg);
    if (!zl_tp_item_live(R, tile, seg)) return;
    const uint16_t *W = Wall + R.hop_base;
    std::vector<uint16_t> sH(ZL_TP_SEG), sL(ZL_TP_SEG + ZL_TP_TILE);
    for (int32_t i = 0; i < ZL_TP_SEG; ++i) { const int32_t h = zl_tp_h_index(R, seg, i); sH[(size_t)i] = h >= 0 ? load_w(W, R, h, w) : 0; }
    for (int32_t j = 0; j < ZL_TP_SEG + ZL_TP_TILE; ++j) { const int32_t h = zl_tp_l_index(R, tile, seg, j); sL[(size_t)j] = h >= 0 ? load_w(W, R, h, w) : 0; }
    const int32_t h0 = zl_tp_seg_hop(seg);
    const int32_t len = std::min(R.hops - h0, (int32_t)ZL_TP_SEG);
    const int32_t words = (len + 7) / 8 * 8;
    for (int lane = 0; lane < kThreads; ++lane) {
        const int32_t l = tile * ZL_TP_TILE + lane, lag = R.first_lag + l;
        uint64_t acc = 0;
        for (int32_t i = 0; i < words; ++i) {
            const int32_t word = zl_tp_window_word(i, lane), h = h0 + i;
            acc += (uint64_t)sH[(size_t)i] * (uint64_t)sL[(size_t)word];
            if (l >= R.nlags) continue;
            const bool real = h < R.hops && h - lag >= 0;
            if (zl_tp_l_index(R, tile, seg, word) != (h - lag >= 0 && h - lag < R.hops ? h - lag : -1)) ++w.mismatched;
            if (real) { ++w.products; if (counts && counts[r]) counts[r][(size_t)l * (size_t)R.hops + (size_t)h] += 1; }
        }
        if (l < R.nlags) {
            uint64_t *A = Aall + R.acf_base + l;
            if (R.nsegs == 1) *A = acc; else *A += acc;
        }
    }
}

void pick(const ZlTpRequest &R, const uint64_t *A, const ZlTpStat &st, ZlTpResult *out)
{
    int32_t bl[kThreads]; uint64_t ba[kThreads];
    for (int t = 0; t < kThreads; ++t) {
        bl[t] = 0; ba[t] = 0;
        for (int32_t l = R.lmin + t; l <= R.lmax; l += kThreads) {
            const uint64_t a = A[l - R.first_lag];
            if (bl[t] == 0 || zl_tp_beats(a, l, ba[t], bl[t], R.hops)) { bl[t] = l; ba[t] = a; }
        }
    }
    int32_t l = 0; uint64_t a = 0;
    for (int t = kThreads - 1; t >= 0; --t)                         // (any order: a total preorder)
        if (bl[t] != 0 && (l == 0 || zl_tp_beats(ba[t], bl[t], a, l, R.hops))) { l = bl[t]; a = ba[t]; }
    zl_tp_record(R, st, A, l, out);
}

}  // namespace

extern "C" {

uint64_t zltp_isqrt(uint64_t x) { return zl_tp_isqrt(x); }
int32_t zltp_resolve(double sr, int32_t *hop, float *bpm_min, float *bpm_max) { return zl_tp_resolve(sr, hop, bpm_min, bpm_max); }
int32_t zltp_result_bytes(void) { return (int32_t)sizeof(ZlTpResult); }

// A call of nreq requests over hand-made or computed energies.  hops, rate, hop, bpm_min, bpm_max: [nreq]; E: the requests' energies
// one behind the other.  W [sum of hops], A [capacity], geom [nreq][8] = (lmin, lmax, cap, first_lag, nlags, acf_base, items, nsegs),
// out [nreq] records (bpm and confidence finished), counts [nreq] pointers (each null or [nlags][hops] zeroed bytes) or null,
// walk [3] = (products entered, indices refused, staged words that are not the hop the lane means).  Returns the lags used, or -1 if
// `capacity` is too small.
int64_t zltp_call(int32_t nreq, const int32_t *hops, const double *rate, const int32_t *hop, const float *bpm_min, const float *bpm_max, const uint64_t *E,
                  uint16_t *W, uint64_t *A, int64_t capacity, int32_t *geom, ZlTpResult *out, uint8_t *const *counts, int64_t *walk)
{
    std::vector<ZlTpRequest> reqs((size_t)nreq);
    int64_t nh = 0, nl = 0, items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlTpRequest &T = reqs[(size_t)i];
        double lmin, lmax;
        zl_tp_lags(rate[i], hop[i], bpm_min[i], bpm_max[i], &lmin, &lmax);
        zl_tp_geometry(&T, hops[i], lmin, lmax);
        T.hop_base = (int32_t)nh; T.acf_base = (int32_t)nl; T.item_base = (int32_t)items;
        const int32_t g[8] = {T.lmin, T.lmax, T.cap, T.first_lag, T.nlags, T.acf_base, zl_tp_items(T), T.nsegs};
        std::memcpy(geom + 8 * i, g, sizeof(g));
        nh += T.hops; nl += T.nlags; items += zl_tp_items(T);
    }
    if (nl > capacity) return -1;
    std::vector<ZlTpStat> st((size_t)nreq);
    for (int32_t i = nreq - 1; i >= 0; --i) flux(reqs[(size_t)i], E + reqs[(size_t)i].hop_base, W + reqs[(size_t)i].hop_base, A + reqs[(size_t)i].acf_base, &st[(size_t)i]);
    Walk w;
    for (int64_t it = items - 1; it >= 0; --it) acf_item(reqs.data(), nreq, (int32_t)it, W, A, counts, w);      // (any order: integer sums)
    for (int32_t i = 0; i < nreq; ++i) {
        pick(reqs[(size_t)i], A + reqs[(size_t)i].acf_base, st[(size_t)i], &out[i]);
        zl_tp_finish(rate[i], hop[i], &out[i]);
    }
    walk[0] = w.products; walk[1] = w.refused; walk[2] = w.mismatched;
    return nl;
}

// the whole request over planar data (right: null for a mono clip), straight sums, the energies on `threads` threads; returns 0
int32_t zltp_run_planar(const float *left, const float *right, int32_t first, int32_t frames, double rate, int32_t hop, float bpm_min, float bpm_max, int32_t threads,
                        ZlTpResult *out)
{
    if (zl_tp_resolve(rate, &hop, &bpm_min, &bpm_max) != 0) return -1;
    const int32_t hops = (int32_t)zl_on_hops(frames, hop);
    std::vector<uint64_t> E((size_t)hops);
    auto work = [&](int32_t t) {
        for (int32_t h = (int32_t)((int64_t)hops * t / threads); h < (int32_t)((int64_t)hops * (t + 1) / threads); ++h) {
            int64_t lo, hi;
            zl_on_hop_range(first, frames, hop, h, &lo, &hi);
            uint64_t s = 0;
            for (int64_t f = lo; f < hi; ++f) s += (uint64_t)zl_on_sq(left[f]) + (right ? (uint64_t)zl_on_sq(right[f]) : 0u);
            E[(size_t)h] = s;
        }
    };
    std::vector<std::thread> pool;
    for (int32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    ZlTpRequest R;
    double lmin, lmax;
    zl_tp_lags(rate, hop, bpm_min, bpm_max, &lmin, &lmax);
    zl_tp_geometry(&R, hops, lmin, lmax);
    R.hop_base = 0; R.acf_base = 0; R.item_base = 0;
    std::vector<uint16_t> W((size_t)hops);
    std::vector<uint64_t> A((size_t)std::max(R.nlags, 1));
    ZlTpStat st;
    flux(R, E.data(), W.data(), A.data(), &st);
    for (int32_t l = 0; l < R.nlags; ++l) {
        const int32_t lag = R.first_lag + l;
        uint64_t acc = 0;
        for (int32_t h = lag; h < hops; ++h) acc += (uint64_t)W[(size_t)h] * (uint64_t)W[(size_t)(h - lag)];
        A[(size_t)l] = acc;
    }
    pick(R, A.data(), st, out);
    zl_tp_finish(rate, hop, out);
    return 0;
}

}
