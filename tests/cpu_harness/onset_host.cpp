// Host build of the transient detection's definition (libzl_amd/csrc/zl_onset.h) for the CPU tier -- TEST HARNESS ONLY.
// zlon_energy walks a request the way zl_k_onset_energy does -- hop by hop, a hop's 16-byte groups lane by lane with the head and tail
// masked by zl_ov_valid -- with the header's own arithmetic and counts the visits of every word of the extent; zlon_pick does what
// zl_k_onset_pick does to one word per hop (novelty, the blocks' running maxima, the histogram and its cut-off, the compaction in hop
// order); zlon_refine is a kept hop's walk over its sub-blocks.  zlon_run_planar is the whole request over planar data on several
// threads: the host side of scripts/onset_bench.py.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "zl_onset.h"

extern "C" {

int32_t zlon_level(uint64_t x) { return zl_on_level(x); }
int32_t zlon_q(float v) { return zl_st_q(v); }
int32_t zlon_resolve(double sr, int32_t *five) { return zl_on_resolve(sr, &five[0], &five[1], &five[2], &five[3], &five[4]); }
int64_t zlon_hops(int64_t frames, int64_t hop) { return zl_on_hops(frames, hop); }

// data: the extent as floats, (length + 8) * channels words rounded up to 4 (interleaved, the pad behind the sound included).
// visits [extent words]: += 1 for every word that enters a sum.  E [hops].  Returns the largest word index LOADED (masked or not).
int64_t zlon_energy(const float *data, int32_t channels, int32_t first, int32_t frames, int32_t hop, int32_t *visits, uint64_t *E)
{
    const int64_t hops = zl_on_hops(frames, hop);
    int64_t top = -1;
    for (int64_t h = 0; h < hops; ++h) {
        int64_t lo, hi, f0, f1, g0, g1;
        zl_on_hop_range(first, frames, hop, h, &lo, &hi);
        zl_ov_groups(lo, hi, channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        uint64_t lanes[ZL_ON_WAVE] = {0};
        for (int32_t gb = 0; gb < ngroups; gb += ZL_ON_WAVE)
            for (int lane = 0; lane < ZL_ON_WAVE; ++lane) {
                const int32_t g = gb + lane;
                if (g >= ngroups) continue;                        // (the kernel's lanes behind the hop read its last group again and mask it)
                top = std::max(top, 4 * (g0 + g) + 3);
                uint32_t s = 0;
                for (int j = 0; j < 4; ++j)
                    if (zl_ov_valid(g, j, head, count)) { visits[4 * (g0 + g) + j] += 1; s += zl_on_sq(data[4 * (g0 + g) + j]); }
                lanes[lane] += s;
            }
        uint64_t acc = 0;
        for (int lane = ZL_ON_WAVE - 1; lane >= 0; --lane) acc += lanes[lane];      // (any order: integers)
        E[h] = acc;
    }
    return top;
}

// N [hops] (out), kept [max_onsets] (out: the kept hops in hop order); returns their number.  cand (may be null): [hops] flags
int32_t zlon_pick(const uint64_t *E, int32_t hops, uint64_t floor_, int32_t threshold, int32_t gap, int32_t max_onsets, int32_t *N, int32_t *kept, uint8_t *cand)
{
    for (int32_t h = 0; h < hops; ++h) N[h] = zl_on_novelty(E[h], h > 0 ? E[h - 1] : 0, floor_);
    std::vector<uint32_t> ps((size_t)hops), hist(ZL_ON_LEVELS, 0u);
    for (int32_t b = 0; b < (hops + gap - 1) / gap; ++b) zl_on_scan_block(N, ps.data(), hops, gap, b);
    for (int32_t h = 0; h < hops; ++h) {
        const bool c = zl_on_candidate(N, ps.data(), hops, gap, threshold, h);
        if (cand) cand[h] = c;
        if (c) hist[(size_t)N[h]] += 1;
    }
    int32_t cut, quota;
    zl_on_cutoff(hist.data(), max_onsets, &cut, &quota);
    uint32_t above = 0, equal = 0;
    for (int32_t h = 0; h < hops; ++h) {
        if (!zl_on_candidate(N, ps.data(), hops, gap, threshold, h)) continue;
        const bool isAbove = N[h] > cut, isEqual = N[h] == cut;
        if (isAbove || (isEqual && equal < (uint32_t)quota)) kept[above + std::min<uint32_t>(equal, (uint32_t)quota)] = h;
        above += isAbove; equal += isEqual;
    }
    return (int32_t)(above + std::min<uint32_t>(equal, (uint32_t)quota));
}

}  // extern "C"

namespace {

struct Interleaved {
    const float *d; int ch;
    uint64_t e(int64_t f) const { uint64_t s = 0; for (int c = 0; c < ch; ++c) s += zl_on_sq(d[f * ch + c]); return s; }
};
struct Planar {
    const float *l, *r;
    uint64_t e(int64_t f) const { return (uint64_t)zl_on_sq(l[f]) + (r ? (uint64_t)zl_on_sq(r[f]) : 0u); }
};

template <typename Src> int32_t refine(const Src &src, int32_t first, int32_t frames, int32_t hop, int32_t h, const uint64_t *E, uint64_t floor_)
{
    const uint64_t ep = (h > 0 ? E[h - 1] : 0) + floor_;
    for (int s = 0; s < 2 * ZL_ON_SUBBLOCKS; ++s) {
        int64_t lo, hi;
        if (!zl_on_subblock(first, frames, hop, h, s, &lo, &hi)) continue;
        uint64_t es = 0;
        for (int64_t f = lo; f < hi; ++f) es += src.e(f);
        if (zl_on_hit(es, ep)) return (int32_t)lo;
    }
    return (int32_t)(first + (int64_t)h * hop);
}

}  // namespace

extern "C" {

int32_t zlon_refine(const float *data, int32_t channels, int32_t first, int32_t frames, int32_t hop, int32_t h, const uint64_t *E, uint64_t floor_)
{
    return refine(Interleaved{data, channels}, first, frames, hop, h, E, floor_);
}

// the whole request over planar data (right: null for a mono clip) on `threads` threads; out [max_onsets][2]; returns the count
int32_t zlon_run_planar(const float *left, const float *right, int32_t first, int32_t frames, int32_t hop, int32_t gate, int32_t threshold, int32_t gap,
                        int32_t max_onsets, int32_t threads, int32_t *out)
{
    const Planar src{left, right};
    const int32_t hops = (int32_t)zl_on_hops(frames, hop);
    std::vector<uint64_t> E((size_t)hops);
    auto work = [&](int32_t t) {
        for (int32_t h = (int32_t)((int64_t)hops * t / threads); h < (int32_t)((int64_t)hops * (t + 1) / threads); ++h) {
            int64_t lo, hi;
            zl_on_hop_range(first, frames, hop, h, &lo, &hi);
            uint64_t s = 0;
            for (int64_t f = lo; f < hi; ++f) s += src.e(f);
            E[(size_t)h] = s;
        }
    };
    std::vector<std::thread> pool;
    for (int32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    const uint64_t floor_ = zl_on_floor(hop, right ? 2 : 1, gate);
    std::vector<int32_t> N((size_t)hops), kept((size_t)max_onsets);
    const int32_t n = zlon_pick(E.data(), hops, floor_, threshold, gap, max_onsets, N.data(), kept.data(), nullptr);
    for (int32_t i = 0; i < n; ++i) {
        out[2 * i] = refine(src, first, frames, hop, kept[(size_t)i], E.data(), floor_);
        out[2 * i + 1] = N[(size_t)kept[(size_t)i]];
    }
    return n;
}

}
