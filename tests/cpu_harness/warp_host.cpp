// Host build of zl_warp.h for the CPU tier (tests/test_warp_cpu.py, tests/cpp/warp_check.cpp): a call walked the way the kernels walk
// it -- the seek one workgroup per stretched region with more than one segment, window and weighted reference staged in arrays of the
// kernel's sizes, the synthesis workgroup by workgroup (found by the bisection over wg_base) and lane by lane from the workgroup's first
// region -- with the header's own arithmetic, a count of the writes per float of every extent, and a source that is read through an
// accessor which checks the float's index against the buffer it was given and refuses what lies outside.
#include <limits.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_warp.h"

namespace {
// a clip's floats as the caller handed them over; a read outside them is counted and answered with a NaN, so that it also shows in the bits
struct Source {
    const float *p; int64_t floats; int64_t len; int ch; int64_t *refused;
    float operator()(int64_t n, int c) const
    {
        if (n >= len) return 0.0f;
        const int64_t index = n * ch + c;
        if (n < 0 || index >= floats) { *refused += 1; return __builtin_nanf(""); }
        return p[index];
    }
};
}  // namespace

extern "C" {

int zlwp_resolve(double rate, int32_t length, const zlhip_warp_anchor *an, int32_t count, zlhip_warp *out)
{
    ZlWpSummary s;
    if (zl_wp_resolve(rate, length, (const ZlWpAnchor *)an, count, &s, nullptr) != 0) return -1;
    memcpy(out, &s, sizeof s);
    return 0;
}

int zlwp_plan(double rate, int32_t length, const int32_t *onsets, int32_t n, double src_bpm, double dst_bpm, int32_t steps, double strength, int32_t origin,
              int32_t preroll, zlhip_warp_anchor *out, int32_t capacity, int32_t *count, int32_t *dropped)
{
    return zl_wp_plan(rate, length, onsets, n, src_bpm, dst_bpm, steps, strength, origin, preroll, (ZlWpAnchor *)out, capacity, count, dropped);
}

int64_t zlwp_map(const zlhip_warp_anchor *an, int32_t count, int64_t src) { return zl_wp_map((const ZlWpAnchor *)an, count, src); }
int64_t zlwp_extent_floats(int64_t N, int32_t channels) { return zl_wp_extent_floats(N, channels); }

// One call.  Request i is clip i: counts[i] anchors at anchors[i]; data[i]: the clip's interleaved floats, src_floats[i] of them (the
// accessor's bound: length * channels where the caller is exact); dst[i], writes[i]: the extent's floats of an applied request;
// offsets[i]: the request's seek offsets (its summary's `segments`), may be null; verdicts[i]: in: 1 where the original lacks
// ZL_SOUND_FINITE, out: the clip's word.  walk: seek workgroups, synthesis workgroups, segments searched, reads refused.
// Returns the number of applied requests, -1 on a request that does not resolve, -2 where the walk leaves a buffer of its own.
int32_t zlwp_call(int32_t nreq, const int32_t *counts, const zlhip_warp_anchor *const *anchors, const float *const *data, const int64_t *src_floats,
                  const int32_t *length, const int32_t *channels, const double *rate, float *const *dst, int32_t *const *writes, zlhip_warp *out,
                  int32_t *const *offsets, uint32_t *verdicts, int64_t *walk)
{
    walk[0] = walk[1] = walk[2] = walk[3] = 0;
    std::vector<ZlWpJob> jobs; std::vector<ZlWpRegion> table; std::vector<int32_t> seekList, jobReq;
    int32_t wgs = 0, offs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlWpSummary s;
        std::vector<ZlWpRegion> regs((size_t)(counts[i] > 1 && counts[i] <= ZL_WP_MAX_ANCHORS ? counts[i] - 1 : 0));
        if (zl_wp_resolve(rate[i], length[i], (const ZlWpAnchor *)anchors[i], counts[i], &s, regs.data()) != 0) return -1;
        memcpy(&out[i], &s, sizeof s);
        if (!s.applied) continue;
        ZlWpJob J; memset(&J, 0, sizeof J);
        J.len = length[i]; J.channels = channels[i]; J.N = s.length; J.O = s.overlap;
        J.region_base = (int32_t)table.size(); J.nregions = s.regions; J.wg_base = wgs; J.verdict = (int32_t)jobs.size();
        wgs += zl_wp_job_wgs(J);
        for (ZlWpRegion R : regs) {
            R.off_base += offs; R.job = J.verdict;
            if (R.nseg > 1) seekList.push_back((int32_t)table.size());
            table.push_back(R);
        }
        offs += s.segments;
        jobs.push_back(J); jobReq.push_back(i);
    }
    const int32_t njobs = (int32_t)jobs.size();
    if (njobs == 0) return 0;
    std::vector<int32_t> off((size_t)offs, 0);                     // (zeroed, as the engine zeroes the call's offsets)
    // the seek kernel: one workgroup per listed region
    std::vector<int32_t> sIn(2 * ZL_ST_MAX_WINDOW), sRef(2 * ZL_ST_OVERLAP_MAX);
    for (size_t w = 0; w < seekList.size(); ++w) {
        const ZlWpRegion R = table[(size_t)seekList[w]];
        const ZlWpJob &J = jobs[(size_t)R.job];
        const int32_t i = jobReq[(size_t)R.job];
        const Source in = { data[i], src_floats[i], J.len, J.channels, &walk[3] };
        const int ch = J.channels, O = J.O, W = R.W, L = R.L;
        if (O > ZL_ST_OVERLAP_MAX || W + O > ZL_ST_MAX_WINDOW || R.off_base < 0 || R.off_base + R.nseg > offs) return -2;
        ++walk[0];
        off[(size_t)R.off_base] = 0;
        int64_t prev = R.a;
        for (int32_t k = 1; k < R.nseg; ++k) {
            const int64_t base = zl_wp_nominal(R, k);
            for (int t = 0; t < O; ++t)
                for (int c = 0; c < ch; ++c) sRef[(size_t)(c * ZL_ST_OVERLAP_MAX + t)] = zl_st_ref(zl_st_q(in(prev + L + t, c)), t, O);
            for (int j = 0; j < W + O; ++j)
                for (int c = 0; c < ch; ++c) sIn[(size_t)(c * ZL_ST_MAX_WINDOW + j)] = zl_st_q(in(base + j, c));
            double bs = -INFINITY; int32_t bo = INT_MAX;
            // (the lanes' order: lane t takes o = t, t + 512, ...; zl_st_better is a total order, so any order gives the same pick -- walked
            // backwards here so that the tie rule, not the order, has to pick the smallest offset)
            for (int o = W - 1; o >= 0; --o) {
                int64_t corr = 0, norm = 0;
                for (int c = 0; c < ch; ++c) {
                    const int32_t *x = &sIn[(size_t)(c * ZL_ST_MAX_WINDOW + o)], *r = &sRef[(size_t)(c * ZL_ST_OVERLAP_MAX)];
                    for (int t = 0; t < O; t += 2) {
                        const int32_t x0 = x[t], x1 = x[t + 1];
                        corr += (int64_t)(r[t] * x0 + r[t + 1] * x1);
                        norm += (int64_t)(x0 * x0 + x1 * x1);
                    }
                }
                const double s = zl_st_score(corr, norm);
                if (zl_st_better(s, o, bs, bo)) { bs = s; bo = o; }
            }
            off[(size_t)(R.off_base + k)] = bo;
            prev = base + bo;
            ++walk[2];
        }
    }
    // the synthesis kernel: the workgroups of the call
    for (int32_t wg = 0; wg < wgs; ++wg) {
        int32_t r = 0;
        for (int32_t lo = 0, hi = njobs - 1; ; ) {
            if (lo >= hi) { r = lo; break; }
            const int32_t mid = (lo + hi + 1) >> 1;
            if (jobs[(size_t)mid].wg_base <= wg) lo = mid; else hi = mid - 1;
        }
        const ZlWpJob &J = jobs[(size_t)r];
        const int32_t i = jobReq[(size_t)r];
        if (wg - J.wg_base >= zl_wp_job_wgs(J)) return -2;
        const ZlWpRegion *regs = table.data() + J.region_base;
        const Source in = { data[i], src_floats[i], J.len, J.channels, &walk[3] };
        const int64_t floats = zl_wp_extent_floats(J.N, J.channels), n0 = (int64_t)(wg - J.wg_base) * ZL_WP_SYNTH_THREADS;
        ++walk[1];
        for (int32_t tid = 0; tid < ZL_WP_SYNTH_THREADS; ++tid) {
            const int64_t n = n0 + tid;
            if (!(n < zl_wp_lanes(J))) continue;
            float y[2] = {0.0f, 0.0f};
            if (n < J.N) {
                int32_t ri = zl_wp_find_region(regs, J.nregions, (int32_t)(n0 < J.N ? n0 : 0));
                while (ri + 1 < J.nregions && regs[ri + 1].d <= (int32_t)n) ++ri;
                if (!(regs[ri].d <= n && n < (int64_t)regs[ri].d + regs[ri].D)) return -2;
                const ZlWpTap t = zl_wp_tap(regs, ri, off.data(), J.O, (int32_t)n);
                for (int c = 0; c < J.channels; ++c) {
                    y[c] = zl_wp_sample(t, J.O, c, in);
                    if (!zl_wp_finite(y[c])) verdicts[i] |= 1u;
                }
            }
            for (int c = 0; c < J.channels; ++c) {
                const int64_t f = n * J.channels + c;
                if (f < 0 || f >= floats) return -2;
                dst[i][f] = y[c];
                writes[i][f] += 1;
            }
        }
    }
    for (int32_t r = 0; r < njobs; ++r) {
        const int32_t i = jobReq[(size_t)r];
        if (offsets[i]) memcpy(offsets[i], off.data() + table[(size_t)jobs[(size_t)r].region_base].off_base, (size_t)out[i].segments * sizeof(int32_t));
    }
    return njobs;
}

}  // extern "C"
