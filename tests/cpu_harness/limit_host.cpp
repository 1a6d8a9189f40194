// Host build of zl_limit.h for the CPU tier (tests/test_limit_cpu.py, tests/cpp/limit_check.cpp): a call walked the way the kernels walk
// it -- the detecting workgroups chunk by chunk and group by group through zl_ov_groups / zl_ov_valid, the render kernel tile by tile
// (found by the bisection over wg_base), lane by lane, through the same staging arrays with the same indices -- with the header's own
// arithmetic, a count of the writes per float of every extent, staging arrays that refuse an index outside themselves, and a source that
// is read through an accessor which knows nothing of the masks: it checks the float's index against the buffer it was given.
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_limit.h"

namespace {
struct Source {
    const float *p; int64_t floats; int64_t *refused;
    float at(int64_t index)
    {
        if (index < 0 || index >= floats) { *refused += 1; return __builtin_nanf(""); }
        return p[index];
    }
};
// an LDS array: an index outside it is counted (and lands in a spare word)
template <typename T> struct Lds {
    std::vector<T> v; int64_t *refused;
    Lds(size_t n, int64_t *r) : v(n + 1), refused(r) {}
    T &operator[](int64_t i) { if (i < 0 || i >= (int64_t)v.size() - 1) { *refused += 1; return v.back(); } return v[(size_t)i]; }
    // 64 consecutive words from i, as the phase rows read them
    const T *window(int64_t i) { if (i < 0 || i + ZL_LM_TAPS > (int64_t)v.size() - 1) { *refused += 1; return nullptr; } return v.data() + i; }
};
template <typename T> int32_t find(const std::vector<T> &recs, int32_t wg)
{
    for (int32_t lo = 0, hi = (int32_t)recs.size() - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (recs[(size_t)mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
}

// the detecting kernel over the requests; records [wgs].  walk[3]: reads refused, walk[4]: detecting workgroups.  0, or -2
int detect(const std::vector<ZlLmScan> &scans, const std::vector<Source> &srcs, int32_t wgs, const float *tables, ZlLmRecord *records, int32_t *rec_writes, int64_t *walk)
{
    for (int32_t wg = 0; wg < wgs; ++wg) {
        const int32_t ri = find(scans, wg);
        const ZlLmScan &S = scans[(size_t)ri];
        Source src = srcs[(size_t)ri];
        if (wg - S.wg_base >= zl_lm_chunks(S.b - S.a)) return -2;
        ++walk[4];
        const bool tp = S.F > 1;
        int32_t lo, hi, s0, s1;
        zl_lm_chunk(S, wg - S.wg_base, &lo, &hi, &s0, &s1);
        if (lo < S.a || hi > S.b || hi - lo < 1 || s0 < S.a || s1 > S.b) return -2;
        const int32_t base = lo - (ZL_LM_HALF - 1);
        Lds<float> sV0(ZL_LM_DET_STAGE, &walk[3]), sV1(ZL_LM_DET_STAGE, &walk[3]);
        int64_t f0, f1, g0, g1;
        zl_ov_groups(s0, s1, S.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        uint32_t m[4] = {0u, 0u, 0u, 0u};
        for (int32_t g = 0; g < ngroups; ++g) {
            for (int j = 0; j < 4; ++j) {
                if (!zl_ov_valid(g, j, head, count)) continue;     // (the kernel loads the whole group; what the mask drops decides nothing)
                const int64_t idx = 4 * (g0 + g) + j;
                const int32_t f = (int32_t)(S.channels == 2 ? idx >> 1 : idx), c = S.channels == 2 ? (int32_t)(idx & 1) : 0;
                if (f < s0 || f >= s1) return -2;
                const float v = zl_lm_v(src.at(idx), S.gain, S.sanitize);
                if (tp) (c ? sV1 : sV0)[f - base] = v;
                if (f >= lo && f < hi) m[c] = zl_lm_max_bits(m[c], zl_lm_abs_bits(v));
            }
        }
        if (tp) {
            const float *table = tables + zl_lm_table_at(S.F);
            for (int32_t f = lo; f < hi; ++f) {
                for (int32_t c = 0; c < S.channels; ++c) {
                    const float *win = (c ? sV1 : sV0).window(f - lo);
                    if (!win) return -2;
                    m[2 + c] = zl_lm_max_bits(m[2 + c], zl_lm_ips_bits(table, S.F, win));
                }
            }
        }
        ZlLmRecord &o = records[wg];
        o.sample_peak[0] = zl_lm_float(m[0]); o.sample_peak[1] = zl_lm_float(m[1]); o.inter_peak[0] = zl_lm_float(m[2]); o.inter_peak[1] = zl_lm_float(m[3]);
        rec_writes[wg] += 1;
    }
    return 0;
}
}  // namespace

extern "C" {

int zllm_resolve(double rate, zlhip_limit_request *q)
{
    static_assert(sizeof(zlhip_limit_request) == sizeof(ZlLmRequest), "the request's layout");
    ZlLmRequest r;
    memcpy(&r, q, sizeof r);
    if (zl_lm_resolve(rate, &r) != 0) return -1;
    memcpy(q, &r, sizeof r);
    return 0;
}
int zllm_peak_resolve(double rate, int32_t length, const zlhip_peak_request *q)
{
    static_assert(sizeof(zlhip_peak_request) == sizeof(ZlLmPeakRequest), "the request's layout");
    ZlLmPeakRequest r;
    memcpy(&r, q, sizeof r);
    return zl_lm_peak_resolve(rate, length, &r);
}
void zllm_design(int32_t L, float *w) { zl_lm_design(L, w); }
void zllm_tables(float *t) { zl_lm_tables(t); }
int32_t zllm_table_at(int32_t F) { return zl_lm_table_at(F); }
int32_t zllm_oversampling(double rate) { return zl_lm_oversampling(rate); }
int64_t zllm_extent_floats(int64_t length, int32_t channels) { return zl_lm_extent_floats(length, channels); }
int32_t zllm_chunk(void) { return ZL_LM_CHUNK; }
int32_t zllm_tile(void) { return ZL_LM_TILE; }
int32_t zllm_wg(void) { return ZL_LM_WG; }

// The analysis of one call.  reqs[i] over data[i] (src_floats[i] floats, `length[i]` frames, channels[i], rate[i]); records: room for
// every request's chunks, one behind the other; rec_writes: as many counters.  out[i]: the result.  Returns the records written,
// -1 on a request that does not resolve, -2 where the walk leaves a buffer of its own.  walk as zllm_call's
int32_t zllm_peak_call(int32_t nreq, const zlhip_peak_request *reqs, const float *const *data, const int64_t *src_floats, const int32_t *length, const int32_t *channels,
                       const double *rate, zlhip_peak *out, ZlLmRecord *records, int32_t *rec_writes, int64_t *walk)
{
    for (int k = 0; k < 8; ++k) walk[k] = 0;
    std::vector<float> tables(ZL_LM_TABLE_FLOATS);
    zl_lm_tables(tables.data());
    std::vector<ZlLmScan> scans; std::vector<Source> srcs;
    int32_t wgs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        if (zllm_peak_resolve(rate[i], length[i], &reqs[i]) != 0) return -1;
        ZlLmScan S; memset(&S, 0, sizeof S);
        S.channels = channels[i]; S.a = reqs[i].first_frame; S.b = reqs[i].first_frame + reqs[i].num_frames; S.wg_base = wgs;
        S.F = (reqs[i].flags & ZL_LM_TRUE_PEAK) ? zl_lm_oversampling(rate[i]) : 1; S.sanitize = 1; S.gain = 1.0f;
        wgs += zl_lm_chunks(S.b - S.a);
        scans.push_back(S); srcs.push_back(Source{ data[i], src_floats[i], &walk[3] });
    }
    if (detect(scans, srcs, wgs, tables.data(), records, rec_writes, walk) != 0) return -2;
    for (int32_t i = 0; i < nreq; ++i) {
        const ZlLmScan &S = scans[(size_t)i];
        uint32_t m[4] = {0u, 0u, 0u, 0u};
        for (int32_t k = 0; k < zl_lm_chunks(S.b - S.a); ++k) {
            const ZlLmRecord &r = records[S.wg_base + k];
            m[0] = zl_lm_max_bits(m[0], zl_lm_bits(r.sample_peak[0])); m[1] = zl_lm_max_bits(m[1], zl_lm_bits(r.sample_peak[1]));
            m[2] = zl_lm_max_bits(m[2], zl_lm_bits(r.inter_peak[0])); m[3] = zl_lm_max_bits(m[3], zl_lm_bits(r.inter_peak[1]));
        }
        zlhip_peak &o = out[i];
        o.sample_peak[0] = zl_lm_float(m[0]); o.sample_peak[1] = zl_lm_float(m[1]);
        o.true_peak[0] = zl_lm_float(zl_lm_max_bits(m[0], m[2])); o.true_peak[1] = zl_lm_float(zl_lm_max_bits(m[1], m[3]));
        o.oversampling = S.F; o.chunks = zl_lm_chunks(S.b - S.a);
    }
    return wgs;
}

// One limiter call.  reqs (id is ignored: request i is clip i); data[i]: clip i's interleaved floats, src_floats[i] of them (the accessor's
// bound); dst[i], writes[i]: room for zllm_extent_floats floats; out[i]: the result; verdicts[i]: out: the clip's word.
// walk: 0 cold tiles, 1 hot tiles, 2 render workgroups, 3 reads or LDS indices refused, 4 detecting workgroups, 5 cold tiles with a hot
// frame in reach (must stay 0), 6 hot tiles without one, 7 records not written exactly once.
// Returns the number of applied requests, -1 on a request that does not resolve, -2 where the walk leaves a buffer of its own.
int32_t zllm_call(int32_t nreq, const zlhip_limit_request *reqs, const float *const *data, const int64_t *src_floats, const int32_t *length, const int32_t *channels,
                  const double *rate, float *const *dst, int32_t *const *writes, zlhip_limit *out, uint32_t *verdicts, int64_t *walk)
{
    for (int k = 0; k < 8; ++k) walk[k] = 0;
    std::vector<float> tables(ZL_LM_TABLE_FLOATS);
    zl_lm_tables(tables.data());
    std::vector<zlhip_limit_request> res((size_t)nreq);
    std::vector<ZlLmScan> scans; std::vector<Source> srcs;
    int32_t swgs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        res[(size_t)i] = reqs[i];
        if (zllm_resolve(rate[i], &res[(size_t)i]) != 0 || length[i] < 1) return -1;
        const zlhip_limit_request &q = res[(size_t)i];
        ZlLmScan S; memset(&S, 0, sizeof S);
        S.channels = channels[i]; S.a = 0; S.b = length[i]; S.wg_base = swgs;
        S.F = (q.flags & ZL_LM_TRUE_PEAK) ? zl_lm_oversampling(rate[i]) : 1; S.sanitize = 0; S.gain = q.gain;
        swgs += zl_lm_chunks(length[i]);
        scans.push_back(S); srcs.push_back(Source{ data[i], src_floats[i], &walk[3] });
    }
    std::vector<ZlLmRecord> records((size_t)swgs);
    std::vector<int32_t> recWrites((size_t)swgs, 0);
    if (detect(scans, srcs, swgs, tables.data(), records.data(), recWrites.data(), walk) != 0) return -2;
    for (int32_t k = 0; k < swgs; ++k) if (recWrites[(size_t)k] != 1) ++walk[7];
    // the jobs
    std::vector<ZlLmJob> jobs; std::vector<int32_t> jobReq;
    std::vector<float> weights;
    int32_t wgs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        const zlhip_limit_request &q = res[(size_t)i];
        const ZlLmScan &S = scans[(size_t)i];
        uint32_t peak = 0u;
        for (int32_t k = 0; k < zl_lm_chunks(length[i]); ++k) peak = zl_lm_max_bits(peak, zl_lm_record_bits(records[(size_t)(S.wg_base + k)]));
        zlhip_limit &r = out[i];
        memset(&r, 0, sizeof r);
        r.lookahead_frames = q.lookahead_frames; r.hold_frames = q.hold_frames; r.oversampling = S.F; r.peak_before = zl_lm_float(peak);
        r.min_gain = 1.0f; r.ceiling = q.ceiling; r.gain = q.gain;
        verdicts[i] = 0u;
        if (q.gain == 1.0f && !(peak > zl_lm_bits(q.ceiling))) continue;
        r.applied = 1;
        ZlLmJob J; memset(&J, 0, sizeof J);
        J.channels = channels[i]; J.n = length[i]; J.L = q.lookahead_frames; J.H = q.hold_frames; J.F = S.F; J.ceiling = q.ceiling; J.gain = q.gain;
        J.wg_base = wgs; J.rec_base = S.wg_base; J.weights = (int32_t)weights.size(); J.verdict = (int32_t)jobs.size();
        weights.resize(weights.size() + (size_t)J.L + 1);
        zl_lm_design(J.L, weights.data() + J.weights);
        wgs += zl_lm_job_tiles(J);
        jobs.push_back(J); jobReq.push_back(i);
    }
    const int32_t njobs = (int32_t)jobs.size();
    if (njobs == 0) return 0;
    std::vector<ZlLmStats> stats((size_t)njobs, ZlLmStats{ 0u, 0x3f800000u });
    // the render kernel: the workgroups of the call
    for (int32_t wg = 0; wg < wgs; ++wg) {
        const ZlLmJob &J = jobs[(size_t)find(jobs, wg)];
        const int32_t i = jobReq[(size_t)J.verdict];
        if (wg - J.wg_base >= zl_lm_job_tiles(J)) return -2;
        Source S = { data[i], src_floats[i], &walk[3] };
        ++walk[2];
        const int32_t t0 = (wg - J.wg_base) * ZL_LM_TILE;
        const bool stereo = J.channels == 2;
        const float c = J.ceiling;
        const bool hot = !zl_lm_tile_cold(J, records.data() + J.rec_base, t0);
        ++walk[hot ? 1 : 0];
        const int32_t NR = zl_lm_reach_frames(J), NM = zl_lm_mr_count(J), j0 = t0 - J.L - J.H;
        const bool tp = J.F > 1;
        // what the definition says about the tile's reach, frame by frame (the check on the cold decision; sample peaks and, with the
        // flag, the records' inter-sample peaks cannot be asked per frame: a hot tile recomputes them below and is compared there)
        std::vector<float> G((size_t)ZL_LM_TILE, 1.0f);
        bool anyHot = false;
        if (hot) {
            Lds<float> sV0(ZL_LM_STAGE, &walk[3]), sV1(ZL_LM_STAGE, &walk[3]), sMr(4 * ZL_LM_MR_Q, &walk[3]);
            Lds<uint32_t> sIps(ZL_LM_MAX_REACH + 1, &walk[3]), sR(ZL_LM_MAX_REACH, &walk[3]);
            if (NR > ZL_LM_MAX_REACH || NM > ZL_LM_MAX_MR) return -2;
            if (tp) {
                for (int32_t idx = 0; idx < NR + ZL_LM_TAPS; ++idx) {
                    const int32_t f = j0 - ZL_LM_HALF + idx;
                    float a = 0.0f, b = 0.0f;
                    if (f >= 0 && f < J.n) {
                        if (stereo) { a = S.at(2 * (int64_t)f) * J.gain; b = S.at(2 * (int64_t)f + 1) * J.gain; }
                        else a = S.at(f) * J.gain;
                    }
                    sV0[idx] = a; sV1[idx] = b;
                }
                const float *table = tables.data() + zl_lm_table_at(J.F);
                for (int32_t idx = 0; idx < NR + 1; ++idx) {
                    const int32_t f = j0 - 1 + idx;
                    uint32_t b = 0u;
                    if (f >= 0 && f < J.n) {
                        const float *w0 = sV0.window(idx), *w1 = sV1.window(idx);
                        if (!w0 || !w1) return -2;
                        b = zl_lm_ips_bits(table, J.F, w0);
                        if (stereo) b = zl_lm_max_bits(b, zl_lm_ips_bits(table, J.F, w1));
                    }
                    sIps[idx] = b;
                }
            }
            for (int32_t q = 0; q < NR; ++q) {
                const int32_t f = j0 + q;
                uint32_t r = 0u;
                if (f >= 0 && f < J.n) {
                    uint32_t p;
                    if (tp) {
                        p = zl_lm_max_bits(zl_lm_abs_bits(sV0[q + ZL_LM_HALF]), zl_lm_abs_bits(sV1[q + ZL_LM_HALF]));
                        p = zl_lm_max_bits(p, zl_lm_max_bits(sIps[q], sIps[q + 1]));
                    } else if (stereo) {
                        p = zl_lm_max_bits(zl_lm_abs_bits(S.at(2 * (int64_t)f) * J.gain), zl_lm_abs_bits(S.at(2 * (int64_t)f + 1) * J.gain));
                    } else {
                        p = zl_lm_abs_bits(S.at(f) * J.gain);
                    }
                    r = zl_lm_bits(zl_lm_reduction(p, c));
                    anyHot = anyHot || r != 0u;
                }
                sR[q] = r;
            }
            // log-step doubling, every step from a copy: what the barriers between a step's reads and its writes give
            const int32_t W = J.L + J.H + 1, P = zl_lm_pow2(W);
            for (int32_t s = 1; s < P; s <<= 1) {
                std::vector<uint32_t> nb((size_t)NR);
                for (int32_t q = 0; q < NR; ++q) nb[(size_t)q] = q + s < NR ? (uint32_t)sR[q + s] : 0u;
                for (int32_t q = 0; q < NR; ++q) sR[q] = zl_lm_max_bits(sR[q], nb[(size_t)q]);
            }
            for (int32_t m = 0; m < NM; ++m) sMr[zl_lm_mr_pos(m)] = zl_lm_float(zl_lm_max_bits(sR[m], sR[m + W - P]));
            uint32_t reduced = 0u, mn = 0x3f800000u;
            for (int32_t tid = 0; tid < ZL_LM_WG; ++tid) {
                const int32_t m0 = ZL_LM_PER * tid + J.L;
                float win[ZL_LM_PER], acc[ZL_LM_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int32_t e = 0; e < ZL_LM_PER; ++e) win[e] = sMr[zl_lm_mr_pos(m0 + e)];
                for (int32_t k = 0; k <= J.L; ++k) {
                    const float wk = weights[(size_t)(J.weights + k)];
                    for (int32_t e = 0; e < ZL_LM_PER; ++e) { const float p = wk * win[e]; acc[e] = acc[e] + p; }
                    win[3] = win[2]; win[2] = win[1]; win[1] = win[0];
                    win[0] = k < J.L ? (float)sMr[zl_lm_mr_pos(m0 - k - 1)] : 0.0f;
                }
                for (int32_t e = 0; e < ZL_LM_PER; ++e) {
                    const float g = zl_lm_gain_of(acc[e]);
                    G[(size_t)(ZL_LM_PER * tid + e)] = g;
                    if (t0 + ZL_LM_PER * tid + e < J.n) {
                        reduced += g < 1.0f ? 1u : 0u;
                        mn = zl_lm_bits(g) < mn ? zl_lm_bits(g) : mn;
                    }
                }
            }
            if (reduced != 0u) {
                ZlLmStats &st = stats[(size_t)J.verdict];
                st.frames_reduced += reduced; st.min_gain_bits = mn < st.min_gain_bits ? mn : st.min_gain_bits;
            }
            if (!anyHot) ++walk[6];
        } else {
            // a cold tile: is any frame of its reach hot by the sample peak?  (the inter-sample part is the records' own)
            int32_t lo, hi;
            if (zl_lm_tile_reach(J, t0, &lo, &hi)) {
                for (int32_t f = lo; f <= hi; ++f)
                    for (int32_t ch = 0; ch < J.channels; ++ch)
                        if (fabsf(S.at((int64_t)f * J.channels + ch) * J.gain) > c) { ++walk[5]; f = hi; break; }
            }
        }
        const int64_t groups = zl_lm_groups(J), datafloats = (int64_t)J.n * J.channels, floats = zl_lm_extent_floats(J.n, J.channels);
        const int32_t per = stereo ? 2 : 1;
        for (int32_t tid = 0; tid < ZL_LM_WG; ++tid) {
            const int64_t gfirst = (int64_t)(wg - J.wg_base) * zl_lm_tile_groups(J.channels) + (int64_t)tid * per;
            for (int32_t h = 0; h < per; ++h) {
                const int64_t g = gfirst + h;
                if (!(g < groups)) continue;
                float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * g < datafloats) {
                    float x[4];
                    for (int j = 0; j < 4; ++j) x[j] = S.at(4 * g + j);                  // (one wide load: the whole group, pad included)
                    for (int j = 0; j < 4; ++j) {
                        if (4 * g + j >= datafloats) continue;
                        const float v = x[j] * J.gain;
                        const int32_t e = stereo ? 2 * h + (j >> 1) : j;
                        if ((4 * g + j) / J.channels != (int64_t)t0 + ZL_LM_PER * tid + e) return -2;
                        y[j] = hot ? zl_lm_apply(v, G[(size_t)(ZL_LM_PER * tid + e)], c) : v;
                        if (!zl_lm_finite(y[j])) verdicts[i] |= 1u;
                    }
                }
                for (int j = 0; j < 4; ++j) {
                    if (4 * g + j >= floats) return -2;
                    dst[i][4 * g + j] = y[j];
                    writes[i][4 * g + j] += 1;
                }
            }
        }
    }
    for (int32_t r = 0; r < njobs; ++r) {
        zlhip_limit &o = out[jobReq[(size_t)r]];
        o.frames_reduced = (int32_t)stats[(size_t)r].frames_reduced; o.min_gain = zl_lm_float(stats[(size_t)r].min_gain_bits);
    }
    return njobs;
}

}  // extern "C"
