// Host build of zl_xfade.h for the CPU tier (tests/test_xfade_cpu.py, tests/cpp/xfade_check.cpp): a call walked the way the kernels
// walk it -- the measuring workgroup chunk by chunk and group by group through zl_ov_groups / zl_pt_group_mix, the render kernel
// workgroup by workgroup (found by the bisection over wg_base) and group by group -- with the header's own arithmetic, a count of the
// writes per float of every extent, and a source that is read through an accessor which knows nothing of the masks: it checks the
// float's index against the buffer it was given and refuses what lies outside.
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_xfade.h"

namespace {
// a clip's floats as the caller handed them over; a read outside them is counted and answered with a NaN, so that it also shows in the bits
struct Source {
    const float *p; int64_t floats; int64_t *refused;
    float at(int64_t index)
    {
        if (index < 0 || index >= floats) { *refused += 1; return __builtin_nanf(""); }
        return p[index];
    }
};

// frames [lo, hi) of the clip mixed into out[0 .. hi - lo), as zl_xf_mix_span does it (zl_xfade.hip): the elements the mask lets
// through are the only ones looked at
void mix_span(const ZlXfJob &J, Source &S, int32_t lo, int32_t hi, int32_t *out, int64_t *refused)
{
    int64_t f0, f1, g0, g1;
    zl_ov_groups(lo, hi, J.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    for (int32_t g = 0; g < ngroups; ++g) {
        float v[4];
        for (int j = 0; j < 4; ++j) {
            const uint32_t nan = 0x7fc00000u;
            memcpy(&v[j], &nan, 4);
            if (zl_ov_valid(g, j, head, count)) v[j] = S.at(4 * (g0 + g) + j);
        }
        int32_t m[4], idx[4];
        zl_pt_group_mix(v[0], v[1], v[2], v[3], g, head, count, J.channels, m, idx);
        for (int j = 0; j < 4; ++j) {
            if (idx[j] < 0) continue;
            if (idx[j] >= hi - lo || idx[j] >= ZL_XF_CHUNK) { *refused += 1; continue; }
            out[idx[j]] = m[j];
        }
    }
}
}  // namespace

extern "C" {

int zlxf_resolve(double rate, int32_t length, zlhip_xfade_request *q)
{
    int32_t X = q->fade_frames;
    if (zl_xf_resolve(rate, length, q->start_frame, q->stop_frame, &X, q->curve) != 0) return -1;
    q->fade_frames = X;
    return 0;
}

void zlxf_finish(int64_t sab, int64_t saa, int64_t sbb, double *corr, double *rho) { zl_xf_finish(sab, saa, sbb, corr, rho); }
void zlxf_design(int32_t X, double rho, float *ab) { zl_xf_design(X, rho, ab); }
int64_t zlxf_extent_floats(int64_t length, int32_t channels) { return zl_xf_extent_floats(length, channels); }

// One call.  reqs: the requests (id is ignored: request i is clip i); data[i]: clip i's interleaved floats, src_floats[i] of them (the
// accessor's bound: length * channels where the caller is exact); dst[i], writes[i]: the extent's floats of an applied request (may be
// null for one that is not).  out[i]: the result; weights[i]: [2 X] or null; verdicts[i]: in: 1 where the original lacks
// ZL_SOUND_FINITE, out: the clip's word.  walk: groups loaded, groups faded, workgroups, reads refused.
// Returns the number of applied requests, -1 on a request that does not resolve, -2 where the walk leaves a buffer of its own.
int32_t zlxf_call(int32_t nreq, const zlhip_xfade_request *reqs, const float *const *data, const int64_t *src_floats, const int32_t *length, const int32_t *channels,
                  const double *rate, float *const *dst, int32_t *const *writes, zlhip_xfade *out, float *const *weights, uint32_t *verdicts, int64_t *walk)
{
    walk[0] = walk[1] = walk[2] = walk[3] = 0;
    std::vector<ZlXfJob> jobs; std::vector<int32_t> jobReq;
    int32_t wgs = 0, pairs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_xfade_request q = reqs[i];
        if (zlxf_resolve(rate[i], length[i], &q) != 0) return -1;
        memset(&out[i], 0, sizeof out[i]);
        if (q.fade_frames == 0) continue;
        ZlXfJob J; memset(&J, 0, sizeof J);
        J.length = length[i]; J.channels = channels[i]; J.s = q.start_frame; J.e = q.stop_frame; J.X = q.fade_frames;
        J.wg_base = wgs; J.weights = pairs; J.verdict = (int32_t)jobs.size();
        wgs += zl_xf_job_wgs(J); pairs += J.X;
        out[i].applied = 1; out[i].fade_frames = J.X; out[i].start_frame = J.s; out[i].stop_frame = J.e; out[i].curve = q.curve;
        jobs.push_back(J); jobReq.push_back(i);
    }
    const int32_t njobs = (int32_t)jobs.size();
    if (njobs == 0) return 0;
    // the measuring kernel: one workgroup per job
    std::vector<float> table((size_t)pairs * 2);
    std::vector<int32_t> sA(ZL_XF_CHUNK), sB(ZL_XF_CHUNK);
    for (int32_t r = 0; r < njobs; ++r) {
        const ZlXfJob &J = jobs[(size_t)r];
        const int32_t i = jobReq[(size_t)r];
        Source S = { data[i], src_floats[i], &walk[3] };
        int64_t ab = 0, aa = 0, bb = 0;
        for (int32_t c = 0; c < zl_xf_chunks(J.X); ++c) {
            int32_t i0, i1;
            zl_xf_chunk(J.X, c, &i0, &i1);
            if (i1 - i0 < 1 || i1 - i0 > ZL_XF_CHUNK) return -2;
            mix_span(J, S, J.e - J.X + i0, J.e - J.X + i1, sA.data(), &walk[3]);
            mix_span(J, S, J.s - J.X + i0, J.s - J.X + i1, sB.data(), &walk[3]);
            for (int32_t k = 0; k < i1 - i0; ++k) {
                const int64_t a = sA[(size_t)k], b = sB[(size_t)k];
                ab += a * b; aa += a * a; bb += b * b;
            }
        }
        double corr, rho;
        zl_xf_finish(ab, aa, bb, &corr, &rho);
        zlhip_xfade &o = out[i];
        o.sab = ab; o.saa = aa; o.sbb = bb; o.correlation = corr; o.rho = zl_xf_curve_rho(o.curve, rho);
        zl_xf_design(J.X, o.rho, table.data() + 2 * (size_t)J.weights);
        if (weights[i]) memcpy(weights[i], table.data() + 2 * (size_t)J.weights, (size_t)J.X * 2 * sizeof(float));
    }
    // the render kernel: the workgroups of the call
    for (int32_t wg = 0; wg < wgs; ++wg) {
        int32_t r = 0;
        for (int32_t lo = 0, hi = njobs - 1; ; ) {
            if (lo >= hi) { r = lo; break; }
            const int32_t mid = (lo + hi + 1) >> 1;
            if (jobs[(size_t)mid].wg_base <= wg) lo = mid; else hi = mid - 1;
        }
        const ZlXfJob &J = jobs[(size_t)r];
        const int32_t i = jobReq[(size_t)r];
        if (wg - J.wg_base >= zl_xf_job_wgs(J)) return -2;
        Source S = { data[i], src_floats[i], &walk[3] };
        const int64_t floats = zl_xf_extent_floats(J.length, J.channels);
        ++walk[2];
        for (int32_t tid = 0; tid < ZL_XF_WG; ++tid) {
            const int64_t g = (int64_t)(wg - J.wg_base) * ZL_XF_WG + tid;
            if (!(g < zl_xf_groups(J))) continue;
            const int64_t k0 = 4 * g, datafloats = zl_xf_data_floats(J);
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (zl_xf_group_loads(J, g)) {
                ++walk[0];
                for (int j = 0; j < 4; ++j) if (k0 + j < datafloats) y[j] = S.at(k0 + j);      // (the floats behind the data are produced zeros)
            }
            if (zl_xf_group_fades(J, g)) {
                ++walk[1];
                for (int j = 0; j < 4; ++j) {
                    const int64_t k = k0 + j;
                    if (!zl_xf_fades(J, k)) continue;
                    const int32_t w = zl_xf_weight_index(J, k);
                    if (w < 0 || w >= J.X) return -2;
                    const float *ab = table.data() + 2 * ((size_t)J.weights + (size_t)w);
                    y[j] = zl_xf_mix(ab[0], ab[1], y[j], S.at(zl_xf_b_index(J, k)));
                    if (!zl_xf_finite(y[j])) verdicts[i] |= 1u;
                }
            }
            for (int j = 0; j < 4; ++j) {
                if (k0 + j >= floats) return -2;
                dst[i][k0 + j] = y[j];
                writes[i][k0 + j] += 1;
            }
        }
    }
    return njobs;
}

}  // extern "C"
