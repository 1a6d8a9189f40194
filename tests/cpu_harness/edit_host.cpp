// Host build of zl_edit.h for the CPU tier (tests/test_edit_cpu.py, tests/cpp/edit_check.cpp): a call walked the way the kernels walk it
// -- the scanning workgroups chunk by chunk and group by group through zl_ov_groups / zl_ov_valid, the render kernel workgroup by
// workgroup (found by the bisection over wg_base) and group by group -- with the header's own arithmetic, a count of the writes per float
// of every extent, and a source that is read through an accessor which knows nothing of the masks: it checks the float's index against
// the buffer it was given and refuses what lies outside.
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_edit.h"

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

template <typename T> int32_t find(const std::vector<T> &recs, int32_t wg)
{
    for (int32_t lo = 0, hi = (int32_t)recs.size() - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (recs[(size_t)mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
}
}  // namespace

extern "C" {

int zled_resolve(int32_t length, zlhip_edit_request *q)
{
    static_assert(sizeof(zlhip_edit_request) == sizeof(ZlEdRequest), "the request's layout");
    ZlEdRequest r;
    memcpy(&r, q, sizeof r);
    if (zl_ed_resolve(length, &r) != 0) return -1;
    memcpy(q, &r, sizeof r);
    return 0;
}

void zled_design(int32_t X, int32_t curve, float *w) { zl_ed_design(X, curve, w); }
int64_t zled_extent_floats(int64_t length, int32_t channels) { return zl_ed_extent_floats(length, channels); }
int32_t zled_chunk(void) { return ZL_ED_CHUNK; }
int32_t zled_wg(void) { return ZL_ED_WG; }

// One call.  reqs: the requests (id is ignored: request i is clip i); data[i]: clip i's interleaved floats, src_floats[i] of them (the
// accessor's bound: length * channels where the caller is exact); dst[i], writes[i]: room for the extent's floats of the request's
// largest possible result (zled_extent_floats of its length).  out[i]: the result; w_in[i], w_out[i]: room for the asked fades' weights,
// or null; verdicts[i]: in: 1 where the original lacks ZL_SOUND_FINITE, out: the clip's word.
// walk: full groups loaded wide, groups faded, render workgroups, reads refused, scanning workgroups, weights loaded.
// Returns the number of applied requests, -1 on a request that does not resolve, -2 where the walk leaves a buffer of its own.
int32_t zled_call(int32_t nreq, const zlhip_edit_request *reqs, const float *const *data, const int64_t *src_floats, const int32_t *length, const int32_t *channels,
                  float *const *dst, int32_t *const *writes, zlhip_edit *out, float *const *w_in, float *const *w_out, uint32_t *verdicts, int64_t *walk)
{
    for (int k = 0; k < 6; ++k) walk[k] = 0;
    std::vector<zlhip_edit_request> res((size_t)nreq);
    std::vector<ZlEdScan> scans; std::vector<int32_t> scanReq;
    int32_t swgs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        res[(size_t)i] = reqs[i];
        zlhip_edit_request &q = res[(size_t)i];
        if (zled_resolve(length[i], &q) != 0) return -1;
        if (!(q.flags & ZL_ED_TRIM)) continue;
        ZlEdScan S; memset(&S, 0, sizeof S);
        S.channels = channels[i]; S.a = q.first_frame; S.b = q.first_frame + q.num_frames; S.threshold = q.threshold;
        S.wg_base = swgs; S.found = (int32_t)scans.size();
        swgs += zl_ed_scan_wgs(S);
        scans.push_back(S); scanReq.push_back(i);
    }
    // the scanning kernel: the workgroups of the call
    std::vector<ZlEdFound> found(scans.size(), ZlEdFound{ INT32_MAX, -1 });
    for (int32_t wg = 0; wg < swgs; ++wg) {
        const ZlEdScan &S = scans[(size_t)find(scans, wg)];
        const int32_t i = scanReq[(size_t)S.found];
        if (wg - S.wg_base >= zl_ed_scan_wgs(S)) return -2;
        Source src = { data[i], src_floats[i], &walk[3] };
        ++walk[4];
        int32_t lo, hi;
        zl_ed_chunk(S, wg - S.wg_base, &lo, &hi);
        if (lo < S.a || hi > S.b || hi - lo < 1 || hi - lo > ZL_ED_CHUNK) return -2;
        int64_t f0, f1, g0, g1;
        zl_ov_groups(lo, hi, S.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        int32_t mn = INT32_MAX, mx = -1;
        for (int32_t tid = 0; tid < ZL_ED_WG; ++tid) {
            for (int32_t g = tid; g < ngroups; g += ZL_ED_WG) {
                for (int j = 0; j < 4; ++j) {
                    if (!zl_ov_valid(g, j, head, count)) continue;   // (the kernel loads the whole group; what the mask drops decides nothing)
                    if (!zl_ed_loud(src.at(4 * (g0 + g) + j), S.threshold)) continue;
                    const int32_t f = zl_ed_frame_of(4 * (g0 + g) + j, S.channels);
                    if (f < lo || f >= hi) return -2;
                    mn = f < mn ? f : mn; mx = f > mx ? f : mx;
                }
            }
        }
        if (mx >= 0) {
            ZlEdFound &o = found[(size_t)S.found];
            o.first = mn < o.first ? mn : o.first; o.last = mx > o.last ? mx : o.last;
        }
    }
    // the regions and the jobs
    std::vector<ZlEdJob> jobs; std::vector<int32_t> jobReq;
    int32_t wgs = 0, nw = 0;
    for (int32_t i = 0, k = 0; i < nreq; ++i) {
        const zlhip_edit_request &q = res[(size_t)i];
        const bool trim = (q.flags & ZL_ED_TRIM) != 0, reverse = (q.flags & ZL_ED_REVERSE) != 0;
        const ZlEdFound f = trim ? found[(size_t)k++] : ZlEdFound{ INT32_MAX, -1 };
        zlhip_edit &r = out[i];
        memset(&r, 0, sizeof r);
        r.curve = q.curve; r.first_loud = -1; r.last_loud = -1;
        int32_t a2, b2, Xi, Xo;
        if (!zl_ed_region(q.first_frame, q.first_frame + q.num_frames, trim, f.first, f.last, q.pre_roll_frames, q.hold_frames, &a2, &b2)) {
            r.silent = 1; r.first_frame = q.first_frame; r.num_frames = q.num_frames; r.length = length[i];
            continue;
        }
        if (trim) { r.first_loud = f.first; r.last_loud = f.last; }
        zl_ed_fades(b2 - a2, q.fade_in_frames, q.fade_out_frames, &Xi, &Xo);
        r.first_frame = a2; r.num_frames = b2 - a2; r.length = b2 - a2;
        if (zl_ed_identity(length[i], a2, b2 - a2, reverse, Xi, Xo)) continue;
        r.applied = 1; r.fade_in_frames = Xi; r.fade_out_frames = Xo; r.reversed = reverse ? 1 : 0;
        ZlEdJob J; memset(&J, 0, sizeof J);
        J.channels = channels[i]; J.a = a2; J.n = b2 - a2; J.reverse = reverse ? 1 : 0; J.Xi = Xi; J.Xo = Xo;
        J.wg_base = wgs; J.w_in = nw; J.w_out = nw + Xi; J.verdict = (int32_t)jobs.size();
        wgs += zl_ed_job_wgs(J); nw += Xi + Xo;
        jobs.push_back(J); jobReq.push_back(i);
    }
    const int32_t njobs = (int32_t)jobs.size();
    if (njobs == 0) return 0;
    std::vector<float> table((size_t)nw);
    for (int32_t r = 0; r < njobs; ++r) {
        const ZlEdJob &J = jobs[(size_t)r];
        const int32_t i = jobReq[(size_t)r];
        zl_ed_design(J.Xi, res[(size_t)i].curve, table.data() + J.w_in);
        zl_ed_design(J.Xo, res[(size_t)i].curve, table.data() + J.w_out);
        if (w_in[i] && J.Xi) memcpy(w_in[i], table.data() + J.w_in, (size_t)J.Xi * sizeof(float));
        if (w_out[i] && J.Xo) memcpy(w_out[i], table.data() + J.w_out, (size_t)J.Xo * sizeof(float));
    }
    // the render kernel: the workgroups of the call
    for (int32_t wg = 0; wg < wgs; ++wg) {
        const ZlEdJob &J = jobs[(size_t)find(jobs, wg)];
        const int32_t i = jobReq[(size_t)J.verdict];
        if (wg - J.wg_base >= zl_ed_job_wgs(J)) return -2;
        Source S = { data[i], src_floats[i], &walk[3] };
        const int64_t floats = zl_ed_extent_floats(J.n, J.channels), datafloats = zl_ed_data_floats(J);
        ++walk[2];
        for (int32_t tid = 0; tid < ZL_ED_WG; ++tid) {
            const int64_t g = (int64_t)(wg - J.wg_base) * ZL_ED_WG + tid;
            if (!(g < zl_ed_groups(J))) continue;
            const int64_t k0 = 4 * g;
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (zl_ed_group_full(J, g)) {
                ++walk[0];
                const int64_t first = zl_ed_group_first(J, g);
                float v[4];
                for (int m = 0; m < 4; ++m) v[m] = S.at(first + m);       // (one wide load)
                for (int j = 0; j < 4; ++j) {
                    if (first + zl_ed_lane(J, j) != zl_ed_src_index(J, k0 + j)) return -2;
                    y[j] = v[zl_ed_lane(J, j)];
                }
            } else if (zl_ed_group_loads(J, g)) {
                for (int j = 0; j < 4; ++j) if (k0 + j < datafloats) y[j] = S.at(zl_ed_src_index(J, k0 + j));
            }
            if (zl_ed_group_fades(J, g)) {
                ++walk[1];
                const int32_t per = 4 / J.channels, i0 = (int32_t)(k0 / J.channels);
                for (int32_t f = 0; f < per; ++f) {
                    if (i0 + f >= J.n) continue;
                    const int32_t w = zl_ed_weight_index(J, i0 + f);
                    if (w < 0) continue;
                    if (w >= nw) return -2;
                    ++walk[5];
                    for (int32_t c = 0; c < J.channels; ++c) {
                        float &s = y[f * J.channels + c];
                        s = table[(size_t)w] * s;
                        if (!zl_ed_finite(s)) verdicts[i] |= 1u;
                    }
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
