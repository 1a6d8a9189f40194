// zl_edit.hip -- HIP kernels of the clip edit (zlhip_sound_edit / _batch; the definition is in zl_edit.h).
//
//   zl_k_edit_scan    the call's TRIM requests only.  A workgroup of ZL_ED_WG lanes reads one chunk of ZL_ED_CHUNK frames of one
//                     request's region and finds its request by bisection over the requests' wg_base with scalar loads.  The chunk's
//                     span is read in 16-byte groups of the arena's own layout, head and tail masked by float index: no float outside
//                     the region decides anything.  A lane keeps the smallest and the largest loud frame it saw; shuffles over the
//                     wave, LDS over the workgroup; its first lane sends one atomic min and one atomic max to the request's two words,
//                     and only where the chunk holds a loud frame.
//   zl_k_edit_render  the hot path, a copy from a source that is in general not 16-byte aligned to its destination, forwards or
//                     backwards: one lane per 16-byte group of the destination extent, a workgroup is ZL_ED_WG consecutive groups of
//                     one job, found by bisection.  A group that lies wholly inside the data is ONE dword-aligned 16-byte load (four
//                     consecutive source floats, zl_ed_group_first), a permutation in registers when the job reverses, and one aligned
//                     16-byte store.  The one group of a job that the data's end cuts loads its floats one by one, so that no load
//                     touches a float outside the kept region; the floats behind the data -- the zero frames and the pad -- are
//                     produced.  A group that overlaps a fade (the first Xi and the last Xo frames) reads one weight per faded frame
//                     and multiplies.  A clip's verdict on a non-finite faded sample: a ballot per wave, one atomic OR by its first
//                     lane, only when something is set.
//   (the sound-table entries switch by zl_k_resample_publish, zl_resample.hip)
//
// No scratch memory.  LDS: the render kernel none; the scanning kernel eight words for the reduction.
#include <hip/hip_runtime.h>
#include "zl_edit.h"

#define ZL_ED_WAVE 64
#define ZL_ED_WAVES (ZL_ED_WG / ZL_ED_WAVE)

namespace {

typedef float zl_ed_f4 __attribute__((ext_vector_type(4)));
// four floats at a dword-aligned address: one global_load_dwordx4 (the device takes any dword alignment for it)
typedef zl_ed_f4 zl_ed_f4u __attribute__((aligned(4)));
// the extents' addresses arrive as integers in the job record: tell the compiler that they are global memory
typedef const float __attribute__((address_space(1))) *ZlEdGlobalF;
typedef const zl_ed_f4 __attribute__((address_space(1))) *ZlEdGlobalF4;
typedef const zl_ed_f4u __attribute__((address_space(1))) *ZlEdGlobalF4u;
typedef zl_ed_f4 __attribute__((address_space(1))) *ZlEdGlobalOutF4;

// the record of workgroup wg: the last one whose wg_base is <= wg (wg_base is increasing, recs[0].wg_base == 0)
template <typename T> __device__ __forceinline__ int32_t zl_ed_find(const T *__restrict__ recs, int32_t n, int32_t wg)
{
    for (int32_t lo = 0, hi = n - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (recs[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
}

}  // namespace

__global__ void __launch_bounds__(ZL_ED_WG) zl_k_edit_scan(const ZlEdScan *__restrict__ reqs, int32_t nscan, ZlEdFound *__restrict__ found)
{
    __shared__ int32_t sMin[ZL_ED_WAVES];
    __shared__ int32_t sMax[ZL_ED_WAVES];
    const int32_t wg = (int32_t)blockIdx.x;
    const ZlEdScan S = reqs[zl_ed_find(reqs, nscan, wg)];
    const int tid = (int)threadIdx.x;
    int32_t lo, hi;
    zl_ed_chunk(S, wg - S.wg_base, &lo, &hi);
    int64_t f0, f1, g0, g1;
    zl_ov_groups(lo, hi, S.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const ZlEdGlobalF4 src = (ZlEdGlobalF4)S.src + g0;
    int32_t mn = INT32_MAX, mx = -1;
    for (int32_t g = tid; g < ngroups; g += ZL_ED_WG) {
        const zl_ed_f4 v = src[g];
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (zl_ov_valid(g, j, head, count) && zl_ed_loud(x[j], S.threshold)) {
                const int32_t f = zl_ed_frame_of(4 * (g0 + g) + j, S.channels);
                mn = f < mn ? f : mn; mx = f > mx ? f : mx;
            }
        }
    }
#pragma unroll
    for (int d = 1; d < ZL_ED_WAVE; d <<= 1) {
        const int32_t a = __shfl_xor(mn, d, ZL_ED_WAVE), b = __shfl_xor(mx, d, ZL_ED_WAVE);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    if ((tid & (ZL_ED_WAVE - 1)) == 0) { sMin[tid / ZL_ED_WAVE] = mn; sMax[tid / ZL_ED_WAVE] = mx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < ZL_ED_WAVES; ++w) { mn = sMin[w] < mn ? sMin[w] : mn; mx = sMax[w] > mx ? sMax[w] : mx; }
        if (mx >= 0) {
            atomicMin(&found[S.found].first, mn);
            atomicMax(&found[S.found].last, mx);
        }
    }
}

__global__ void __launch_bounds__(ZL_ED_WG) zl_k_edit_render(const ZlEdJob *__restrict__ jobs, int32_t njobs, const float *__restrict__ weights, uint32_t *__restrict__ verdicts)
{
    const int32_t wg = (int32_t)blockIdx.x;
    const ZlEdJob J = jobs[zl_ed_find(jobs, njobs, wg)];
    const int32_t tid = (int32_t)threadIdx.x;
    const int64_t g = (int64_t)(wg - J.wg_base) * ZL_ED_WG + tid;
    const bool live = g < zl_ed_groups(J);
    bool bad = false;
    if (live) {
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const ZlEdGlobalF src = (ZlEdGlobalF)J.src;
        const int64_t k0 = 4 * g, data = zl_ed_data_floats(J);
        if (zl_ed_group_full(J, g)) {
            const zl_ed_f4 v = *(ZlEdGlobalF4u)(src + zl_ed_group_first(J, g));
            const bool stereo = J.channels == 2;
            // (zl_ed_lane, as selects on the job's two uniform flags)
            y[0] = !J.reverse ? v.x : (stereo ? v.z : v.w);
            y[1] = !J.reverse ? v.y : (stereo ? v.w : v.z);
            y[2] = !J.reverse ? v.z : (stereo ? v.x : v.y);
            y[3] = !J.reverse ? v.w : (stereo ? v.y : v.x);
        } else if (zl_ed_group_loads(J, g)) {                     // the group the data's end cuts: one per job at most
#pragma unroll
            for (int j = 0; j < 4; ++j) if (k0 + j < data) y[j] = src[zl_ed_src_index(J, k0 + j)];
        }
        if (zl_ed_group_fades(J, g)) {
            const int32_t per = 4 / J.channels;                    // frames of a group
            const int32_t i0 = (int32_t)(k0 / J.channels);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const int32_t i = i0 + f;
                if (f < per && i < J.n) {
                    const int32_t w = zl_ed_weight_index(J, i);
                    if (w >= 0) {
                        const float wt = weights[w];               // one 4-byte load per faded frame
                        if (J.channels == 2) {
                            y[2 * (f & 1)] = wt * y[2 * (f & 1)]; y[2 * (f & 1) + 1] = wt * y[2 * (f & 1) + 1];
                            bad = bad || !zl_ed_finite(y[2 * (f & 1)]) || !zl_ed_finite(y[2 * (f & 1) + 1]);
                        } else {
                            y[f] = wt * y[f];
                            bad = bad || !zl_ed_finite(y[f]);
                        }
                    }
                }
            }
        }
        zl_ed_f4 o; o.x = y[0]; o.y = y[1]; o.z = y[2]; o.w = y[3];
        ((ZlEdGlobalOutF4)J.dst)[g] = o;
    }
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (any && (tid & (ZL_ED_WAVE - 1)) == 0) atomicOr(verdicts + J.verdict, 1u);
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_edit_scan(const ZlEdScan *reqs, int32_t nscan, int32_t wgs, ZlEdFound *found, hipStream_t s)
{
    if (nscan <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_edit_scan, dim3((unsigned)wgs), dim3(ZL_ED_WG), 0, s, reqs, nscan, found);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_edit_render(const ZlEdJob *jobs, int32_t njobs, int32_t wgs, const float *weights, uint32_t *verdicts, hipStream_t s)
{
    if (njobs <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_edit_render, dim3((unsigned)wgs), dim3(ZL_ED_WG), 0, s, jobs, njobs, weights, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}
