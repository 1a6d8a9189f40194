// zl_warp.hip -- HIP kernels of the warp (zlhip_sound_warp / _batch; the definition is in zl_warp.h).
//
//   zl_k_warp_seek    one workgroup per stretched region of the whole call that has more than one segment: it walks the region's segments
//                     1 .. nseg - 1 in order, as zl_k_stretch_seek walks a clip's (zl_stretch.hip): the quantised seek window and the
//                     weighted reference staged in LDS, W candidates spread over the lanes, int32 pair sums into int64, the argmax by
//                     shuffles over the wave and LDS over the workgroup.  A region's first segment starts at its anchor: off[0] = 0.
//   zl_k_warp_synth   one lane per frame of the new extent of every clip of the call, the zero frames and the floats up to the 16-byte
//                     boundary included: nothing is copied, there is no intermediate buffer.  A workgroup is ZL_WP_SYNTH_THREADS
//                     consecutive frames of one clip and finds its clip by bisection over the jobs' wg_base and its first region by
//                     bisection over the clip's region records, both on uniform values (scalar loads); its lanes step forward from
//                     there.  The verdict on a non-finite sample: a ballot per wave, one atomic OR by its first lane, only when set.
//   (the sound-table entries switch by zl_k_resample_publish, zl_resample.hip)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math, as zl_stretch.hip.  No scratch memory.  LDS: the seek kernel
// section 8's (two channels of ZL_ST_MAX_WINDOW and of ZL_ST_OVERLAP_MAX int32, the reduction's words), the synthesis kernel none.
#include <hip/hip_runtime.h>
#include <climits>
#include "zl_warp.h"

namespace {

struct ZlWpIn {
    const float *src; int64_t len; int ch;
    __device__ float operator()(int64_t n, int c) const { return n < len ? src[n * ch + c] : 0.0f; }
};

__device__ inline void zl_wp_pick(double &bs, int32_t &bo, double s, int32_t o)
{
    if (zl_st_better(s, o, bs, bo)) { bs = s; bo = o; }
}

}  // namespace

__global__ void __launch_bounds__(ZL_WP_SEEK_THREADS) zl_k_warp_seek(const ZlWpJob *__restrict__ jobs, const ZlWpRegion *__restrict__ regions,
                                                                       const int32_t *__restrict__ seek_regions, int32_t *__restrict__ offsets)
{
    __shared__ int32_t sIn[2][ZL_ST_MAX_WINDOW];      // q(in[base_k + j]), j < W + O, per channel
    __shared__ int32_t sRef[2][ZL_ST_OVERLAP_MAX];    // the weighted reference of the segment's mid
    __shared__ double  sBest[ZL_WP_SEEK_THREADS / 64];
    __shared__ int32_t sBestO[ZL_WP_SEEK_THREADS / 64];
    __shared__ int64_t sPrev;                         // b_{k-1}

    const ZlWpRegion R = regions[seek_regions[blockIdx.x]];
    const ZlWpJob &J = jobs[R.job];
    const int ch = J.channels, O = J.O, W = R.W, L = R.L;
    const ZlWpIn in{reinterpret_cast<const float *>(J.src), J.len, ch};
    int32_t *off = offsets + R.off_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { off[0] = 0; sPrev = R.a; }
    __syncthreads();

    for (int32_t k = 1; k < R.nseg; ++k) {
        const int64_t base = zl_wp_nominal(R, k), prev = sPrev;
        for (int i = tid; i < O; i += ZL_WP_SEEK_THREADS)
            for (int c = 0; c < ch; ++c) sRef[c][i] = zl_st_ref(zl_st_q(in(prev + L + i, c)), i, O);
        for (int j = tid; j < W + O; j += ZL_WP_SEEK_THREADS)
            for (int c = 0; c < ch; ++c) sIn[c][j] = zl_st_q(in(base + j, c));
        __syncthreads();

        double bs = -INFINITY; int32_t bo = INT_MAX;
        for (int o = tid; o < W; o += ZL_WP_SEEK_THREADS) {
            int64_t corr = 0, norm = 0;
            for (int c = 0; c < ch; ++c) {
                const int32_t *x = &sIn[c][o], *r = sRef[c];
                // pairs of products fit int32 (|ref|, |q| <= 32767); O is a multiple of 8
                for (int i = 0; i < O; i += 2) {
                    const int32_t x0 = x[i], x1 = x[i + 1];
                    corr += (int64_t)(r[i] * x0 + r[i + 1] * x1);
                    norm += (int64_t)(x0 * x0 + x1 * x1);
                }
            }
            zl_wp_pick(bs, bo, zl_st_score(corr, norm), o);
        }
        // argmax over the wave, then over the workgroup (zl_st_better is a total order: the order of the comparisons does not matter)
        for (int d = 32; d >= 1; d >>= 1) {
            const double s2 = __shfl_xor(bs, d, 64);
            const int32_t o2 = __shfl_xor(bo, d, 64);
            zl_wp_pick(bs, bo, s2, o2);
        }
        if (lane == 0) { sBest[wave] = bs; sBestO[wave] = bo; }
        __syncthreads();
        if (tid == 0) {
            double s = sBest[0]; int32_t o = sBestO[0];
            for (int w = 1; w < ZL_WP_SEEK_THREADS / 64; ++w) zl_wp_pick(s, o, sBest[w], sBestO[w]);
            off[k] = o;
            sPrev = base + o;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(ZL_WP_SYNTH_THREADS) zl_k_warp_synth(const ZlWpJob *__restrict__ jobs, int32_t njobs, const ZlWpRegion *__restrict__ regions,
                                                                         const int32_t *__restrict__ offsets, uint32_t *__restrict__ verdicts)
{
    const int32_t wg = (int32_t)blockIdx.x;
    // the job of the workgroup: the last one whose wg_base is <= wg (wg_base is increasing, jobs[0].wg_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = njobs - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (jobs[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
    const ZlWpJob J = jobs[r];
    const ZlWpRegion *regs = regions + J.region_base;
    const int32_t tid = (int32_t)threadIdx.x;
    const int64_t n0 = (int64_t)(wg - J.wg_base) * ZL_WP_SYNTH_THREADS, n = n0 + tid;
    const int ch = J.channels;
    bool bad = false;
    if (n < zl_wp_lanes(J)) {
        float y0 = 0.0f, y1 = 0.0f;                              // (y1 stays +0 for a mono clip)
        if (n < J.N) {
            // the workgroup's first region (uniform), then forward to the lane's own
            int32_t i = zl_wp_find_region(regs, J.nregions, (int32_t)(n0 < J.N ? n0 : 0));
            while (i + 1 < J.nregions && regs[i + 1].d <= (int32_t)n) ++i;
            const ZlWpTap t = zl_wp_tap(regs, i, offsets, J.O, (int32_t)n);
            if (ch == 2) {                                         // a stereo frame is one 8-byte load (the extents are 16-byte aligned)
                const float2 *src = reinterpret_cast<const float2 *>(J.src);
                float2 v = make_float2(0.0f, 0.0f), p = make_float2(0.0f, 0.0f);
                if (t.v < J.len) v = src[t.v];
                if (t.fade && t.p < J.len) p = src[t.p];
                y0 = zl_wp_join(t, J.O, p.x, v.x); y1 = zl_wp_join(t, J.O, p.y, v.y);
            } else {
                const ZlWpIn in{reinterpret_cast<const float *>(J.src), J.len, ch};
                y0 = zl_wp_sample(t, J.O, 0, in);
            }
            bad = !zl_wp_finite(y0) || !zl_wp_finite(y1);
        }
        float *dst = reinterpret_cast<float *>(J.dst) + n * ch;
        if (ch == 2) *reinterpret_cast<float2 *>(dst) = make_float2(y0, y1); else dst[0] = y0;
    }
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (any && (tid & 63) == 0) atomicOr(verdicts + J.verdict, 1u);
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_warp_seek(const ZlWpJob *jobs, const ZlWpRegion *regions, const int32_t *seek_regions, int32_t nseek, int32_t *offsets, hipStream_t s)
{
    if (nseek <= 0) return 0;
    hipLaunchKernelGGL(zl_k_warp_seek, dim3((unsigned)nseek), dim3(ZL_WP_SEEK_THREADS), 0, s, jobs, regions, seek_regions, offsets);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_warp_synth(const ZlWpJob *jobs, int32_t njobs, int32_t wgs, const ZlWpRegion *regions, const int32_t *offsets, uint32_t *verdicts, hipStream_t s)
{
    if (njobs <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_warp_synth, dim3((unsigned)wgs), dim3(ZL_WP_SYNTH_THREADS), 0, s, jobs, njobs, regions, offsets, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}
