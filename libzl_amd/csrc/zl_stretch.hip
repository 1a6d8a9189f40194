// zl_stretch.hip -- HIP kernels of the clip re-render (zlhip_sound_rerender / _batch; the definition is in zl_stretch.h).
//
//   zl_k_stretch_seek    one workgroup per clip whose stretch stage runs: walks its segments in order (each offset depends on the
//                        previous one through the cross-fade source), staging the quantised seek window and the weighted reference
//                        in LDS, W candidates spread over the lanes, exact int64 correlation sums, argmax over the workgroup
//   zl_k_stretch_synth   one lane per output frame of every clip of the call: stretch + resample + gain fused, written straight into
//                        the clip's new arena extent (interleaved, ZL_ST_PAD zero frames behind it)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -- the seek's double division and square root must be the
// correctly rounded sequences, and the synthesis' float arithmetic must round after every operation, as the host build does.
#include <hip/hip_runtime.h>
#include <climits>
#include "zl_stretch.h"

#define ZL_ST_SEEK_THREADS 512
#define ZL_ST_SYNTH_THREADS 256

namespace {

struct ZlStIn {
    const float *src; int64_t len; int ch;
    __device__ float operator()(int64_t n, int c) const { return n < len ? src[n * ch + c] : 0.0f; }
};

__device__ inline void zl_st_pick(double &bs, int32_t &bo, double s, int32_t o)
{
    if (zl_st_better(s, o, bs, bo)) { bs = s; bo = o; }
}

}  // namespace

__global__ void __launch_bounds__(ZL_ST_SEEK_THREADS) zl_k_stretch_seek(const ZlStretchJob *jobs, const int32_t *seek_jobs, int32_t *offsets)
{
    __shared__ int32_t sIn[2][ZL_ST_MAX_WINDOW];      // q(in[base_k + j]), j < W + O, per channel
    __shared__ int32_t sRef[2][ZL_ST_OVERLAP_MAX];    // the weighted reference of the segment's mid
    __shared__ double  sBest[ZL_ST_SEEK_THREADS / 64];
    __shared__ int32_t sBestO[ZL_ST_SEEK_THREADS / 64];
    __shared__ int64_t sPrev;                         // b_{k-1}

    const ZlStretchJob &J = jobs[seek_jobs[blockIdx.x]];
    const ZlStretchGeom g = J.geom;
    const int ch = J.channels, O = g.O, W = g.W, L = g.S - g.O;
    const ZlStIn in{reinterpret_cast<const float *>(J.src), g.len, ch};
    int32_t *off = offsets + J.off_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { off[0] = 0; sPrev = 0; }
    __syncthreads();

    for (int32_t k = 1; k < g.nseg; ++k) {
        const int64_t base = zl_st_base(g, k), prev = sPrev;
        for (int i = tid; i < O; i += ZL_ST_SEEK_THREADS)
            for (int c = 0; c < ch; ++c) sRef[c][i] = zl_st_ref(zl_st_q(in(prev + L + i, c)), i, O);
        for (int j = tid; j < W + O; j += ZL_ST_SEEK_THREADS)
            for (int c = 0; c < ch; ++c) sIn[c][j] = zl_st_q(in(base + j, c));
        __syncthreads();

        double bs = -INFINITY; int32_t bo = INT_MAX;
        for (int o = tid; o < W; o += ZL_ST_SEEK_THREADS) {
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
            zl_st_pick(bs, bo, zl_st_score(corr, norm), o);
        }
        // argmax over the wave, then over the workgroup (the order of the comparisons does not matter: zl_st_better is a total order)
        for (int d = 32; d >= 1; d >>= 1) {
            const double s2 = __shfl_xor(bs, d, 64);
            const int32_t o2 = __shfl_xor(bo, d, 64);
            zl_st_pick(bs, bo, s2, o2);
        }
        if (lane == 0) { sBest[wave] = bs; sBestO[wave] = bo; }
        __syncthreads();
        if (tid == 0) {
            double s = sBest[0]; int32_t o = sBestO[0];
            for (int w = 1; w < ZL_ST_SEEK_THREADS / 64; ++w) zl_st_pick(s, o, sBest[w], sBestO[w]);
            off[k] = o;
            sPrev = base + o;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(ZL_ST_SYNTH_THREADS) zl_k_stretch_synth(const ZlStretchJob *jobs, const int32_t *offsets)
{
    const ZlStretchJob &J = jobs[blockIdx.y];
    const ZlStretchGeom g = J.geom;
    const int64_t j = (int64_t)blockIdx.x * ZL_ST_SYNTH_THREADS + threadIdx.x;
    if (j >= g.N + ZL_ST_PAD) return;
    const int ch = J.channels;
    const ZlStIn in{reinterpret_cast<const float *>(J.src), g.len, ch};
    const int32_t *off = offsets + J.off_base;
    float *dst = reinterpret_cast<float *>(J.dst) + j * ch;
    for (int c = 0; c < ch; ++c) dst[c] = j < g.N ? zl_st_y(g, off, j, c, in) : 0.0f;
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_stretch_seek(const ZlStretchJob *jobs, const int32_t *seek_jobs, int nseek, int32_t *offsets, hipStream_t s)
{
    if (nseek <= 0) return 0;
    hipLaunchKernelGGL(zl_k_stretch_seek, dim3(nseek), dim3(ZL_ST_SEEK_THREADS), 0, s, jobs, seek_jobs, offsets);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_stretch_synth(const ZlStretchJob *jobs, int njobs, int64_t max_frames, const int32_t *offsets, hipStream_t s)
{
    if (njobs <= 0) return 0;
    const int64_t gx = (max_frames + ZL_ST_PAD + ZL_ST_SYNTH_THREADS - 1) / ZL_ST_SYNTH_THREADS;
    hipLaunchKernelGGL(zl_k_stretch_synth, dim3((unsigned)gx, (unsigned)njobs), dim3(ZL_ST_SYNTH_THREADS), 0, s, jobs, offsets);
    ZL_LAUNCH_CHECK();
    return 0;
}
