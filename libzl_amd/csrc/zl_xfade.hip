// zl_xfade.hip -- HIP kernels of the loop crossfade (zlhip_sound_loop_crossfade / _batch; the definition is in zl_xfade.h).
//
//   zl_k_xfade_measure  one workgroup of ZL_XF_WG lanes per job.  It walks the fade in chunks of ZL_XF_CHUNK frames: the chunk's span of
//                       A and its span of B are read in 16-byte groups of the arena's own layout, head and tail masked by float index
//                       (no float outside the two regions is looked at), mixed and quantised (zl_pt_group_mix) and left in LDS by the
//                       frame's number in the chunk -- the two regions sit (e - s) channels floats apart and are in general not aligned
//                       to each other, so the products pair up there.  A lane sums m_a m_b, m_a^2 and m_b^2 of its frames in int64;
//                       shuffles over the wave, LDS over the workgroup; one lane writes {sab, saa, sbb} into host memory mapped into
//                       the device.
//   zl_k_xfade_render   the hot path, a fused copy-and-fade: one lane per 16-byte group of the destination extent, a workgroup is
//                       ZL_XF_WG consecutive groups of one job and finds its job by bisection over the jobs' wg_base with scalar loads.
//                       A group outside A is one 16-byte load and one 16-byte store.  A group that overlaps A (about 1 % of them)
//                       reads, per float of A, the float (e - s) channels lower and the (a, b) pair of its frame (one 8-byte load) and
//                       computes the definition's three operations.  The floats behind the data's end -- the zero frames and the pad --
//                       are produced, not copied.  A clip's verdict on a non-finite fade sample: a ballot per wave, one atomic OR by
//                       its first lane, only when something is set.
//   (the sound-table entries switch by zl_k_resample_publish, zl_resample.hip)
//
// No scratch memory.  LDS: the render kernel none; the measuring kernel two chunks of int32 and twelve words for the reduction.
#include <hip/hip_runtime.h>
#include "zl_xfade.h"

#define ZL_XF_WAVE 64
#define ZL_XF_WAVES (ZL_XF_WG / ZL_XF_WAVE)

namespace {

typedef float zl_xf_f2 __attribute__((ext_vector_type(2)));
typedef float zl_xf_f4 __attribute__((ext_vector_type(4)));
// the extents' addresses arrive as integers in the job record: tell the compiler that they are global memory
typedef const float __attribute__((address_space(1))) *ZlXfGlobalF;
typedef const zl_xf_f2 __attribute__((address_space(1))) *ZlXfGlobalF2;
typedef const zl_xf_f4 __attribute__((address_space(1))) *ZlXfGlobalF4;
typedef zl_xf_f4 __attribute__((address_space(1))) *ZlXfGlobalOutF4;

__device__ __forceinline__ int64_t zl_xf_wave_sum(int64_t v)
{
#pragma unroll
    for (int d = 1; d < ZL_XF_WAVE; d <<= 1) v += (int64_t)__shfl_xor((long long)v, d, ZL_XF_WAVE);
    return v;
}

// frames [lo, hi) of the clip (hi - lo <= ZL_XF_CHUNK) mixed into out[0 .. hi - lo)
__device__ __forceinline__ void zl_xf_mix_span(const ZlXfJob &J, int32_t lo, int32_t hi, int32_t *out, int tid)
{
    int64_t f0, f1, g0, g1;
    zl_ov_groups(lo, hi, J.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const ZlXfGlobalF4 src = (ZlXfGlobalF4)J.src + g0;
    for (int32_t g = tid; g < ngroups; g += ZL_XF_WG) {
        const zl_xf_f4 v = src[g];
        int32_t m[4], idx[4];
        zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, J.channels, m, idx);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (idx[j] >= 0 && idx[j] < hi - lo) out[idx[j]] = m[j];
    }
}

}  // namespace

__global__ void __launch_bounds__(ZL_XF_WG) zl_k_xfade_measure(const ZlXfJob *__restrict__ jobs, ZlXfSums *__restrict__ sums)
{
    __shared__ int32_t sA[ZL_XF_CHUNK];
    __shared__ int32_t sB[ZL_XF_CHUNK];
    __shared__ int64_t sRed[3][ZL_XF_WAVES];
    const ZlXfJob J = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    int64_t ab = 0, aa = 0, bb = 0;
    const int32_t chunks = zl_xf_chunks(J.X);
    for (int32_t c = 0; c < chunks; ++c) {                          // (uniform)
        int32_t i0, i1;
        zl_xf_chunk(J.X, c, &i0, &i1);
        zl_xf_mix_span(J, J.e - J.X + i0, J.e - J.X + i1, sA, tid);
        zl_xf_mix_span(J, J.s - J.X + i0, J.s - J.X + i1, sB, tid);
        __syncthreads();
        for (int32_t i = tid; i < i1 - i0; i += ZL_XF_WG) {
            const int64_t a = sA[i], b = sB[i];
            ab += a * b; aa += a * a; bb += b * b;
        }
        __syncthreads();                                           // (the chunk's last readers are done)
    }
    ab = zl_xf_wave_sum(ab); aa = zl_xf_wave_sum(aa); bb = zl_xf_wave_sum(bb);
    if ((tid & (ZL_XF_WAVE - 1)) == 0) { sRed[0][tid / ZL_XF_WAVE] = ab; sRed[1][tid / ZL_XF_WAVE] = aa; sRed[2][tid / ZL_XF_WAVE] = bb; }
    __syncthreads();
    if (tid == 0) {
        ZlXfSums o; o.sab = 0; o.saa = 0; o.sbb = 0;
#pragma unroll
        for (int w = 0; w < ZL_XF_WAVES; ++w) { o.sab += sRed[0][w]; o.saa += sRed[1][w]; o.sbb += sRed[2][w]; }
        sums[blockIdx.x] = o;
    }
}

__global__ void __launch_bounds__(ZL_XF_WG) zl_k_xfade_render(const ZlXfJob *__restrict__ jobs, int32_t njobs, const float *__restrict__ weights, uint32_t *__restrict__ verdicts)
{
    const int32_t wg = (int32_t)blockIdx.x;
    // the job of the workgroup: the last one whose wg_base is <= wg (wg_base is increasing, jobs[0].wg_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = njobs - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (jobs[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
    const ZlXfJob J = jobs[r];
    const int32_t tid = (int32_t)threadIdx.x;
    const int64_t g = (int64_t)(wg - J.wg_base) * ZL_XF_WG + tid;
    const bool live = g < zl_xf_groups(J);
    bool bad = false;
    if (live) {
        zl_xf_f4 v = (zl_xf_f4)(0.0f);
        if (zl_xf_group_loads(J, g)) v = ((ZlXfGlobalF4)J.src)[g];
        float y[4] = {v.x, v.y, v.z, v.w};
        const int64_t k0 = 4 * g, data = zl_xf_data_floats(J);
        if (k0 + 4 > data) {                                       // the group reaches behind the data: those floats are produced zeros
#pragma unroll
            for (int j = 0; j < 4; ++j) if (k0 + j >= data) y[j] = 0.0f;
        }
        if (zl_xf_group_fades(J, g)) {
            const ZlXfGlobalF src = (ZlXfGlobalF)J.src;
            const ZlXfGlobalF2 ab = (ZlXfGlobalF2)weights + J.weights;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = k0 + j;
                if (zl_xf_fades(J, k)) {
                    const zl_xf_f2 w = ab[zl_xf_weight_index(J, k)];
                    const float xb = src[zl_xf_b_index(J, k)];
                    y[j] = zl_xf_mix(w.x, w.y, y[j], xb);
                    bad = bad || !zl_xf_finite(y[j]);
                }
            }
        }
        zl_xf_f4 o; o.x = y[0]; o.y = y[1]; o.z = y[2]; o.w = y[3];
        ((ZlXfGlobalOutF4)J.dst)[g] = o;
    }
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (any && (tid & (ZL_XF_WAVE - 1)) == 0) atomicOr(verdicts + J.verdict, 1u);
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_xfade_measure(const ZlXfJob *jobs, int32_t njobs, ZlXfSums *sums, hipStream_t s)
{
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_xfade_measure, dim3((unsigned)njobs), dim3(ZL_XF_WG), 0, s, jobs, sums);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_xfade_render(const ZlXfJob *jobs, int32_t njobs, int32_t wgs, const float *weights, uint32_t *verdicts, hipStream_t s)
{
    if (njobs <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_xfade_render, dim3((unsigned)wgs), dim3(ZL_XF_WG), 0, s, jobs, njobs, weights, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}
