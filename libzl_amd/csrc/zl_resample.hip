// zl_resample.hip -- HIP kernels of the sample-rate conversion (zlhip_sound_convert_rate / _batch; the definition is in zl_resample.h).
//
//   zl_k_resample          one launch per call.  A workgroup is ZL_RS_WG consecutive output frames of one job (clip), one per lane; it
//                          finds its job by bisection over the jobs' wg_base with scalar loads.  The workgroup stages the input frames
//                          its lanes read (zl_rs_span) in LDS, masked by frame index: a frame outside [0, len) is a produced +0.  Every
//                          lane reads its phase's row of the filter table from global memory (16-byte loads; the table stays in L2)
//                          and per tap one frame from LDS: a stereo pair is multiplied and added as a pair, each half the IEEE single
//                          operation, never fused.  Stores: one frame per lane (8 bytes stereo, 4 mono).  The job's last workgroup
//                          also writes the zero frames behind the clip.  A clip's verdict on non-finite output: a ballot, one atomic
//                          OR by one lane, only when something is set.
//   zl_k_resample_publish  one lane per clip of the call: the sound-table entry, ZL_SOUND_FINITE from the clip's verdict word.
//
// No scratch memory.  LDS: ZL_RS_STAGE_FRAMES stereo frames (20 KB).
#include <hip/hip_runtime.h>
#include "zl_resample.h"

namespace {

typedef float zl_rs_f2 __attribute__((ext_vector_type(2)));
typedef float zl_rs_f4 __attribute__((ext_vector_type(4)));
// the extents' and the table's addresses arrive as integers in the job record: tell the compiler that they are global memory
typedef const float __attribute__((address_space(1))) *ZlRsGlobalF;
typedef const zl_rs_f2 __attribute__((address_space(1))) *ZlRsGlobalF2;
typedef const zl_rs_f4 __attribute__((address_space(1))) *ZlRsGlobalF4;
typedef float __attribute__((address_space(1))) *ZlRsGlobalOutF;
typedef zl_rs_f2 __attribute__((address_space(1))) *ZlRsGlobalOutF2;

// the taps of one output frame: `row` is the lane's table row, x(k) the staged frame k behind the lane's first tap
template <class V, class X> __device__ __forceinline__ V zl_rs_frame(ZlRsGlobalF row, int32_t taps, const X &x)
{
    V acc = (V)(0.0f);
    int32_t t = 0;
    for (; t + 4 <= taps; t += 4) {                                // (taps is the same in every lane of the workgroup)
        const zl_rs_f4 h = *(ZlRsGlobalF4)(row + t);
        const V m0 = x(t) * h.x;     acc = acc + m0;
        const V m1 = x(t + 1) * h.y; acc = acc + m1;
        const V m2 = x(t + 2) * h.z; acc = acc + m2;
        const V m3 = x(t + 3) * h.w; acc = acc + m3;
    }
    if (t < taps) {                                                // taps is even: two are left
        const zl_rs_f2 h = *(ZlRsGlobalF2)(row + t);
        const V m0 = x(t) * h.x;     acc = acc + m0;
        const V m1 = x(t + 1) * h.y; acc = acc + m1;
    }
    return acc;
}

}  // namespace

__global__ void __launch_bounds__(ZL_RS_WG) zl_k_resample(const ZlRsJob *__restrict__ jobs, int32_t njobs, uint32_t *__restrict__ verdicts)
{
    __shared__ zl_rs_f2 stage[ZL_RS_STAGE_FRAMES];
    const int32_t wg = (int32_t)blockIdx.x;
    // the job of the workgroup: the last one whose wg_base is <= wg (wg_base is increasing, jobs[0].wg_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = njobs - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (jobs[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
    const ZlRsJob J = jobs[r];
    const int32_t w = wg - J.wg_base;
    const int32_t tid = (int32_t)threadIdx.x;

    int64_t first; int32_t count;
    zl_rs_span(J, w, &first, &count);
    if (count > ZL_RS_STAGE_FRAMES) count = ZL_RS_STAGE_FRAMES;    // (never: the host's limits; the LDS image is not left in any case)
    if (J.channels == 2) {
        const ZlRsGlobalF2 src = (ZlRsGlobalF2)J.src;
        for (int32_t k = tid; k < count; k += ZL_RS_WG) {
            const int64_t f = first + k;
            zl_rs_f2 v = (zl_rs_f2)(0.0f);
            if (zl_rs_in_clip(J, f)) v = src[f];
            stage[k] = v;
        }
    } else {
        float *const st = reinterpret_cast<float *>(stage);
        const ZlRsGlobalF src = (ZlRsGlobalF)J.src;
        for (int32_t k = tid; k < count; k += ZL_RS_WG) {
            const int64_t f = first + k;
            float v = 0.0f;
            if (zl_rs_in_clip(J, f)) v = src[f];
            st[k] = v;
        }
    }
    __syncthreads();

    const int64_t j = (int64_t)w * ZL_RS_WG + tid;
    const bool live = j < (int64_t)J.N;
    int64_t i; int32_t p;
    zl_rs_position(J, live ? j : (int64_t)J.N - 1, &i, &p);        // (a lane behind the clip walks the last frame's taps and stores nothing)
    const int32_t o = (int32_t)(i - J.half + 1 - first);           // the lane's first tap in the stage: 0 <= o, o + taps <= count
    const ZlRsGlobalF row = (ZlRsGlobalF)J.table + (size_t)p * (size_t)J.row;
    bool bad = false;
    if (J.channels == 2) {
        const zl_rs_f2 *const x0 = stage + o;
        const zl_rs_f2 y = zl_rs_frame<zl_rs_f2>(row, J.taps, [x0](int32_t t) { return x0[t]; });
        if (live) {
            ((ZlRsGlobalOutF2)J.dst)[j] = y;
            bad = !(zl_rs_finite(y.x) && zl_rs_finite(y.y));
        }
    } else {
        const float *const x0 = reinterpret_cast<const float *>(stage) + o;
        const float y = zl_rs_frame<float>(row, J.taps, [x0](int32_t t) { return x0[t]; });
        if (live) {
            ((ZlRsGlobalOutF)J.dst)[j] = y;
            bad = !zl_rs_finite(y);
        }
    }
    // the zero frames behind the clip and the floats up to the 16-byte boundary: the job's last workgroup, one float per lane
    if (w == zl_rs_job_wgs(J.N) - 1 && tid < zl_rs_tail_floats(J))
        ((ZlRsGlobalOutF)J.dst)[(int64_t)J.N * J.channels + tid] = 0.0f;
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (any && (tid & 63) == 0) atomicOr(verdicts + J.verdict, 1u);
}

__global__ void __launch_bounds__(ZL_RS_WG) zl_k_resample_publish(const ZlRsPublish *__restrict__ recs, int32_t n, const uint32_t *__restrict__ verdicts, ZlSound *table)
{
    const int32_t i = (int32_t)(blockIdx.x * ZL_RS_WG + threadIdx.x);
    if (i >= n) return;
    ZlRsPublish p = recs[i];
    if (verdicts[p.verdict] == 0u) p.s.flags |= ZL_SOUND_FINITE;
    table[p.id] = p.s;
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_resample(const ZlRsJob *jobs, int32_t njobs, int32_t wgs, uint32_t *verdicts, hipStream_t s)
{
    if (njobs <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_resample, dim3((unsigned)wgs), dim3(ZL_RS_WG), 0, s, jobs, njobs, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_resample_publish(const ZlRsPublish *recs, int32_t n, const uint32_t *verdicts, ZlSound *table, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(zl_k_resample_publish, dim3((unsigned)((n + ZL_RS_WG - 1) / ZL_RS_WG)), dim3(ZL_RS_WG), 0, s, recs, n, verdicts, table);
    ZL_LAUNCH_CHECK();
    return 0;
}
