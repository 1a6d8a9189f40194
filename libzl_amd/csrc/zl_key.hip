// zl_key.hip -- HIP kernels of the key detection (zlhip_sound_key / _batch; the definition is in zl_key.h).
//
//   zl_k_key_gate       one workgroup per analysis frame: it reads the frame's L samples in 16-byte groups of the arena's own layout,
//                       head and tail masked by float index, mixes and quantises them and reduces the span's energy as integers; one
//                       lane stores the energy and the verdict "silent".
//   zl_k_key_correlate  the hot path.  A workgroup takes one work item (request, frame, group of 8 bins) and finds its request by
//                       bisection over the records' item_base; a silent frame's item stores zeros and leaves.  The table sits in LDS
//                       as 4096 words (cos | sin << 16, 16 KB, paired by the host and copied in with four 16-byte loads a lane): one gather gives both factors of a phase, and the window is the low
//                       half of a second gather.  The frame's mixed samples are shared by all bins of the group, so they are staged
//                       in chunks of 2048 int32 (8 KB) of the group's widest window -- a 32768-sample span next to the table would
//                       leave one workgroup per CU.  A bin belongs to 32 lanes, half a wavefront, which stride j: the 32 staged
//                       samples of one step are consecutive words, conflict-free in ds_read_b32's 32-lane groups; the window gather
//                       of 32 neighbouring j falls into a few words (4096 / N entries per sample: a broadcast), so the phase gather
//                       is the one that pays bank conflicts -- for a low bin 32 lanes cover 32 step / 2^20 entries (179 at 65 Hz and
//                       48 kHz), for a high one they scatter.  Phases and window indices are j step and j wstep modulo 2^32: the lane
//                       multiplies once per chunk and then adds 32 step, which is the same number (no rounding is carried), so the
//                       loop multiplies three times per term: m w as a 32-bit product (quarter rate; the compiler does not take the 24-bit
//                       form for it, and forcing it by hand measured under 2.5 % and stopped the unrolling), v c and v s as 24-bit multiplies
//                       that pick their half of the pair by operand select.  Four steps are unrolled so that twelve LDS reads are in
//                       flight per lane;
//                       a term can reach 2^31 - 131070, so each is widened and added as 64 bits (zl_key.h: no chunk fits 32 bits).
//                       The 32 lanes of a bin combine by shuffles inside their half-wave; every (frame, bin) has one writer.
//   zl_k_key_fold       one workgroup per request: a lane per bin sums the energies that pass the bin gate over the sounding frames (the
//                       per-bin totals), twelve lanes fold them into the chroma, one lane writes the integer record into host memory
//                       mapped into the device.
//
// A call is these three launches, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_key.h"

#define ZL_KY_THREADS 256
#define ZL_KY_WAVE 64
#define ZL_KY_WAVES_PER_BLOCK (ZL_KY_THREADS / ZL_KY_WAVE)

static_assert(ZL_KY_THREADS == ZL_KY_ITEM_BINS * ZL_KY_BIN_LANES, "a lane group per bin of the item");
static_assert(ZL_KY_BIN_LANES * 2 == ZL_KY_WAVE, "a bin's lanes are half a wavefront: the shuffles stay inside it");
static_assert(ZL_KY_MAX_BINS <= ZL_KY_THREADS, "a lane per bin in the fold");
static_assert(ZL_KY_TABLE % (4 * ZL_KY_THREADS) == 0, "the table is staged in whole rounds of 16-byte loads");

namespace {

template <typename T> using ZlKyGlobal = const T __attribute__((address_space(1))) *;
typedef float zl_ky_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t zl_ky_u32x4 __attribute__((ext_vector_type(4)));

// the sum over the workgroup, in every thread.  sRed: ZL_KY_WAVES_PER_BLOCK words of LDS
__device__ __forceinline__ uint64_t zl_ky_block_sum(uint64_t v, uint64_t *sRed)
{
#pragma unroll
    for (int d = 1; d < ZL_KY_WAVE; d <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, ZL_KY_WAVE);
    __syncthreads();
    if ((threadIdx.x & (ZL_KY_WAVE - 1)) == 0) sRed[threadIdx.x / ZL_KY_WAVE] = v;
    __syncthreads();
    uint64_t r = sRed[0];
#pragma unroll
    for (int w = 1; w < ZL_KY_WAVES_PER_BLOCK; ++w) r += sRed[w];
    return r;
}

// the request of item / frame `at`: the last one whose base is <= at (the bases do not decrease; a request without frames shares its
// base with the next one, which is then the one found)
template <bool kItems> __device__ __forceinline__ int32_t zl_ky_find(const ZlKyRequest *__restrict__ reqs, int32_t nreq, int32_t at)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((kItems ? reqs[mid].item_base : reqs[mid].frame_base) <= at) lo = mid; else hi = mid - 1;
    }
}

}  // namespace

__global__ void __launch_bounds__(ZL_KY_THREADS) zl_k_key_gate(const ZlKyRequest *__restrict__ reqs, int32_t nreq, ZlKyStat *__restrict__ stat)
{
    __shared__ uint64_t sRed[ZL_KY_WAVES_PER_BLOCK];
    const int32_t f = (int32_t)blockIdx.x;
    const ZlKyRequest R = reqs[zl_ky_find<false>(reqs, nreq, f)];
    const int tid = threadIdx.x;
    const int64_t s0 = zl_ky_frame_start(R, f - R.frame_base);
    int64_t f0, f1, g0, g1;
    zl_ov_groups(s0, s0 + R.span, R.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const ZlKyGlobal<zl_ky_f32x4> src = (ZlKyGlobal<zl_ky_f32x4>)R.src + g0;
    uint64_t energy = 0;
    for (int32_t g = tid; g < ngroups; g += ZL_KY_THREADS) {
        const zl_ky_f32x4 v = src[g];
        int32_t m[4], idx[4];
        zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
        for (int j = 0; j < 4; ++j) energy += (uint64_t)((int64_t)m[j] * m[j]);            // (0 where the slot holds nothing)
    }
    energy = zl_ky_block_sum(energy, sRed);
    if (tid == 0) { ZlKyStat st; st.energy = energy; st.silent = energy < R.floor_ ? 1 : 0; st.reserved = 0; stat[f] = st; }
}

__global__ void __launch_bounds__(ZL_KY_THREADS) zl_k_key_correlate(const ZlKyRequest *__restrict__ reqs, int32_t nreq, const ZlKyBin *__restrict__ bins,
                                                                     const uint32_t *__restrict__ P, const ZlKyStat *__restrict__ stat, ZlKyAcc *__restrict__ acc)
{
    __shared__ __attribute__((aligned(16))) uint32_t sP[ZL_KY_TABLE];
    __shared__ int32_t sM[ZL_KY_CHUNK];
    const int32_t item = (int32_t)blockIdx.x;
    const ZlKyRequest R = reqs[zl_ky_find<true>(reqs, nreq, item)];
    int32_t frame, group;
    zl_ky_item_of(R, item - R.item_base, &frame, &group);
    const int tid = threadIdx.x, lane = tid & (ZL_KY_BIN_LANES - 1);
    const int32_t b = group * ZL_KY_ITEM_BINS + tid / ZL_KY_BIN_LANES;
    const bool live = b < R.nbins;
    ZlKyAcc *const dst = acc + R.acc_base + (int64_t)frame * R.nbins + b;
    if (stat[R.frame_base + frame].silent) {                       // (the same verdict in every thread: nobody waits at a barrier)
        if (live && lane == 0) { ZlKyAcc z; z.re = 0; z.im = 0; *dst = z; }
        return;
    }
#pragma unroll
    for (int i = 0; i < ZL_KY_TABLE / 4 / ZL_KY_THREADS; ++i) ((zl_ky_u32x4 *)sP)[i * ZL_KY_THREADS + tid] = ((ZlKyGlobal<zl_ky_u32x4>)P)[i * ZL_KY_THREADS + tid];
    // the group's widest window is its first bin's (the lowest note); the others lie inside it
    const ZlKyBin wide = bins[R.bin_base + group * ZL_KY_ITEM_BINS];
    const ZlKyBin B = bins[R.bin_base + (live ? b : group * ZL_KY_ITEM_BINS)];
    const int32_t off = zl_ky_bin_off(R, B), w0 = zl_ky_bin_off(R, wide), w1 = w0 + wide.n;
    const int64_t s0 = zl_ky_frame_start(R, frame);
    const uint32_t dstep = B.step * (uint32_t)ZL_KY_BIN_LANES, dwstep = B.wstep * (uint32_t)ZL_KY_BIN_LANES;
    int64_t re = 0, im = 0;
    for (int32_t c0 = w0; c0 < w1; c0 += ZL_KY_CHUNK) {
        const int32_t c1 = c0 + ZL_KY_CHUNK < w1 ? c0 + ZL_KY_CHUNK : w1;
        int64_t f0, f1, g0, g1;
        zl_ov_groups(s0 + c0, s0 + c1, R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const ZlKyGlobal<zl_ky_f32x4> src = (ZlKyGlobal<zl_ky_f32x4>)R.src + g0;
        __syncthreads();                                           // (the last chunk's readers are done; the first time: nothing)
        for (int32_t g = tid; g < ngroups; g += ZL_KY_THREADS) {
            const zl_ky_f32x4 v = src[g];
            int32_t m[4], idx[4];
            zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
            for (int j = 0; j < 4; ++j) if (idx[j] >= 0) sM[idx[j]] = m[j];               // idx < c1 - c0 <= ZL_KY_CHUNK
        }
        __syncthreads();                                           // (the first time it also publishes the table)
        if (!live) continue;
        int32_t j0, j1;
        zl_ky_lane_range(off, B.n, c0, c1, lane, &j0, &j1);
        const int32_t *m = sM + (off - c0);                        // sample j of the bin is staged at j + off - c0, inside [0, c1 - c0) for j in [j0, j1)
        uint32_t ph = (uint32_t)j0 * B.step, wph = (uint32_t)j0 * B.wstep;
#pragma unroll 4
        for (int32_t j = j0; j < j1; j += ZL_KY_BIN_LANES) {
            const int32_t v = zl_ky_windowed(m[j], zl_ky_window(zl_ky_pair_cos(sP[wph >> 20])));
            const uint32_t p = sP[ph >> 20];
            re += (int64_t)(v * zl_ky_pair_cos(p));
            im += (int64_t)(v * zl_ky_pair_sin(p));
            ph += dstep; wph += dwstep;
        }
    }
#pragma unroll
    for (int d = 1; d < ZL_KY_BIN_LANES; d <<= 1) {
        re += (int64_t)__shfl_xor((long long)re, d, ZL_KY_WAVE);
        im += (int64_t)__shfl_xor((long long)im, d, ZL_KY_WAVE);
    }
    if (live && lane == 0) { ZlKyAcc a; a.re = re; a.im = im; *dst = a; }
}

__global__ void __launch_bounds__(ZL_KY_THREADS) zl_k_key_fold(const ZlKyRequest *__restrict__ reqs, const ZlKyBin *__restrict__ bins, const ZlKyStat *__restrict__ stat,
                                                                const ZlKyAcc *__restrict__ acc, uint64_t *__restrict__ totals, ZlKyResult *__restrict__ out)
{
    __shared__ uint64_t sTotal[ZL_KY_MAX_BINS];
    __shared__ int32_t sClass[ZL_KY_MAX_BINS];
    const ZlKyRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const ZlKyStat *const S = stat + R.frame_base;
    if (tid < R.nbins) {
        const ZlKyBin B = bins[R.bin_base + tid];
        const ZlKyAcc *a = acc + R.acc_base + tid;
        uint64_t t = 0;
        for (int32_t k = 0; k < R.frames; ++k, a += R.nbins)
            if (!S[k].silent) t += zl_ky_counted(a->re, a->im, B.n, R.span, S[k].energy);
        totals[R.bin_base + tid] = t;
        sTotal[tid] = t; sClass[tid] = B.note % 12;
    }
    __syncthreads();
    if (tid < 12) {
        uint64_t c = 0;
        for (int32_t b = 0; b < R.nbins; ++b) if (sClass[b] == tid) c += sTotal[b];
        out[blockIdx.x].chroma[tid] = c;
    }
    if (tid == 12) {
        int32_t sounding = 0;
        for (int32_t k = 0; k < R.frames; ++k) sounding += S[k].silent ? 0 : 1;
        ZlKyResult *o = &out[blockIdx.x];
        o->tonic = 0; o->mode = 0; o->second_tonic = 0; o->second_mode = 0; o->frames = R.frames; o->sounding = sounding;
        o->confidence = 0.0; o->second_confidence = 0.0;
    }
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_key_gate(const ZlKyRequest *reqs, int32_t nreq, int64_t frames, ZlKyStat *stat, hipStream_t s)
{
    if (nreq <= 0 || frames <= 0) return 0;
    hipLaunchKernelGGL(zl_k_key_gate, dim3((unsigned)frames), dim3(ZL_KY_THREADS), 0, s, reqs, nreq, stat);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_key_correlate(const ZlKyRequest *reqs, int32_t nreq, int64_t items, const ZlKyBin *bins, const uint32_t *P, const ZlKyStat *stat, ZlKyAcc *acc, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(zl_k_key_correlate, dim3((unsigned)items), dim3(ZL_KY_THREADS), 0, s, reqs, nreq, bins, P, stat, acc);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_key_fold(const ZlKyRequest *reqs, int32_t nreq, const ZlKyBin *bins, const ZlKyStat *stat, const ZlKyAcc *acc, uint64_t *totals, ZlKyResult *out, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_key_fold, dim3((unsigned)nreq), dim3(ZL_KY_THREADS), 0, s, reqs, bins, stat, acc, totals, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
