// zl_tempo.hip -- HIP kernels of the tempo estimate (zlhip_sound_tempo / _batch; the definition is in zl_tempo.h).
//
//   zl_k_onset_energy   (zl_onset.hip) the only pass that reads the clip: one uint64 per hop.
//   zl_k_tempo_flux     one workgroup per request: R = isqrt(E), its maximum (integers: any order), the shift, W as uint16, the sum of
//                       W and A[0]; it also zeroes the request's A, so there is no memset.
//   zl_k_tempo_acf      the hot path.  A workgroup takes one work item (request, tile of 256 lags, segment of at most 4096 hops) and
//                       finds its request by bisection over the records' item_base.  The segment's W[h] and the lagged window
//                       W[h - l] of the tile are staged in LDS as uint16 (16.5 KB); a lane owns one lag, so W[h] is a broadcast read
//                       and the lagged read is consecutive across the lanes; eight h per iteration, a 64-bit accumulator (the
//                       products reach 2^32), one no-return 64-bit atomicAdd per lane into A[l] -- a plain store where the request
//                       has one segment.  Integer sums commute: the bits do not depend on the order.  What lies before hop 0 or at
//                       or behind `hops` is staged as zero without forming its address.
//   zl_k_tempo_pick     one workgroup per request: the coarse argmax in the order of zl_tp_beats (a total preorder: wave shuffle,
//                       then LDS), the doublings by one lane, the integer record into host memory mapped into the device.
//
// A call is these four launches, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_tempo.h"

#define ZL_TP_THREADS 256
#define ZL_TP_WAVE 64
#define ZL_TP_WAVES_PER_BLOCK (ZL_TP_THREADS / ZL_TP_WAVE)
#define ZL_TP_UNROLL 8

static_assert(ZL_TP_THREADS == ZL_TP_TILE, "one lane per lag of the tile");
static_assert(ZL_TP_SEG % ZL_TP_UNROLL == 0, "the segment is a whole number of iterations");

namespace {

__device__ __forceinline__ uint64_t zl_tp_shfl_xor(uint64_t v, int d) { return (uint64_t)__shfl_xor((unsigned long long)v, d, ZL_TP_WAVE); }

// the sum / the maximum over the workgroup, in every thread.  sRed: ZL_TP_WAVES_PER_BLOCK words of LDS
template <bool kMax> __device__ __forceinline__ uint64_t zl_tp_block_reduce(uint64_t v, uint64_t *sRed)
{
#pragma unroll
    for (int d = 1; d < ZL_TP_WAVE; d <<= 1) { const uint64_t t = zl_tp_shfl_xor(v, d); v = kMax ? (t > v ? t : v) : v + t; }
    __syncthreads();                                               // (sRed's last readers are done)
    if ((threadIdx.x & (ZL_TP_WAVE - 1)) == 0) sRed[threadIdx.x / ZL_TP_WAVE] = v;
    __syncthreads();
    uint64_t r = sRed[0];
#pragma unroll
    for (int w = 1; w < ZL_TP_WAVES_PER_BLOCK; ++w) r = kMax ? (sRed[w] > r ? sRed[w] : r) : r + sRed[w];
    return r;
}

}  // namespace

__global__ void __launch_bounds__(ZL_TP_THREADS) zl_k_tempo_flux(const ZlTpRequest *__restrict__ reqs, const uint64_t *__restrict__ Eall, uint16_t *__restrict__ Wall,
                                                                 uint64_t *__restrict__ Aall, ZlTpStat *__restrict__ stat)
{
    __shared__ uint64_t sRed[ZL_TP_WAVES_PER_BLOCK];
    const ZlTpRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t *E = Eall + R.hop_base;
    uint16_t *W = Wall + R.hop_base;
    uint64_t *A = Aall + R.acf_base;
    for (int32_t l = tid; l < R.nlags; l += ZL_TP_THREADS) A[l] = 0;
    uint64_t rmax = 0;
    for (int32_t h = tid; h < R.hops; h += ZL_TP_THREADS) { const uint64_t r = zl_tp_isqrt(E[h]); rmax = r > rmax ? r : rmax; }
    rmax = zl_tp_block_reduce<true>(rmax, sRed);
    const int32_t shift = zl_tp_shift(rmax);
    uint64_t sum = 0, sq = 0;
    for (int32_t h = tid; h < R.hops; h += ZL_TP_THREADS) {
        const uint32_t w = zl_tp_flux(zl_tp_isqrt(E[h]), h > 0 ? zl_tp_isqrt(E[h - 1]) : 0, shift);
        W[h] = (uint16_t)w;
        sum += w;
        sq += (uint64_t)w * w;
    }
    sum = zl_tp_block_reduce<false>(sum, sRed);
    sq = zl_tp_block_reduce<false>(sq, sRed);
    if (tid == 0) { ZlTpStat st; st.acf_zero = sq; st.sum = sum; st.shift = shift; st.pad = 0; stat[blockIdx.x] = st; }
}

__global__ void __launch_bounds__(ZL_TP_THREADS) zl_k_tempo_acf(const ZlTpRequest *__restrict__ reqs, int32_t nreq, const uint16_t *__restrict__ Wall,
                                                                uint64_t *__restrict__ Aall)
{
    __shared__ __attribute__((aligned(16))) uint16_t sH[ZL_TP_SEG];
    __shared__ __attribute__((aligned(16))) uint16_t sL[ZL_TP_SEG + ZL_TP_TILE];
    const int32_t item = (int32_t)blockIdx.x;
    // the request of the item: the last one whose item_base is <= item (item_base does not decrease; a request without items shares its
    // base with the next one, which is then the one found)
    int32_t r = 0;
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= item) lo = mid; else hi = mid - 1;
    }
    const ZlTpRequest R = reqs[r];
    int32_t tile, seg;
    zl_tp_item_of(R, item - R.item_base, &tile, &seg);
    if (!zl_tp_item_live(R, tile, seg)) return;                    // (the same in every lane)
    const int tid = threadIdx.x;
    const uint16_t *W = Wall + R.hop_base;
    for (int32_t i = tid; i < ZL_TP_SEG; i += ZL_TP_THREADS) {
        const int32_t h = zl_tp_h_index(R, seg, i);
        sH[i] = h >= 0 ? W[h] : (uint16_t)0;
    }
    for (int32_t j = tid; j < ZL_TP_SEG + ZL_TP_TILE; j += ZL_TP_THREADS) {
        const int32_t h = zl_tp_l_index(R, tile, seg, j);
        sL[j] = h >= 0 ? W[h] : (uint16_t)0;
    }
    __syncthreads();
    const int32_t h0 = zl_tp_seg_hop(seg);
    const int32_t len = R.hops - h0 < ZL_TP_SEG ? R.hops - h0 : ZL_TP_SEG;
    const int32_t iters = (len + ZL_TP_UNROLL - 1) / ZL_TP_UNROLL;         // (the words behind `len` are zeros)
    const uint16_t *win = sL + zl_tp_window_word(0, tid);
    uint64_t acc = 0;
    for (int32_t it = 0; it < iters; ++it) {
        const int32_t i = it * ZL_TP_UNROLL;
        const uint4 hv = *(const uint4 *)(sH + i);                 // eight W[h], the same address in every lane
        const uint32_t hw[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int k = 0; k < ZL_TP_UNROLL; ++k) {
            const uint32_t a = (k & 1) ? hw[k >> 1] >> 16 : hw[k >> 1] & 0xffffu;
            acc += (uint64_t)a * (uint64_t)win[i + k];
        }
    }
    const int32_t l = tile * ZL_TP_TILE + tid;                     // counted from first_lag
    if (l < R.nlags) {
        uint64_t *A = Aall + R.acf_base + l;
        if (R.nsegs == 1) *A = acc;
        else if (acc != 0) (void)atomicAdd((unsigned long long *)A, (unsigned long long)acc);
    }
}

__global__ void __launch_bounds__(ZL_TP_THREADS) zl_k_tempo_pick(const ZlTpRequest *__restrict__ reqs, const uint64_t *__restrict__ Aall, const ZlTpStat *__restrict__ stat,
                                                                 ZlTpResult *__restrict__ out)
{
    __shared__ uint64_t sA[ZL_TP_WAVES_PER_BLOCK];
    __shared__ int32_t sLag[ZL_TP_WAVES_PER_BLOCK];
    const ZlTpRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t *A = Aall + R.acf_base;
    // the coarse argmax: every lane the best of its lags, then the wave, then the workgroup.  lag 0 = none yet
    int32_t bl = 0; uint64_t ba = 0;
    for (int32_t l = R.lmin + tid; l <= R.lmax; l += ZL_TP_THREADS) {
        const uint64_t a = A[l - R.first_lag];
        if (bl == 0 || zl_tp_beats(a, l, ba, bl, R.hops)) { bl = l; ba = a; }
    }
#pragma unroll
    for (int d = 1; d < ZL_TP_WAVE; d <<= 1) {
        const int32_t ol = __shfl_xor(bl, d, ZL_TP_WAVE);
        const uint64_t oa = (uint64_t)__shfl_xor((unsigned long long)ba, d, ZL_TP_WAVE);
        if (ol != 0 && (bl == 0 || zl_tp_beats(oa, ol, ba, bl, R.hops))) { bl = ol; ba = oa; }
    }
    if ((tid & (ZL_TP_WAVE - 1)) == 0) { sA[tid / ZL_TP_WAVE] = ba; sLag[tid / ZL_TP_WAVE] = bl; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ZL_TP_WAVES_PER_BLOCK; ++w)
            if (sLag[w] != 0 && (bl == 0 || zl_tp_beats(sA[w], sLag[w], ba, bl, R.hops))) { bl = sLag[w]; ba = sA[w]; }
        zl_tp_record(R, stat[blockIdx.x], A, bl, &out[blockIdx.x]);
    }
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_tempo_flux(const ZlTpRequest *reqs, int32_t nreq, const uint64_t *E, uint16_t *W, uint64_t *A, ZlTpStat *stat, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_tempo_flux, dim3((unsigned)nreq), dim3(ZL_TP_THREADS), 0, s, reqs, E, W, A, stat);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_tempo_acf(const ZlTpRequest *reqs, int32_t nreq, int64_t items, const uint16_t *W, uint64_t *A, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(zl_k_tempo_acf, dim3((unsigned)items), dim3(ZL_TP_THREADS), 0, s, reqs, nreq, W, A);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_tempo_pick(const ZlTpRequest *reqs, int32_t nreq, const uint64_t *A, const ZlTpStat *stat, ZlTpResult *out, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_tempo_pick, dim3((unsigned)nreq), dim3(ZL_TP_THREADS), 0, s, reqs, A, stat, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
