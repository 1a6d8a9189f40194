// zl_onset.hip -- HIP kernels of the transient detection (zlhip_sound_onsets / _batch; the definition is in zl_onset.h).
//
//   zl_k_onset_energy   the only pass that reads the clip.  One wavefront per hop: every wavefront takes a run of consecutive hops of
//                       the call and finds the request of its first hop by bisection over the requests' hop_base.  16-byte loads of the
//                       arena's layout, one group per lane, head and tail masked by float index, samples quantised and squared as
//                       integers, an integer butterfly over the wave, lane 0 stores E[h]: a hop has exactly one writer, so there is
//                       no atomic and no memset.
//   zl_k_onset_pick     one workgroup per request, over one word per hop: the novelty N, the running maxima per block of min_gap hops
//                       (zl_on_scan_block), the candidates' histogram of strengths in LDS and its cut-off (the select rule), the kept
//                       hops compacted in hop order by a prefix count, and per kept hop one wavefront that refines the onset over two
//                       hops of samples (a lane per sub-block).  It writes a request's count and its onsets, nothing else.
//
// A call is these two launches, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_onset.h"

#define ZL_ON_THREADS 256
#define ZL_ON_WAVES_PER_BLOCK (ZL_ON_THREADS / ZL_ON_WAVE)
#define ZL_ON_MAX_BLOCKS 4096          // 256 CUs x 16 workgroups: the grid stops growing there, the waves' runs get longer
#define ZL_ON_UNROLL 4                 // 16-byte loads a lane has in flight

namespace {

template <typename T> using ZlOnGlobal = const T __attribute__((address_space(1))) *;
typedef float zl_on_f32x2 __attribute__((ext_vector_type(2)));
typedef float zl_on_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t zl_on_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 1; d < ZL_ON_WAVE; d <<= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, ZL_ON_WAVE);
    return v;
}

// exclusive prefix sum over the workgroup; *total: the sum over all threads.  sWave: ZL_ON_WAVES_PER_BLOCK words of LDS
__device__ __forceinline__ uint32_t zl_on_block_scan(uint32_t v, uint32_t *sWave, uint32_t *total)
{
    const int lane = threadIdx.x & (ZL_ON_WAVE - 1), wave = threadIdx.x / ZL_ON_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < ZL_ON_WAVE; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d, ZL_ON_WAVE);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                               // (sWave's last readers are done)
    if (lane == ZL_ON_WAVE - 1) sWave[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < ZL_ON_WAVES_PER_BLOCK; ++w) { if (w < wave) base += sWave[w]; sum += sWave[w]; }
    *total = sum;
    return base + inc - v;
}

}  // namespace

__global__ void __launch_bounds__(ZL_ON_THREADS) zl_k_onset_energy(const ZlOnRequest *__restrict__ reqs, int32_t nreq, int64_t hops, uint64_t *__restrict__ E)
{
    const int lane = threadIdx.x & (ZL_ON_WAVE - 1);
    const int64_t wave = (int64_t)blockIdx.x * ZL_ON_WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / ZL_ON_WAVE));
    const int64_t nwaves = (int64_t)gridDim.x * ZL_ON_WAVES_PER_BLOCK;
    // the wave's run of hops: [wave * hops / nwaves, (wave + 1) * hops / nwaves), without the 64-bit product
    const int64_t q = hops / nwaves, rem = hops - q * nwaves;
    int64_t it = wave * q + (wave < rem ? wave : rem);
    const int64_t end = it + q + (wave < rem ? 1 : 0);
    if (it >= end) return;

    // the request of the first hop: the last one whose hop_base is <= it (hop_base is increasing, reqs[0].hop_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].hop_base <= it) lo = mid; else hi = mid - 1;
    }
    ZlOnRequest R = reqs[r];
    for (; it < end; ++it) {
        while (r + 1 < nreq && reqs[r + 1].hop_base <= it) R = reqs[++r];       // (requests hold at least one hop each)
        int64_t lo, hi, f0, f1, g0, g1;
        zl_on_hop_range(R.first, R.frames, R.hop, it - R.hop_base, &lo, &hi);
        zl_ov_groups(lo, hi, R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const ZlOnGlobal<zl_on_f32x4> src = (ZlOnGlobal<zl_on_f32x4>)R.src + g0;
        uint64_t acc = 0;
        for (int32_t gb = 0; gb < ngroups; gb += ZL_ON_UNROLL * ZL_ON_WAVE) {
            zl_on_f32x4 v[ZL_ON_UNROLL];
#pragma unroll
            for (int k = 0; k < ZL_ON_UNROLL; ++k) {
                v[k] = zl_on_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (gb + k * ZL_ON_WAVE < ngroups) {               // (the same in every lane)
                    const int32_t g = gb + k * ZL_ON_WAVE + lane;
                    v[k] = src[g < ngroups ? g : ngroups - 1];     // lanes behind the hop read its last group again and mask all of it
                }
            }
#pragma unroll
            for (int k = 0; k < ZL_ON_UNROLL; ++k) {
                const int32_t g = gb + k * ZL_ON_WAVE + lane;
                if (g < ngroups) {
                    // four squares of at most 32767^2: their sum fits 32 bits
                    uint32_t s = 0;
                    s += zl_ov_valid(g, 0, head, count) ? zl_on_sq(v[k].x) : 0u;
                    s += zl_ov_valid(g, 1, head, count) ? zl_on_sq(v[k].y) : 0u;
                    s += zl_ov_valid(g, 2, head, count) ? zl_on_sq(v[k].z) : 0u;
                    s += zl_ov_valid(g, 3, head, count) ? zl_on_sq(v[k].w) : 0u;
                    acc += s;
                }
            }
        }
        acc = zl_on_wave_sum(acc);
        if (lane == 0) E[it] = acc;                                // the wave owns the hop
    }
}

__global__ void __launch_bounds__(ZL_ON_THREADS) zl_k_onset_pick(const ZlOnRequest *__restrict__ reqs, const uint64_t *__restrict__ Eall, int32_t *__restrict__ Nall,
                                                                 uint32_t *__restrict__ psAll, int32_t *__restrict__ counts, ZlOnOnset *__restrict__ outAll)
{
    __shared__ uint32_t sHist[ZL_ON_LEVELS];
    __shared__ int32_t sKept[ZL_ON_MAX_ONSETS];
    __shared__ uint32_t sWave[ZL_ON_WAVES_PER_BLOCK];
    __shared__ int32_t sCut[2];

    const ZlOnRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t *E = Eall + R.hop_base;
    int32_t *N = Nall + R.hop_base;
    uint32_t *ps = psAll + R.hop_base;

    // the novelty, one word per hop
    for (int32_t h = tid; h < R.hops; h += ZL_ON_THREADS) N[h] = zl_on_novelty(E[h], h > 0 ? E[h - 1] : 0, R.floor_);
    for (int32_t s = tid; s < ZL_ON_LEVELS; s += ZL_ON_THREADS) sHist[s] = 0u;
    __syncthreads();
    // the running maxima of every block of min_gap hops
    const int32_t nblocks = (R.hops + R.min_gap - 1) / R.min_gap;
    for (int32_t b = tid; b < nblocks; b += ZL_ON_THREADS) zl_on_scan_block(N, ps, R.hops, R.min_gap, b);
    __syncthreads();
    // the candidates' strengths
    for (int32_t h = tid; h < R.hops; h += ZL_ON_THREADS)
        if (zl_on_candidate(N, ps, R.hops, R.min_gap, R.threshold, h)) atomicAdd(&sHist[N[h]], 1u);
    __syncthreads();
    if (tid == 0) zl_on_cutoff(sHist, R.max_onsets, &sCut[0], &sCut[1]);
    __syncthreads();
    const int32_t cut = sCut[0], quota = sCut[1];
    // the kept hops in hop order: everything above the cut-off, and of those equal to it the first `quota`
    uint32_t above = 0, equal = 0;                                 // of the hops in front of the tile
    for (int32_t h0 = 0; h0 < R.hops; h0 += ZL_ON_THREADS) {
        const int32_t h = h0 + tid;
        const bool cand = h < R.hops && zl_on_candidate(N, ps, R.hops, R.min_gap, R.threshold, h);
        const int32_t n = cand ? N[h] : 0;
        const bool isAbove = cand && n > cut, isEqual = cand && n == cut;
        uint32_t total;
        const uint32_t x = zl_on_block_scan((isAbove ? 1u : 0u) | (isEqual ? 0x10000u : 0u), sWave, &total);    // (a tile holds 256 hops)
        const uint32_t a = above + (x & 0xffffu), q = equal + (x >> 16);
        if (isAbove || (isEqual && q < (uint32_t)quota)) sKept[a + (q < (uint32_t)quota ? q : (uint32_t)quota)] = h;
        above += total & 0xffffu; equal += total >> 16;
    }
    __syncthreads();
    const int32_t kept = (int32_t)(above + (equal < (uint32_t)quota ? equal : (uint32_t)quota));
    if (tid == 0) counts[blockIdx.x] = kept;
    // refine: a wavefront per kept hop, a lane per sub-block
    const int lane = tid & (ZL_ON_WAVE - 1);
    ZlOnOnset *out = outAll + R.out_base;
    for (int32_t i = tid / ZL_ON_WAVE; i < kept; i += ZL_ON_WAVES_PER_BLOCK) {
        const int32_t h = sKept[i];
        int64_t lo, hi;
        uint64_t es = 0;
        const bool there = lane < 2 * ZL_ON_SUBBLOCKS && zl_on_subblock(R.first, R.frames, R.hop, h, lane, &lo, &hi);
        if (there) {
            if (R.channels == 2) {
                const ZlOnGlobal<zl_on_f32x2> src = (ZlOnGlobal<zl_on_f32x2>)R.src;
                for (int64_t f = lo; f < hi; ++f) { const zl_on_f32x2 v = src[f]; es += zl_on_sq(v.x); es += zl_on_sq(v.y); }
            } else {
                const ZlOnGlobal<float> src = (ZlOnGlobal<float>)R.src;
                for (int64_t f = lo; f < hi; ++f) es += zl_on_sq(src[f]);
            }
        }
        const uint64_t ep = (h > 0 ? E[h - 1] : 0) + R.floor_;
        const unsigned long long hits = __ballot(there && zl_on_hit(es, ep));
        const int first = hits ? __ffsll((long long)hits) - 1 : -1;
        if (lane == (first < 0 ? 0 : first)) {
            ZlOnOnset o;
            o.frame = first < 0 ? (int32_t)(R.first + (int64_t)h * R.hop) : (int32_t)lo;
            o.strength = N[h];
            out[i] = o;
        }
    }
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_onset_energy(const ZlOnRequest *reqs, int32_t nreq, int64_t hops, uint64_t *E, hipStream_t s)
{
    if (nreq <= 0 || hops <= 0) return 0;
    int64_t blocks = (hops + ZL_ON_WAVES_PER_BLOCK - 1) / ZL_ON_WAVES_PER_BLOCK;
    if (blocks > ZL_ON_MAX_BLOCKS) blocks = ZL_ON_MAX_BLOCKS;
    hipLaunchKernelGGL(zl_k_onset_energy, dim3((unsigned)blocks), dim3(ZL_ON_THREADS), 0, s, reqs, nreq, hops, E);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_onset_pick(const ZlOnRequest *reqs, int32_t nreq, const uint64_t *E, int32_t *N, uint32_t *ps, int32_t *counts, ZlOnOnset *out, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_onset_pick, dim3((unsigned)nreq), dim3(ZL_ON_THREADS), 0, s, reqs, E, N, ps, counts, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
