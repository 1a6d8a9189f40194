// zl_loop.hip -- HIP kernels of the loop finder (zlhip_sound_loop / _batch; the definition is in zl_loop.h).
//
//   zl_k_loop_prep      one workgroup per request and the only pass that reads the clip.  It reads the request's two strips in 16-byte
//                       groups of the arena's own layout, head and tail masked by float index (no float outside the strips is looked
//                       at), mixes and quantises them and reduces max |m|; a second pass over the same groups (they are in the cache
//                       now) writes x = m >> sh as int16 into the call's strip array.  Then a lane owns a run of consecutive
//                       candidates: E of the first by the window's sum, the following ones by sliding the window one frame.
//   zl_k_loop_pairs     the hot path.  A workgroup takes one work item (request, tile of 64 starts x 64 ends) and finds its request by
//                       bisection over the records' item_base.  256 lanes stage the item's two strip tiles, 64 + W int16 each, in
//                       LDS; behind a strip's end the staged copy is zero, so no lane reads behind a strip.  A lane owns a register
//                       tile of 4 starts x 4 ends: per four j it reads one 8-byte word per side (lanes that share a start or an end read
//                       the same address: a broadcast; the sixteen distinct addresses of a wave lie 8 bytes apart, on sixteen different
//                       banks) and keeps the samples as packed pairs (x[j], x[j + 1]), so two terms of the cross term X are one dot2;
//                       cost = E(s) + E(e) - 2 X (zl_lp_cost_from_dot: exact).  The difference form -- a packed 16-bit subtract and a
//                       dot2 of the difference with itself per two terms -- is as exact, was built and measured 1.59 times slower
//                        and is not shipped.  Lanes outside a partial tile sum over the zero fill and
//                       contribute nothing.  The item's admissible pairs are counted and the best one is reduced with
//                       zl_lp_better: shuffles over the wave, LDS over the workgroup.  Where the call keeps a cost matrix (a uniform
//                       branch on a null pointer) every candidate pair's cost is stored: one writer each.
//   zl_k_loop_pick      one workgroup per request: the best of its items, the sum of their pairs, the nominal pair's cost straight
//                       from the strips (W terms); one lane writes the integer record into host memory mapped into the device.
//
// A call is these three launches, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_loop.h"

#define ZL_LP_THREADS 256
#define ZL_LP_WAVE 64
#define ZL_LP_WAVES_PER_BLOCK (ZL_LP_THREADS / ZL_LP_WAVE)

static_assert(ZL_LP_THREADS * ZL_LP_LANE * ZL_LP_LANE == ZL_LP_TILE * ZL_LP_TILE, "the lanes' register tiles cover the item's tile");
static_assert(ZL_LP_WINDOW_MIN % 4 == 0, "a window is a whole number of 8-byte words");

namespace {

template <typename T> using ZlLpGlobal = const T __attribute__((address_space(1))) *;
typedef float zl_lp_f32x4 __attribute__((ext_vector_type(4)));
typedef short zl_lp_i16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t zl_lp_shfl_xor(uint64_t v, int d) { return (uint64_t)__shfl_xor((unsigned long long)v, d, ZL_LP_WAVE); }

// the sum / maximum over the workgroup, in every thread.  sRed: ZL_LP_WAVES_PER_BLOCK words of LDS
template <bool kMax> __device__ __forceinline__ uint64_t zl_lp_block_reduce(uint64_t v, uint64_t *sRed)
{
#pragma unroll
    for (int d = 1; d < ZL_LP_WAVE; d <<= 1) { const uint64_t o = zl_lp_shfl_xor(v, d); v = kMax ? (o > v ? o : v) : v + o; }
    __syncthreads();                                               // (sRed's last readers are done)
    if ((threadIdx.x & (ZL_LP_WAVE - 1)) == 0) sRed[threadIdx.x / ZL_LP_WAVE] = v;
    __syncthreads();
    uint64_t r = sRed[0];
#pragma unroll
    for (int w = 1; w < ZL_LP_WAVES_PER_BLOCK; ++w) r = kMax ? (sRed[w] > r ? sRed[w] : r) : r + sRed[w];
    return r;
}

// the best pair over the workgroup (zl_lp_better is total: every lane of a wave ends with the same pair), valid in thread 0.
// sBest: ZL_LP_WAVES_PER_BLOCK pairs of LDS
__device__ __forceinline__ ZlLpPair zl_lp_block_best(ZlLpPair best, int32_t s0, int32_t e0, ZlLpPair *sBest)
{
#pragma unroll
    for (int d = 1; d < ZL_LP_WAVE; d <<= 1) {
        ZlLpPair o;
        o.s = __shfl_xor(best.s, d, ZL_LP_WAVE); o.e = __shfl_xor(best.e, d, ZL_LP_WAVE);
        o.cost = (uint32_t)__shfl_xor((int)best.cost, d, ZL_LP_WAVE); o.den = (uint32_t)__shfl_xor((int)best.den, d, ZL_LP_WAVE);
        if (zl_lp_better(o, best, s0, e0)) best = o;
    }
    __syncthreads();
    if ((threadIdx.x & (ZL_LP_WAVE - 1)) == 0) sBest[threadIdx.x / ZL_LP_WAVE] = best;
    __syncthreads();
    ZlLpPair r = sBest[0];
#pragma unroll
    for (int w = 1; w < ZL_LP_WAVES_PER_BLOCK; ++w) if (zl_lp_better(sBest[w], r, s0, e0)) r = sBest[w];
    return r;
}

// the request of item `at`: the last one whose item_base is <= at (the bases do not decrease; a request without items shares its base
// with the next one, which is then the one found)
__device__ __forceinline__ int32_t zl_lp_find(const ZlLpRequest *__restrict__ reqs, int32_t nreq, int32_t at)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= at) lo = mid; else hi = mid - 1;
    }
}

// the packed pairs P[m] = (x[m], x[m + 1]), m = 0 .. 6, of the eight samples in two 8-byte words (x[0..3], x[4..7])
__device__ __forceinline__ void zl_lp_pairs_of(uint2 lo, uint2 hi, uint32_t *P)
{
    P[0] = lo.x; P[2] = lo.y; P[4] = hi.x; P[6] = hi.y;
    P[1] = __builtin_amdgcn_alignbyte(lo.y, lo.x, 2); P[3] = __builtin_amdgcn_alignbyte(hi.x, lo.y, 2); P[5] = __builtin_amdgcn_alignbyte(hi.y, hi.x, 2);
}

__device__ __forceinline__ zl_lp_i16x2 zl_lp_as_i16x2(uint32_t v) { return __builtin_bit_cast(zl_lp_i16x2, v); }

}  // namespace

__global__ void __launch_bounds__(ZL_LP_THREADS) zl_k_loop_prep(const ZlLpRequest *__restrict__ reqs, int16_t *__restrict__ X, uint32_t *__restrict__ E, int32_t *__restrict__ shifts)
{
    __shared__ uint64_t sRed[ZL_LP_WAVES_PER_BLOCK];
    const ZlLpRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const int32_t W = R.window, H = W >> 1;
    if (R.ns <= 0 || R.ne <= 0) { if (tid == 0) shifts[blockIdx.x] = 0; return; }       // (uniform: no candidates, no strips)
    const int32_t lo[2] = {R.smin - H, R.emin - H}, len[2] = {zl_lp_strip_len(R.ns, W), zl_lp_strip_len(R.ne, W)}, base[2] = {R.xs_base, R.xe_base};

    // pass 1: the largest |m| of the two strips
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int64_t f0, f1, g0, g1;
        zl_ov_groups(lo[k], (int64_t)lo[k] + len[k], R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const ZlLpGlobal<zl_lp_f32x4> src = (ZlLpGlobal<zl_lp_f32x4>)R.src + g0;
        for (int32_t g = tid; g < ngroups; g += ZL_LP_THREADS) {
            const zl_lp_f32x4 v = src[g];
            int32_t m[4], idx[4];
            zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const uint32_t a = (uint32_t)(m[j] < 0 ? -m[j] : m[j]); amax = a > amax ? a : amax; }
        }
    }
    amax = (uint32_t)zl_lp_block_reduce<true>(amax, sRed);
    const int32_t shift = zl_lp_shift(amax);
    if (tid == 0) shifts[blockIdx.x] = shift;

    // pass 2: x = m >> shift into the call's strips
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int64_t f0, f1, g0, g1;
        zl_ov_groups(lo[k], (int64_t)lo[k] + len[k], R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const ZlLpGlobal<zl_lp_f32x4> src = (ZlLpGlobal<zl_lp_f32x4>)R.src + g0;
        for (int32_t g = tid; g < ngroups; g += ZL_LP_THREADS) {
            const zl_lp_f32x4 v = src[g];
            int32_t m[4], idx[4];
            zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
            for (int j = 0; j < 4; ++j) if (idx[j] >= 0 && idx[j] < len[k]) X[base[k] + idx[j]] = (int16_t)(m[j] >> shift);
        }
    }
    __syncthreads();                                               // (the strips are this workgroup's own stores)

    // E per candidate: lane `tid` owns the candidates [c0, c1) of a strip
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int32_t n = k == 0 ? R.ns : R.ne, per = (n + ZL_LP_THREADS - 1) / ZL_LP_THREADS;
        const int32_t c0 = tid * per, c1 = c0 + per < n ? c0 + per : n;
        const int16_t *x = X + base[k];
        uint32_t *out = E + (k == 0 ? R.es_base : R.ee_base);
        if (c0 < c1) {
            uint32_t e = zl_lp_energy(x, c0, W);
            out[c0] = e;
            for (int32_t c = c0 + 1; c < c1; ++c) {                // c + W - 1 <= n - 1 + W - 1: the strip's last element
                const int32_t a = x[c - 1], b = x[c + W - 1];
                e = e - (uint32_t)(a * a) + (uint32_t)(b * b);
                out[c] = e;
            }
        }
    }
}

__global__ void __launch_bounds__(ZL_LP_THREADS) zl_k_loop_pairs(const ZlLpRequest *__restrict__ reqs, int32_t nreq, const int16_t *__restrict__ X, const uint32_t *__restrict__ E,
                                                                 ZlLpItem *__restrict__ out, uint32_t *__restrict__ costs)
{
    __shared__ __attribute__((aligned(16))) int16_t sS[ZL_LP_STAGE];
    __shared__ __attribute__((aligned(16))) int16_t sE[ZL_LP_STAGE];
    __shared__ ZlLpPair sBest[ZL_LP_WAVES_PER_BLOCK];
    __shared__ uint64_t sRed[ZL_LP_WAVES_PER_BLOCK];
    const int32_t item = (int32_t)blockIdx.x;
    const ZlLpRequest R = reqs[zl_lp_find(reqs, nreq, item)];
    int32_t ts, te;
    zl_lp_item_of(R, item - R.item_base, &ts, &te);
    const int tid = threadIdx.x;
    const int32_t W = R.window;
    const int32_t cs0 = ts * ZL_LP_TILE, ce0 = te * ZL_LP_TILE;
    const int32_t ncs = R.ns - cs0 < ZL_LP_TILE ? R.ns - cs0 : ZL_LP_TILE, nce = R.ne - ce0 < ZL_LP_TILE ? R.ne - ce0 : ZL_LP_TILE;
    const int32_t lenS = zl_lp_strip_len(R.ns, W), lenE = zl_lp_strip_len(R.ne, W);

    // the item's two strip tiles: candidates cs0 .. cs0 + 63 need the strip's elements [cs0, cs0 + 63 + W); zero behind the strip
    for (int32_t i = tid; i < ZL_LP_TILE + W; i += ZL_LP_THREADS) {
        sS[i] = cs0 + i < lenS ? X[R.xs_base + cs0 + i] : (int16_t)0;
        sE[i] = ce0 + i < lenE ? X[R.xe_base + ce0 + i] : (int16_t)0;
    }
    __syncthreads();

    // the lane's 4 x 4 pairs: starts a4 .. a4 + 3, ends b4 .. b4 + 3 of the tile
    const int32_t a4 = zl_lp_lane_start(tid), b4 = zl_lp_lane_end(tid);
    const uint2 *pS = (const uint2 *)(sS + a4), *pE = (const uint2 *)(sE + b4);        // 8-byte aligned: a4, b4 are multiples of 4
    int32_t acc[ZL_LP_LANE][ZL_LP_LANE];
#pragma unroll
    for (int i = 0; i < ZL_LP_LANE; ++i)
#pragma unroll
        for (int k = 0; k < ZL_LP_LANE; ++k) acc[i][k] = 0;
    uint2 curS = pS[0], curE = pE[0];
    for (int32_t jb = 0; jb < W; jb += 4) {                        // the last word read ends at element a4 + W + 3 <= 63 + W
        const uint2 nxtS = pS[(jb >> 2) + 1], nxtE = pE[(jb >> 2) + 1];
        uint32_t PS[7], PE[7];
        zl_lp_pairs_of(curS, nxtS, PS);
        zl_lp_pairs_of(curE, nxtE, PE);
#pragma unroll
        for (int jj = 0; jj < 4; jj += 2)
#pragma unroll
            for (int i = 0; i < ZL_LP_LANE; ++i)
#pragma unroll
                for (int k = 0; k < ZL_LP_LANE; ++k) {
                    acc[i][k] = __builtin_amdgcn_sdot2(zl_lp_as_i16x2(PS[i + jj]), zl_lp_as_i16x2(PE[k + jj]), acc[i][k], false);       // |X| <= 2^30
                }
        curS = nxtS; curE = nxtE;
    }

    // the lane's best admissible pair, the costs
    ZlLpPair best = zl_lp_no_pair();
    uint32_t count = 0;
    uint32_t es[ZL_LP_LANE], ee[ZL_LP_LANE];
#pragma unroll
    for (int i = 0; i < ZL_LP_LANE; ++i) {
        es[i] = a4 + i < ncs ? E[R.es_base + cs0 + a4 + i] : 0u;
        ee[i] = b4 + i < nce ? E[R.ee_base + ce0 + b4 + i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < ZL_LP_LANE; ++i)
#pragma unroll
        for (int k = 0; k < ZL_LP_LANE; ++k) {
            if (a4 + i >= ncs || b4 + k >= nce) continue;          // outside a partial tile: nothing
            const int32_t cs = cs0 + a4 + i, ce = ce0 + b4 + k;
            ZlLpPair p;
            p.s = R.smin + cs; p.e = R.emin + ce;
            p.cost = zl_lp_cost_from_dot(es[i], ee[k], acc[i][k]);
            p.den = zl_lp_den(es[i], ee[k]);
            if (costs) costs[R.cost_base + (int64_t)cs * R.ne + ce] = p.cost;
            if (!zl_lp_admissible(p.s, p.e, R.min_length)) continue;
            ++count;
            if (zl_lp_better(p, best, R.s0, R.e0)) best = p;
        }
    const uint64_t pairs = zl_lp_block_reduce<false>(count, sRed);
    best = zl_lp_block_best(best, R.s0, R.e0, sBest);
    if (tid == 0) out[item] = zl_lp_item_record(best, pairs);
}

__global__ void __launch_bounds__(ZL_LP_THREADS) zl_k_loop_pick(const ZlLpRequest *__restrict__ reqs, const int16_t *__restrict__ X, const uint32_t *__restrict__ E,
                                                                const int32_t *__restrict__ shifts, const ZlLpItem *__restrict__ items, ZlLpResult *__restrict__ out)
{
    __shared__ ZlLpPair sBest[ZL_LP_WAVES_PER_BLOCK];
    __shared__ uint64_t sRed[ZL_LP_WAVES_PER_BLOCK];
    const ZlLpRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const int32_t n = zl_lp_items(R);
    ZlLpPair best = zl_lp_no_pair();
    uint64_t pairs = 0;
    for (int32_t i = tid; i < n; i += ZL_LP_THREADS) {
        const ZlLpItem it = items[R.item_base + i];
        ZlLpPair p; p.s = it.start; p.e = it.stop; p.cost = it.cost; p.den = it.den;
        pairs += it.pairs;
        if (zl_lp_better(p, best, R.s0, R.e0)) best = p;
    }
    pairs = zl_lp_block_reduce<false>(pairs, sRed);
    best = zl_lp_block_best(best, R.s0, R.e0, sBest);
    const bool nominal = zl_lp_nominal_valid(R);                   // (uniform)
    uint32_t ncost = 0, nden = 0;
    if (nominal) {
        const int32_t cs = R.s0 - R.smin, ce = R.e0 - R.emin;
        uint32_t part = 0;
        for (int32_t j = tid; j < R.window; j += ZL_LP_THREADS) part += zl_lp_term((int32_t)X[R.xs_base + cs + j], (int32_t)X[R.xe_base + ce + j]);
        ncost = (uint32_t)zl_lp_block_reduce<false>(part, sRed);
        nden = zl_lp_den(E[R.es_base + cs], E[R.ee_base + ce]);
    }
    if (tid == 0) zl_lp_result(R, best, pairs, shifts[blockIdx.x], nominal, ncost, nden, &out[blockIdx.x]);
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_loop_prep(const ZlLpRequest *reqs, int32_t nreq, int16_t *X, uint32_t *E, int32_t *shifts, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_loop_prep, dim3((unsigned)nreq), dim3(ZL_LP_THREADS), 0, s, reqs, X, E, shifts);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_loop_pairs(const ZlLpRequest *reqs, int32_t nreq, int64_t items, const int16_t *X, const uint32_t *E, ZlLpItem *out, uint32_t *costs, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(zl_k_loop_pairs, dim3((unsigned)items), dim3(ZL_LP_THREADS), 0, s, reqs, nreq, X, E, out, costs);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_loop_pick(const ZlLpRequest *reqs, int32_t nreq, const int16_t *X, const uint32_t *E, const int32_t *shifts, const ZlLpItem *items, ZlLpResult *out, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_loop_pick, dim3((unsigned)nreq), dim3(ZL_LP_THREADS), 0, s, reqs, X, E, shifts, items, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
