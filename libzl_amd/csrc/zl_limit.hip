// zl_limit.hip -- HIP kernels of the peak measurement and the look-ahead limiter (zlhip_sound_peak / _limit; the definition is in
// zl_limit.h).
//
//   zl_k_limit_detect  the analysis and the limiter's first pass.  A workgroup of ZL_LM_WG lanes takes one chunk of ZL_LM_CHUNK frames
//                      of one request, found by bisection over the requests' wg_base with scalar loads.  The chunk's span -- with
//                      the true-peak flag 31 frames before and 32 behind as well, clipped to the region -- is read in 16-byte groups
//                      of the arena's own layout, head and tail masked by float index; with the flag v goes planar into LDS (zeros
//                      first: what lies outside the region is +0) and every lane runs the F - 1 phase rows of its frames from there:
//                      consecutive lanes read consecutive words, the coefficients are uniform.  Maxima as bits: shuffles over the
//                      wave, LDS over the workgroup, and lane 0 writes the chunk's record with one 16-byte vector store.  One writer
//                      per record, no atomics, no memset.
//   zl_k_limit_render  the hot path.  A workgroup is one tile of ZL_LM_TILE output frames of one job; a lane owns ZL_LM_PER consecutive
//                      frames, the same 16-byte groups of source and destination.  Every lane reads the chunk records of the tile's
//                      reach (uniform addresses); none above the ceiling: COLD -- aligned 16-byte loads, x gain, aligned 16-byte stores.
//                      Else the workgroup recomputes the reduction r over its reach into LDS (with the flag from v staged in LDS,
//                      ips once per frame), forms the sliding maximum by LOG-STEP DOUBLING in place (after step s a word holds the
//                      maximum over [q, q + 2s); two overlapping windows of the largest power of two give the window of L + H + 1),
//                      writes mr transposed by 4, and every lane slides a register window of four over it: one LDS read per tap for
//                      four frames, consecutive lanes consecutive words.  The verdict on a non-finite written sample is a ballot per
//                      wave and one atomic OR, only when set; frames_reduced and min_gain take one vector atomic each per workgroup
//                      that has something to report.  Barriers are outside divergent code: cold or hot is the same for the whole
//                      workgroup (made uniform by readfirstlane), every trip count is the job's.
//   (the sound-table entries switch by zl_k_resample_publish, zl_resample.hip)
//
// No scratch memory.
#include <hip/hip_runtime.h>
#include "zl_limit.h"

#define ZL_LM_WAVE 64
#define ZL_LM_WAVES (ZL_LM_WG / ZL_LM_WAVE)

namespace {

typedef float zl_lm_f4 __attribute__((ext_vector_type(4)));
typedef float zl_lm_f2 __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(1))) *ZlLmGlobalF;
typedef const zl_lm_f2 __attribute__((address_space(1))) *ZlLmGlobalF2;
typedef const zl_lm_f4 __attribute__((address_space(1))) *ZlLmGlobalF4;
typedef zl_lm_f4 __attribute__((address_space(1))) *ZlLmGlobalOutF4;

template <typename T> __device__ __forceinline__ int32_t zl_lm_find(const T *__restrict__ recs, int32_t n, int32_t wg)
{
    for (int32_t lo = 0, hi = n - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (recs[mid].wg_base <= wg) lo = mid; else hi = mid - 1;
    }
}

__device__ __forceinline__ uint32_t zl_lm_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < ZL_LM_WAVE; d <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d, ZL_LM_WAVE); v = o > v ? o : v; }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(ZL_LM_WG) zl_k_limit_detect(const ZlLmScan *__restrict__ reqs, int32_t nreq, const float *__restrict__ tables, ZlLmRecord *__restrict__ records)
{
    __shared__ float sV[2][ZL_LM_DET_STAGE];
    __shared__ uint32_t sRed[ZL_LM_WAVES][4];
    const int32_t wg = (int32_t)blockIdx.x;
    const ZlLmScan S = reqs[zl_lm_find(reqs, nreq, wg)];
    const int32_t tid = (int32_t)threadIdx.x;
    const bool tp = S.F > 1;
    int32_t lo, hi, s0, s1;
    zl_lm_chunk(S, wg - S.wg_base, &lo, &hi, &s0, &s1);
    const int32_t base = lo - (ZL_LM_HALF - 1);                    // the frame of LDS index 0
    if (tp) {
        for (int32_t i = tid; i < ZL_LM_DET_STAGE; i += ZL_LM_WG) { sV[0][i] = 0.0f; sV[1][i] = 0.0f; }
    }
    __syncthreads();
    int64_t f0, f1, g0, g1;
    zl_ov_groups(s0, s1, S.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const ZlLmGlobalF4 src = (ZlLmGlobalF4)S.src + g0;
    uint32_t m[4] = {0u, 0u, 0u, 0u};                              // sample peak L, R, inter-sample peak L, R
    for (int32_t g = tid; g < ngroups; g += ZL_LM_WG) {
        const zl_lm_f4 x4 = src[g];
        const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (zl_ov_valid(g, j, head, count)) {
                const int64_t idx = 4 * (g0 + g) + j;
                const int32_t f = (int32_t)(S.channels == 2 ? idx >> 1 : idx), c = S.channels == 2 ? (int32_t)(idx & 1) : 0;
                const float v = zl_lm_v(x[j], S.gain, S.sanitize);
                if (tp) sV[c][f - base] = v;
                if (f >= lo && f < hi) m[c] = zl_lm_max_bits(m[c], zl_lm_abs_bits(v));
            }
        }
    }
    __syncthreads();
    if (tp) {
        const float *table = tables + zl_lm_table_at(S.F);
        for (int32_t f = lo + tid; f < hi; f += ZL_LM_WG) {
            for (int32_t c = 0; c < S.channels; ++c) m[2 + c] = zl_lm_max_bits(m[2 + c], zl_lm_ips_bits(table, S.F, &sV[c][f - lo]));
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = zl_lm_wave_max(m[k]);
    if ((tid & (ZL_LM_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sRed[tid / ZL_LM_WAVE][k] = m[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < ZL_LM_WAVES; ++w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = zl_lm_max_bits(m[k], sRed[w][k]);
        }
        zl_lm_f4 o;
        o.x = zl_lm_float(m[0]); o.y = zl_lm_float(m[1]); o.z = zl_lm_float(m[2]); o.w = zl_lm_float(m[3]);
        *(zl_lm_f4 *)(records + wg) = o;
    }
}

// elements of a lane in the strided walks over the tile's LDS arrays
#define ZL_LM_R_PER  ((ZL_LM_MAX_REACH + ZL_LM_WG - 1) / ZL_LM_WG)          // 10
#define ZL_LM_MR_PER ((ZL_LM_MAX_MR + ZL_LM_WG - 1) / ZL_LM_WG)             // 6
#define ZL_LM_V_PER  ((ZL_LM_STAGE + ZL_LM_WG - 1) / ZL_LM_WG)              // 11
#define ZL_LM_I_PER  ((ZL_LM_MAX_REACH + 1 + ZL_LM_WG - 1) / ZL_LM_WG)      // 11

__global__ void __launch_bounds__(ZL_LM_WG) zl_k_limit_render(const ZlLmJob *__restrict__ jobs, int32_t njobs, const float *__restrict__ tables, const ZlLmRecord *__restrict__ records,
                                                              const float *__restrict__ weights, ZlLmStats *__restrict__ stats, uint32_t *__restrict__ verdicts)
{
    __shared__ float sV[2][ZL_LM_STAGE];                           // v over the reach and its taps (true peak only)
    __shared__ uint32_t sIps[ZL_LM_MAX_REACH + 1];                 // ips over the reach, from one frame before it
    __shared__ uint32_t sR[ZL_LM_MAX_REACH];                       // r, then its running maxima
    __shared__ float sMr[4 * ZL_LM_MR_Q];                          // mr, transposed by 4
    __shared__ uint32_t sStat[ZL_LM_WAVES][2];
    const int32_t wg = (int32_t)blockIdx.x;
    const ZlLmJob J = jobs[zl_lm_find(jobs, njobs, wg)];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t t0 = (wg - J.wg_base) * ZL_LM_TILE;
    const bool stereo = J.channels == 2;
    const float c = J.ceiling;
    const bool hot = __builtin_amdgcn_readfirstlane(zl_lm_tile_cold(J, records + J.rec_base, t0) ? 0 : 1) != 0;
    float G[ZL_LM_PER] = {1.0f, 1.0f, 1.0f, 1.0f};
    const ZlLmGlobalF src = (ZlLmGlobalF)J.src;
    if (hot) {
        const int32_t NR = zl_lm_reach_frames(J), NM = zl_lm_mr_count(J), j0 = t0 - J.L - J.H;     // r index q is frame j0 + q
        const bool tp = J.F > 1;
        if (tp) {
            // v over [j0 - 32, j0 + NR + 32), +0 outside the clip
#pragma unroll 1
            for (int32_t e = 0; e < ZL_LM_V_PER; ++e) {
                const int32_t i = tid + e * ZL_LM_WG, f = j0 - ZL_LM_HALF + i;
                if (i < NR + ZL_LM_TAPS) {
                    float a = 0.0f, b = 0.0f;
                    if (f >= 0 && f < J.n) {
                        if (stereo) { const zl_lm_f2 x = ((ZlLmGlobalF2)src)[f]; a = x.x * J.gain; b = x.y * J.gain; }
                        else a = src[f] * J.gain;
                    }
                    sV[0][i] = a; sV[1][i] = b;
                }
            }
        }
        __syncthreads();
        if (tp) {
            // ips of the frames [j0 - 1, j0 + NR): the window of frame j0 - 1 + i starts at LDS index i
            const float *table = tables + zl_lm_table_at(J.F);
#pragma unroll 1
            for (int32_t e = 0; e < ZL_LM_I_PER; ++e) {
                const int32_t i = tid + e * ZL_LM_WG, f = j0 - 1 + i;
                if (i < NR + 1) {
                    uint32_t b = 0u;
                    if (f >= 0 && f < J.n) {
                        b = zl_lm_ips_bits(table, J.F, &sV[0][i]);
                        if (stereo) b = zl_lm_max_bits(b, zl_lm_ips_bits(table, J.F, &sV[1][i]));
                    }
                    sIps[i] = b;
                }
            }
        }
        __syncthreads();
        // r over the reach; a lane keeps its words in registers through the doubling
        uint32_t val[ZL_LM_R_PER];
#pragma unroll
        for (int32_t e = 0; e < ZL_LM_R_PER; ++e) {
            const int32_t q = tid + e * ZL_LM_WG, f = j0 + q;
            uint32_t r = 0u;
            if (q < NR && f >= 0 && f < J.n) {
                uint32_t p;
                if (tp) {
                    p = zl_lm_max_bits(zl_lm_abs_bits(sV[0][q + ZL_LM_HALF]), zl_lm_abs_bits(sV[1][q + ZL_LM_HALF]));
                    p = zl_lm_max_bits(p, zl_lm_max_bits(sIps[q], sIps[q + 1]));
                } else if (stereo) {
                    const zl_lm_f2 x = ((ZlLmGlobalF2)src)[f];
                    p = zl_lm_max_bits(zl_lm_abs_bits(x.x * J.gain), zl_lm_abs_bits(x.y * J.gain));
                } else {
                    p = zl_lm_abs_bits(src[f] * J.gain);
                }
                r = zl_lm_bits(zl_lm_reduction(p, c));
            }
            val[e] = r;
            if (q < NR) sR[q] = r;
        }
        __syncthreads();
        // the sliding maximum by log-step doubling: after the step s a word is the maximum over [q, q + 2 s), clipped to the reach
        const int32_t W = J.L + J.H + 1, P = zl_lm_pow2(W);
#pragma unroll 1
        for (int32_t s = 1; s < P; s <<= 1) {
            uint32_t nb[ZL_LM_R_PER];
#pragma unroll
            for (int32_t e = 0; e < ZL_LM_R_PER; ++e) {
                const int32_t q = tid + e * ZL_LM_WG;
                nb[e] = q + s < NR ? sR[q + s] : 0u;
            }
            __syncthreads();
#pragma unroll
            for (int32_t e = 0; e < ZL_LM_R_PER; ++e) {
                const int32_t q = tid + e * ZL_LM_WG;
                val[e] = zl_lm_max_bits(val[e], nb[e]);
                if (q < NR) sR[q] = val[e];
            }
            __syncthreads();
        }
        // mr[m] = the maximum over [m, m + W) = two windows of P
#pragma unroll
        for (int32_t e = 0; e < ZL_LM_MR_PER; ++e) {
            const int32_t m = tid + e * ZL_LM_WG;
            if (m < NM) sMr[zl_lm_mr_pos(m)] = zl_lm_float(zl_lm_max_bits(sR[m], sR[m + W - P]));
        }
        __syncthreads();
        // R of the lane's four frames: frame t0 + 4 tid + e reads mr index 4 tid + e + L - k at the tap k
        const int32_t m0 = ZL_LM_PER * tid + J.L;
        float win[ZL_LM_PER], acc[ZL_LM_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int32_t e = 0; e < ZL_LM_PER; ++e) win[e] = sMr[zl_lm_mr_pos(m0 + e)];
        const float *w = weights + J.weights;
#pragma unroll 4
        for (int32_t k = 0; k <= J.L; ++k) {
            const float wk = w[k];
#pragma unroll
            for (int32_t e = 0; e < ZL_LM_PER; ++e) { const float p = wk * win[e]; acc[e] = acc[e] + p; }
            win[3] = win[2]; win[2] = win[1]; win[1] = win[0];
            win[0] = k < J.L ? sMr[zl_lm_mr_pos(m0 - k - 1)] : 0.0f;
        }
        uint32_t reduced = 0u, mn = 0x3f800000u;
#pragma unroll
        for (int32_t e = 0; e < ZL_LM_PER; ++e) {
            G[e] = zl_lm_gain_of(acc[e]);
            if (t0 + ZL_LM_PER * tid + e < J.n) {
                reduced += G[e] < 1.0f ? 1u : 0u;
                const uint32_t b = zl_lm_bits(G[e]);
                mn = b < mn ? b : mn;
            }
        }
#pragma unroll
        for (int d = 1; d < ZL_LM_WAVE; d <<= 1) {
            reduced += (uint32_t)__shfl_xor((int)reduced, d, ZL_LM_WAVE);
            const uint32_t o = (uint32_t)__shfl_xor((int)mn, d, ZL_LM_WAVE);
            mn = o < mn ? o : mn;
        }
        if ((tid & (ZL_LM_WAVE - 1)) == 0) { sStat[tid / ZL_LM_WAVE][0] = reduced; sStat[tid / ZL_LM_WAVE][1] = mn; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w_ = 1; w_ < ZL_LM_WAVES; ++w_) { reduced += sStat[w_][0]; mn = sStat[w_][1] < mn ? sStat[w_][1] : mn; }
            if (reduced != 0u) {
                atomicAdd(&stats[J.verdict].frames_reduced, reduced);
                atomicMin(&stats[J.verdict].min_gain_bits, mn);
            }
        }
    }
    // the lane's groups: the same of source and destination; what lies behind the data is produced, not copied
    bool bad = false;
    const int64_t groups = zl_lm_groups(J), data = (int64_t)J.n * J.channels;
    const int32_t per = stereo ? 2 : 1;
    const int64_t gfirst = (int64_t)(wg - J.wg_base) * zl_lm_tile_groups(J.channels) + (int64_t)tid * per;
#pragma unroll
    for (int32_t h = 0; h < 2; ++h) {
        const int64_t g = gfirst + h;
        if (h < per && g < groups) {
            float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (4 * g < data) {
                const zl_lm_f4 x4 = ((ZlLmGlobalF4)src)[g];
                const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * g + j < data) {
                        const float v = x[j] * J.gain;
                        // (the frame of float j among the lane's four: stereo 2 h + j / 2, mono j)
                        y[j] = hot ? zl_lm_apply(v, G[stereo ? 2 * h + (j >> 1) : j], c) : v;
                        bad = bad || !zl_lm_finite(y[j]);
                    }
                }
            }
            zl_lm_f4 o; o.x = y[0]; o.y = y[1]; o.z = y[2]; o.w = y[3];
            ((ZlLmGlobalOutF4)J.dst)[g] = o;
        }
    }
    const bool any = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (any && (tid & (ZL_LM_WAVE - 1)) == 0) atomicOr(verdicts + J.verdict, 1u);
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_limit_detect(const ZlLmScan *reqs, int32_t nreq, int32_t wgs, const float *tables, ZlLmRecord *records, hipStream_t s)
{
    if (nreq <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_limit_detect, dim3((unsigned)wgs), dim3(ZL_LM_WG), 0, s, reqs, nreq, tables, records);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_limit_render(const ZlLmJob *jobs, int32_t njobs, int32_t wgs, const float *tables, const ZlLmRecord *records, const float *weights,
                           ZlLmStats *stats, uint32_t *verdicts, hipStream_t s)
{
    if (njobs <= 0 || wgs <= 0) return 0;
    hipLaunchKernelGGL(zl_k_limit_render, dim3((unsigned)wgs), dim3(ZL_LM_WG), 0, s, jobs, njobs, tables, records, weights, stats, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}
