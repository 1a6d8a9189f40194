// zl_overview.hip -- HIP kernels of the waveform overviews (zlhip_sound_overview / _batch; the definition is in zl_overview.h).
//
//   zl_k_overview_reduce   every wavefront takes a run of consecutive ITEMS of the call (zl_overview.h): it finds the request of its
//                          first item by bisection over the requests' item_base, then walks.  A piece of a wide request: 16-byte
//                          loads of the arena's layout, one group per lane, samples taken as integers, head and tail masked by
//                          float index, DPP integer max over the wave, lane 0 writes (one piece per column) or combines by no-return
//                          atomic max (several).  64 columns of a narrow request: one lane per column over its few frames.
//   zl_k_overview_finish   one lane per column: the accumulated keys back to sample bits, in place.
//
// A call is these two launches behind one memset of the accumulators, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_overview.h"

#define ZL_OV_THREADS 256
#define ZL_OV_WAVES_PER_BLOCK (ZL_OV_THREADS / ZL_OV_WAVE)
#define ZL_OV_MAX_BLOCKS 4096          // 256 CUs x 16 workgroups: the grid stops growing there, the waves' runs get longer
#define ZL_OV_UNROLL 4                 // 16-byte loads a lane has in flight

namespace {

// Wavefront maximum of an unsigned value on the VALU (the DPP tree of zl_wave_max_nonneg, zl_kernels.hip): quad permutes, row_shr 4 and
// 8 leave each 16-lane row's result in its last lane, row_bcast 15 / 31 carry it across the rows; lanes without a source read 0, the
// identity.  The result of the whole wave is in lane 63.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t zl_ov_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xf, false); }
__device__ __forceinline__ uint32_t zl_ov_wave_umax(uint32_t v)
{
    uint32_t t;
    t = zl_ov_dpp<0xB1, 0xf>(v);  v = t > v ? t : v;               // quad_perm [1,0,3,2]
    t = zl_ov_dpp<0x4E, 0xf>(v);  v = t > v ? t : v;               // quad_perm [2,3,0,1]
    t = zl_ov_dpp<0x114, 0xf>(v); v = t > v ? t : v;               // row_shr 4
    t = zl_ov_dpp<0x118, 0xf>(v); v = t > v ? t : v;               // row_shr 8
    t = zl_ov_dpp<0x142, 0xa>(v); v = t > v ? t : v;               // row_bcast 15 -> rows 1, 3
    t = zl_ov_dpp<0x143, 0xc>(v); v = t > v ? t : v;               // row_bcast 31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// running max(key) and max(~key) of the four element positions of a 16-byte group (stereo: L R L R, mono: four frames)
struct ZlOvAcc {
    uint32_t hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
    __device__ __forceinline__ void take(int j, uint32_t bits, bool valid)
    {
        const uint32_t k = zl_ov_key(bits);
        const uint32_t a = valid ? k : 0u, b = valid ? ~k : 0u;
        hi[j] = a > hi[j] ? a : hi[j];
        lo[j] = b > lo[j] ? b : lo[j];
    }
};

__device__ __forceinline__ uint32_t umax2(uint32_t a, uint32_t b) { return a > b ? a : b; }

// an extent's address arrives as an integer in the request record: tell the compiler that it is global memory (global_load, not flat_load)
// (compiler vector types: they load from an address-space pointer as they are)
template <typename T> using ZlOvGlobal = const T __attribute__((address_space(1))) *;
typedef uint32_t zl_ov_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t zl_ov_u32x4 __attribute__((ext_vector_type(4)));

}  // namespace

__global__ void __launch_bounds__(ZL_OV_THREADS) zl_k_overview_reduce(const ZlOvRequest *__restrict__ reqs, int32_t nreq, int64_t items, uint32_t *__restrict__ acc)
{
    const int lane = threadIdx.x & (ZL_OV_WAVE - 1);
    const int64_t wave = (int64_t)blockIdx.x * ZL_OV_WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / ZL_OV_WAVE));
    const int64_t nwaves = (int64_t)gridDim.x * ZL_OV_WAVES_PER_BLOCK;
    // the wave's run of items: [wave * items / nwaves, (wave + 1) * items / nwaves), without the 64-bit product
    const int64_t q = items / nwaves, rem = items - q * nwaves;
    int64_t it = wave * q + (wave < rem ? wave : rem);
    const int64_t end = it + q + (wave < rem ? 1 : 0);
    if (it >= end) return;

    // the request of the first item: the last one whose item_base is <= it (item_base is non-decreasing, reqs[0].item_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= it) lo = mid; else hi = mid - 1;
    }
    ZlOvRequest R = reqs[r];
    for (; it < end; ++it) {
        while (r + 1 < nreq && reqs[r + 1].item_base <= it) R = reqs[++r];     // (requests hold at least one item each)
        const int64_t i = it - R.item_base;
        uint32_t *out = acc + 4 * (int64_t)R.col_base;
        if (R.ppc == 0) {
            // narrow: one lane per column, frame by frame (8-byte stereo frames, 4-byte mono frames)
            const int64_t c = i * ZL_OV_WAVE + lane;
            if (c < R.columns) {
                int64_t lo, hi;
                zl_ov_column(R.first, R.frames, R.columns, c, &lo, &hi);
                uint32_t hL = 0u, lL = 0u, hR = 0u, lR = 0u;
                if (R.channels == 2) {
                    const ZlOvGlobal<zl_ov_u32x2> src = (ZlOvGlobal<zl_ov_u32x2>)R.src;
                    for (int64_t f = lo; f < hi; ++f) {
                        const zl_ov_u32x2 v = src[f];
                        const uint32_t kl = zl_ov_key(v.x), kr = zl_ov_key(v.y);
                        hL = umax2(hL, kl); lL = umax2(lL, ~kl); hR = umax2(hR, kr); lR = umax2(lR, ~kr);
                    }
                } else {
                    const ZlOvGlobal<uint32_t> src = (ZlOvGlobal<uint32_t>)R.src;
                    for (int64_t f = lo; f < hi; ++f) {
                        const uint32_t k = zl_ov_key(src[f]);
                        hL = umax2(hL, k); lL = umax2(lL, ~k);
                    }
                    hR = hL; lR = lL;
                }
                *reinterpret_cast<uint4 *>(out + 4 * c) = make_uint4(lL, hL, lR, hR);     // the lane owns the column
            }
            continue;
        }
        // wide: one piece
        int32_t column; int64_t lo, hi, f0, f1, g0, g1;
        zl_ov_piece(R, i, &column, &lo, &hi);
        zl_ov_groups(lo, hi, R.channels, &f0, &f1, &g0, &g1);
        const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
        const ZlOvGlobal<zl_ov_u32x4> src = (ZlOvGlobal<zl_ov_u32x4>)R.src + g0;
        ZlOvAcc a;
        for (int32_t gb = 0; gb < ngroups; gb += ZL_OV_UNROLL * ZL_OV_WAVE) {
            zl_ov_u32x4 v[ZL_OV_UNROLL];
#pragma unroll
            for (int k = 0; k < ZL_OV_UNROLL; ++k) {
                v[k] = zl_ov_u32x4{0u, 0u, 0u, 0u};
                if (gb + k * ZL_OV_WAVE < ngroups) {               // (the same in every lane)
                    const int32_t g = gb + k * ZL_OV_WAVE + lane;
                    v[k] = src[g < ngroups ? g : ngroups - 1];     // lanes behind the piece read its last group again: a maximum does not mind
                }
            }
#pragma unroll
            for (int k = 0; k < ZL_OV_UNROLL; ++k) {
                if (gb + k * ZL_OV_WAVE < ngroups) {
                    int32_t g = gb + k * ZL_OV_WAVE + lane;
                    g = g < ngroups ? g : ngroups - 1;
                    a.take(0, v[k].x, zl_ov_valid(g, 0, head, count));
                    a.take(1, v[k].y, zl_ov_valid(g, 1, head, count));
                    a.take(2, v[k].z, zl_ov_valid(g, 2, head, count));
                    a.take(3, v[k].w, zl_ov_valid(g, 3, head, count));
                }
            }
        }
        uint32_t hL, lL, hR, lR;
        if (R.channels == 2) {
            hL = umax2(a.hi[0], a.hi[2]); lL = umax2(a.lo[0], a.lo[2]);
            hR = umax2(a.hi[1], a.hi[3]); lR = umax2(a.lo[1], a.lo[3]);
        } else {
            hL = umax2(umax2(a.hi[0], a.hi[1]), umax2(a.hi[2], a.hi[3]));
            lL = umax2(umax2(a.lo[0], a.lo[1]), umax2(a.lo[2], a.lo[3]));
            hR = hL; lR = lL;
        }
        hL = zl_ov_wave_umax(hL); lL = zl_ov_wave_umax(lL);
        if (R.channels == 2) { hR = zl_ov_wave_umax(hR); lR = zl_ov_wave_umax(lR); } else { hR = hL; lR = lL; }
        if (lane == 0) {
            uint32_t *o = out + 4 * (int64_t)column;
            if (R.ppc == 1) {
                *reinterpret_cast<uint4 *>(o) = make_uint4(lL, hL, lR, hR);     // the piece is the column
            } else {
                // the other pieces of the column arrive in any order: integer maxima commute
                atomicMax(o + 0, lL); atomicMax(o + 1, hL); atomicMax(o + 2, lR); atomicMax(o + 3, hR);
            }
        }
    }
}

__global__ void __launch_bounds__(ZL_OV_THREADS) zl_k_overview_finish(uint32_t *acc, int32_t columns)
{
    const int32_t c = (int32_t)(blockIdx.x * ZL_OV_THREADS + threadIdx.x);
    if (c >= columns) return;
    uint4 *p = reinterpret_cast<uint4 *>(acc) + c;
    const uint4 k = *p;                                            // max(~key), max(key) of L, then of R
    *p = make_uint4(zl_ov_unkey(~k.x), zl_ov_unkey(k.y), zl_ov_unkey(~k.z), zl_ov_unkey(k.w));
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_overview_reduce(const ZlOvRequest *reqs, int32_t nreq, int64_t items, uint32_t *acc, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    int64_t blocks = (items + ZL_OV_WAVES_PER_BLOCK - 1) / ZL_OV_WAVES_PER_BLOCK;
    if (blocks > ZL_OV_MAX_BLOCKS) blocks = ZL_OV_MAX_BLOCKS;
    hipLaunchKernelGGL(zl_k_overview_reduce, dim3((unsigned)blocks), dim3(ZL_OV_THREADS), 0, s, reqs, nreq, items, acc);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_overview_finish(uint32_t *acc, int32_t columns, hipStream_t s)
{
    if (columns <= 0) return 0;
    hipLaunchKernelGGL(zl_k_overview_finish, dim3((unsigned)((columns + ZL_OV_THREADS - 1) / ZL_OV_THREADS)), dim3(ZL_OV_THREADS), 0, s, acc, columns);
    ZL_LAUNCH_CHECK();
    return 0;
}
