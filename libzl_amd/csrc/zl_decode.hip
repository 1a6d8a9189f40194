// zl_decode.hip -- HIP kernels of the PCM upload (zlhip_sound_upload_pcm / _batch; the definition is in zl_decode.h).
//
//   zl_k_pcm_decode    one launch per staging pass.  Every wavefront takes a run of consecutive ITEMS of the pass (zl_decode.h): it finds
//                      the piece of its first item by bisection over the pieces' item_base, then walks.  An item is 64 consecutive
//                      16-byte groups of a piece's output, one per lane: the lane loads the group's samples from the stage (one or two
//                      aligned vector loads for sources of one or two channels), converts them (zl_dec_lane, the code the CPU tier
//                      walks) and writes the group with one 16-byte store -- a wave writes 1 KiB contiguous.  A clip's verdict on
//                      non-finite samples: OR over the wave, one atomic OR by one lane, only when something is set.
//   zl_k_pcm_publish   one lane per clip of the call: the sound-table entry, ZL_SOUND_FINITE from the clip's verdict word.
//
// No scratch memory, no LDS.
#include <hip/hip_runtime.h>
#include "zl_decode.h"

#define ZL_DEC_THREADS 256
#define ZL_DEC_WAVES_PER_BLOCK (ZL_DEC_THREADS / ZL_DEC_WAVE)
#define ZL_DEC_MAX_BLOCKS 4096         // 256 CUs x 16 workgroups: the grid stops growing there, the waves' runs get longer

namespace {

typedef uint32_t zl_dec_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t zl_dec_u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t zl_dec_u32x4 __attribute__((ext_vector_type(4)));
// an extent's address arrives as an integer in the piece record: tell the compiler that it is global memory (global_store, not flat_store)
typedef zl_dec_u32x4 __attribute__((address_space(1))) *ZlDecGlobalOut;

// the stage as zl_dec_lane reads it
struct ZlDecStage {
    const unsigned char *base;
    template <int N> __device__ __forceinline__ void dwords(uint32_t off, uint32_t *w) const
    {
        const unsigned char *p = base + off;
        if constexpr (N == 1) { w[0] = *reinterpret_cast<const uint32_t *>(p); }
        else if constexpr (N == 2) { const zl_dec_u32x2 v = *reinterpret_cast<const zl_dec_u32x2 *>(p); w[0] = v.x; w[1] = v.y; }
        else if constexpr (N == 3) {
            // 12 bytes at a 4-byte-aligned offset (three dwords: a 16-byte load would read into the next clip's bytes)
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
            w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
        }
        else { const zl_dec_u32x4 v = *reinterpret_cast<const zl_dec_u32x4 *>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    }
    __device__ __forceinline__ uint32_t byte(uint32_t off) const { return base[off]; }
};

}  // namespace

__global__ void __launch_bounds__(ZL_DEC_THREADS) zl_k_pcm_decode(const ZlDecPiece *__restrict__ pieces, int32_t npieces, int32_t items,
                                                                   const unsigned char *__restrict__ stage, uint32_t *__restrict__ verdicts)
{
    const int lane = threadIdx.x & (ZL_DEC_WAVE - 1);
    const int32_t wave = (int32_t)blockIdx.x * ZL_DEC_WAVES_PER_BLOCK + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / ZL_DEC_WAVE));
    const int32_t nwaves = (int32_t)gridDim.x * ZL_DEC_WAVES_PER_BLOCK;
    // the wave's run of items: [wave * items / nwaves, (wave + 1) * items / nwaves), without the product
    const int32_t q = items / nwaves, rem = items - q * nwaves;
    int32_t it = wave * q + (wave < rem ? wave : rem);
    const int32_t end = it + q + (wave < rem ? 1 : 0);
    if (it >= end) return;

    // the piece of the first item: the last one whose item_base is <= it (item_base is non-decreasing, pieces[0].item_base == 0)
    int32_t r = 0;
    for (int32_t lo = 0, hi = npieces - 1; ; ) {
        if (lo >= hi) { r = lo; break; }
        const int32_t mid = (lo + hi + 1) >> 1;
        if (pieces[mid].item_base <= it) lo = mid; else hi = mid - 1;
    }
    ZlDecPiece R = pieces[r];
    int32_t ngroups = (int32_t)zl_dec_piece_groups(R);
    const ZlDecStage S = { stage };
    for (; it < end; ++it) {
        while (r + 1 < npieces && pieces[r + 1].item_base <= it) { R = pieces[++r]; ngroups = (int32_t)zl_dec_piece_groups(R); }   // (pieces hold at least one item each)
        const int32_t g = (it - R.item_base) * ZL_DEC_WAVE + lane;
        uint32_t bad = 0u;
        if (g < ngroups) {
            uint32_t o[4];
            bad = zl_dec_lane(R, g, S, o);
            const ZlDecGlobalOut dst = (ZlDecGlobalOut)(R.dst + 4ull * (uint64_t)zl_dec_group_float(R, g));
            *dst = zl_dec_u32x4{o[0], o[1], o[2], o[3]};
        }
        if (zl_dec_is_float(R.format)) {                           // (the same in every lane)
            const bool any = __builtin_amdgcn_ballot_w64(bad != 0u) != 0ull;
            if (any && lane == 0) atomicOr(verdicts + R.verdict, 1u);
        }
    }
}

__global__ void __launch_bounds__(ZL_DEC_THREADS) zl_k_pcm_publish(const ZlDecPublish *__restrict__ recs, int32_t n, const uint32_t *__restrict__ verdicts, ZlSound *table)
{
    const int32_t i = (int32_t)(blockIdx.x * ZL_DEC_THREADS + threadIdx.x);
    if (i >= n) return;
    ZlDecPublish p = recs[i];
    if (!p.check || verdicts[i] == 0u) p.s.flags |= ZL_SOUND_FINITE;
    table[p.id] = p.s;
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_pcm_decode(const ZlDecPiece *pieces, int32_t npieces, int32_t items, const void *stage, uint32_t *verdicts, hipStream_t s)
{
    if (npieces <= 0 || items <= 0) return 0;
    int32_t blocks = (items + ZL_DEC_WAVES_PER_BLOCK - 1) / ZL_DEC_WAVES_PER_BLOCK;
    if (blocks > ZL_DEC_MAX_BLOCKS) blocks = ZL_DEC_MAX_BLOCKS;
    hipLaunchKernelGGL(zl_k_pcm_decode, dim3((unsigned)blocks), dim3(ZL_DEC_THREADS), 0, s, pieces, npieces, items, (const unsigned char *)stage, verdicts);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_pcm_publish(const ZlDecPublish *recs, int32_t n, const uint32_t *verdicts, ZlSound *table, hipStream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(zl_k_pcm_publish, dim3((unsigned)((n + ZL_DEC_THREADS - 1) / ZL_DEC_THREADS)), dim3(ZL_DEC_THREADS), 0, s, recs, n, verdicts, table);
    ZL_LAUNCH_CHECK();
    return 0;
}
