// zl_loudness.hip -- the HIP kernel of the loudness measurement (zlhip_sound_loudness / _batch; the definition is in zl_loudness.h).
//
//   zl_k_loudness   the only pass.  A workgroup is one wavefront and takes ZL_LD_GROUP consecutive work items of the call, a lane per
//                   item (request, sub-block): the lane finds its request by bisection over the records' item_base, then walks its
//                   item's 16-byte groups of the arena's own layout with per-lane loads -- consecutive steps of a lane stay in one
//                   128-byte line for eight loads, which the CU's L1 serves -- four groups ahead of the arithmetic, and runs both
//                   channels' two-biquad chains in double.  There is no LDS and no barrier.  The loop runs to the wavefront's
//                   largest number of steps (zl_ld_group_steps) on every lane; a lane past its own end loads its last group again and
//                   does nothing with it.  Every record has one writer: plain stores, into host memory mapped into the device.
//
// A call is this one launch, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_loudness.h"

#define ZL_LD_AHEAD 4              // groups a lane loads ahead of its arithmetic

namespace {

typedef uint32_t zl_ld_u32x4 __attribute__((ext_vector_type(4)));
template <typename T> using ZlLdGlobal = const T __attribute__((address_space(1))) *;

// A lane's walk over its item: `steps` of the wavefront's `gsteps` steps, ZL_LD_AHEAD groups loaded ahead of the arithmetic.  The
// index of a load never passes the item's last group.  (In a wavefront that holds mono and stereo items the two walks run one behind
// the other, each to gsteps.)
template <int kChannels> __device__ __forceinline__ void zl_ld_walk(const double *c, const ZlLdItem &I, ZlLdGlobal<zl_ld_u32x4> src, int32_t steps, int32_t gsteps, ZlLdAcc &a)
{
    const int32_t last = I.steps - 1;                              // (>= 0: an item holds at least one frame)
    zl_ld_u32x4 q[ZL_LD_AHEAD];
#pragma unroll
    for (int u = 0; u < ZL_LD_AHEAD; ++u) q[u] = src[u < last ? u : last];
    for (int32_t n0 = 0; n0 < gsteps; n0 += ZL_LD_AHEAD) {
        zl_ld_u32x4 nx[ZL_LD_AHEAD];
#pragma unroll
        for (int u = 0; u < ZL_LD_AHEAD; ++u) { const int32_t m = n0 + ZL_LD_AHEAD + u; nx[u] = src[m < last ? m : last]; }
#pragma unroll
        for (int u = 0; u < ZL_LD_AHEAD; ++u) {
            const int32_t n = n0 + u;
            if (n < steps) zl_ld_step<kChannels>(c, I, n, q[u].x, q[u].y, q[u].z, q[u].w, a);
            q[u] = nx[u];
        }
    }
}

}  // namespace

__global__ void __launch_bounds__(ZL_LD_GROUP) zl_k_loudness(const ZlLdRequest *__restrict__ reqs, int32_t nreq, int32_t items, ZlLdSub *__restrict__ out)
{
    const int32_t item = (int32_t)blockIdx.x * ZL_LD_GROUP + (int32_t)threadIdx.x;
    const bool live = item < items;
    const ZlLdRequest *Rp = reqs + zl_ld_find(reqs, nreq, live ? item : items - 1);
    const int32_t channels = Rp->channels;
    ZlLdRequest R;                                                 // (the geometry only: the coefficients go to registers of their own)
    R.first = Rp->first; R.frames = Rp->frames; R.sub = Rp->sub; R.channels = channels; R.items = Rp->items; R.item_base = Rp->item_base;
    double c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = Rp->c[i];
    const ZlLdItem I = zl_ld_item(R, (live ? item : items - 1) - R.item_base);
    const int32_t steps = live ? I.steps : 0;
    // the wavefront's largest number of steps: zl_ld_group_steps(reqs, nreq, items, blockIdx.x)
    int32_t gsteps = steps;
#pragma unroll
    for (int d = 1; d < ZL_LD_GROUP; d <<= 1) { const int32_t o = __shfl_xor(gsteps, d, ZL_LD_GROUP); gsteps = o > gsteps ? o : gsteps; }
    gsteps = __builtin_amdgcn_readfirstlane(gsteps);

    const ZlLdGlobal<zl_ld_u32x4> src = (ZlLdGlobal<zl_ld_u32x4>)Rp->src + I.g0;
    const int32_t last = I.steps - 1;                              // (>= 0: an item holds at least one frame)
    ZlLdAcc a;
    zl_ld_acc_init(a);
    if (channels == 2) zl_ld_walk<2>(c, I, src, steps, gsteps, a); else zl_ld_walk<1>(c, I, src, steps, gsteps, a);
    if (live) {                                                    // field by field: a whole-record copy goes through the stack
        ZlLdSub *o = out + item;
        o->sum[0] = a.l.sum; o->sum[1] = a.r.sum;
        o->peak[0] = __uint_as_float(a.l.peak); o->peak[1] = __uint_as_float(a.r.peak);
    }
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_loudness(const ZlLdRequest *reqs, int32_t nreq, int32_t items, ZlLdSub *out, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(zl_k_loudness, dim3((unsigned)((items + ZL_LD_GROUP - 1) / ZL_LD_GROUP)), dim3(ZL_LD_GROUP), 0, s, reqs, nreq, items, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
