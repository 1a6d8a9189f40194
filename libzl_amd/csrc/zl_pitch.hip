// zl_pitch.hip -- HIP kernels of the pitch detection (zlhip_sound_pitch / _batch; the definition is in zl_pitch.h).
//
//   zl_k_pitch_diff     the hot path and the only pass that reads the clip.  A workgroup takes one work item (request, frame, tile of
//                       256 lags) and finds its request by bisection over the records' item_base.  It reads the frame's L samples in
//                       16-byte groups of the arena's own layout, head and tail masked by float index, mixes and quantises them, and
//                       reduces max |m| and the window's energy as integers; a second pass over the same groups (they are in the
//                       cache now) stages x = m >> sh in LDS as int16 (at most 12 KB).  Then a lane owns one lag: x[j] is a
//                       broadcast read of eight samples, x[j + t] is consecutive across the lanes; the squared differences are summed
//                       in 32 bits for 32 terms, then added to a 64-bit accumulator.  Every d[t] has one writer: a plain store.
//                       Tile 0 also stores the frame's energy verdict and shift.
//   zl_k_pitch_pick     one workgroup per frame: the prefix sum C (eight lags per lane, a scan over the lanes' sums), the first lag
//                       below the threshold and the end of the descent as two min-reductions, the frame's record.
//   zl_k_pitch_vote     one workgroup per request, a lane per frame: a histogram of the lags in LDS, scanned by the whole workgroup
//                       for the lower median, the consistent frames counted, the representative as a max-reduction over
//                       (clarity, -frame); one lane writes the integer record into host memory mapped into the device.
//
// A call is these three launches, whatever the number of requests.
#include <hip/hip_runtime.h>
#include "zl_pitch.h"

#define ZL_PT_THREADS 256
#define ZL_PT_WAVE 64
#define ZL_PT_WAVES_PER_BLOCK (ZL_PT_THREADS / ZL_PT_WAVE)
#define ZL_PT_PER_LANE (ZL_PT_MAX_LAGS / ZL_PT_THREADS)           // lags (pick) and histogram bins (vote) of a lane

static_assert(ZL_PT_THREADS == ZL_PT_TILE, "one lane per lag of the tile");
static_assert(ZL_PT_THREADS == ZL_PT_MAX_FRAMES, "one lane per frame in the vote");
static_assert(ZL_PT_WINDOW_MIN % ZL_PT_CHUNK == 0 && 64 % ZL_PT_CHUNK == 0, "a window is a whole number of chunks");

namespace {

template <typename T> using ZlPtGlobal = const T __attribute__((address_space(1))) *;
typedef float zl_pt_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t zl_pt_shfl_xor(uint64_t v, int d) { return (uint64_t)__shfl_xor((unsigned long long)v, d, ZL_PT_WAVE); }

enum { ZL_PT_SUM, ZL_PT_MAX, ZL_PT_MIN };

// the sum / maximum / minimum over the workgroup, in every thread.  sRed: ZL_PT_WAVES_PER_BLOCK words of LDS
template <int kOp> __device__ __forceinline__ uint64_t zl_pt_op(uint64_t a, uint64_t b) { return kOp == ZL_PT_SUM ? a + b : (kOp == ZL_PT_MAX ? (a > b ? a : b) : (a < b ? a : b)); }
template <int kOp> __device__ __forceinline__ uint64_t zl_pt_block_reduce(uint64_t v, uint64_t *sRed)
{
#pragma unroll
    for (int d = 1; d < ZL_PT_WAVE; d <<= 1) v = zl_pt_op<kOp>(v, zl_pt_shfl_xor(v, d));
    __syncthreads();                                               // (sRed's last readers are done)
    if ((threadIdx.x & (ZL_PT_WAVE - 1)) == 0) sRed[threadIdx.x / ZL_PT_WAVE] = v;
    __syncthreads();
    uint64_t r = sRed[0];
#pragma unroll
    for (int w = 1; w < ZL_PT_WAVES_PER_BLOCK; ++w) r = zl_pt_op<kOp>(r, sRed[w]);
    return r;
}

// exclusive prefix sum over the workgroup's threads.  sRed: ZL_PT_WAVES_PER_BLOCK words of LDS
__device__ __forceinline__ uint64_t zl_pt_block_scan(uint64_t v, uint64_t *sRed)
{
    const int lane = threadIdx.x & (ZL_PT_WAVE - 1), wave = threadIdx.x / ZL_PT_WAVE;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < ZL_PT_WAVE; d <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)inc, d, ZL_PT_WAVE);
        if (lane >= d) inc += t;
    }
    __syncthreads();
    if (lane == ZL_PT_WAVE - 1) sRed[wave] = inc;
    __syncthreads();
    uint64_t base = 0;
#pragma unroll
    for (int w = 0; w < ZL_PT_WAVES_PER_BLOCK; ++w) if (w < wave) base += sRed[w];
    return base + inc - v;
}

// the request of item / frame `at`: the last one whose base is <= at (the bases do not decrease; a request without frames shares its
// base with the next one, which is then the one found)
template <bool kItems> __device__ __forceinline__ int32_t zl_pt_find(const ZlPtRequest *__restrict__ reqs, int32_t nreq, int32_t at)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((kItems ? reqs[mid].item_base : reqs[mid].frame_base) <= at) lo = mid; else hi = mid - 1;
    }
}

}  // namespace

__global__ void __launch_bounds__(ZL_PT_THREADS) zl_k_pitch_diff(const ZlPtRequest *__restrict__ reqs, int32_t nreq, uint64_t *__restrict__ Dall, ZlPtStat *__restrict__ stat)
{
    __shared__ __attribute__((aligned(16))) int16_t sX[ZL_PT_MAX_SPAN];
    __shared__ uint64_t sRed[ZL_PT_WAVES_PER_BLOCK];
    const int32_t item = (int32_t)blockIdx.x;
    const ZlPtRequest R = reqs[zl_pt_find<true>(reqs, nreq, item)];
    int32_t frame, tile;
    zl_pt_item_of(R, item - R.item_base, &frame, &tile);
    const int tid = threadIdx.x;
    const int32_t L = zl_pt_span(R), W = R.window;
    const int64_t s0 = zl_pt_frame_start(R, frame);
    int64_t f0, f1, g0, g1;
    zl_ov_groups(s0, s0 + L, R.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const ZlPtGlobal<zl_pt_f32x4> src = (ZlPtGlobal<zl_pt_f32x4>)R.src + g0;

    // pass 1: the largest |m| of the span and the energy of the window
    uint32_t amax = 0; uint64_t energy = 0;
    for (int32_t g = tid; g < ngroups; g += ZL_PT_THREADS) {
        const zl_pt_f32x4 v = src[g];
        int32_t m[4], idx[4];
        zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = (uint32_t)(m[j] < 0 ? -m[j] : m[j]);                  // (0 where the slot holds nothing)
            amax = a > amax ? a : amax;
            if (idx[j] >= 0 && idx[j] < W) energy += (uint64_t)a * a;
        }
    }
    amax = (uint32_t)zl_pt_block_reduce<ZL_PT_MAX>(amax, sRed);
    energy = zl_pt_block_reduce<ZL_PT_SUM>(energy, sRed);
    const int32_t shift = zl_pt_shift(amax);
    if (tile == 0 && tid == 0) { ZlPtStat st; st.energy = energy; st.shift = shift; st.silent = energy < R.floor_ ? 1 : 0; stat[R.frame_base + frame] = st; }

    // pass 2: x = m >> shift into LDS
    for (int32_t g = tid; g < ngroups; g += ZL_PT_THREADS) {
        const zl_pt_f32x4 v = src[g];
        int32_t m[4], idx[4];
        zl_pt_group_mix(v.x, v.y, v.z, v.w, g, head, count, R.channels, m, idx);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (idx[j] >= 0) sX[idx[j]] = (int16_t)(m[j] >> shift);         // idx < L <= ZL_PT_MAX_SPAN
    }
    __syncthreads();

    // the lags: lane `tid` sums d[t] over the window, t + j <= t_max + 1 + W - 1 = L - 1
    const int32_t t = zl_pt_lane_lag(R, tile, tid);
    const int16_t *lagged = sX + t;
    uint64_t acc = 0;
    for (int32_t j0 = 0; j0 < W; j0 += ZL_PT_CHUNK) {
        uint32_t part = 0;
#pragma unroll
        for (int u = 0; u < ZL_PT_CHUNK; u += 8) {
            const uint4 hv = *(const uint4 *)(sX + j0 + u);        // eight x[j], the same address in every lane
            const uint32_t hw[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int32_t a = (int32_t)(int16_t)((k & 1) ? hw[k >> 1] >> 16 : hw[k >> 1] & 0xffffu);
                const int32_t df = a - (int32_t)lagged[j0 + u + k];
                part += (uint32_t)(df * df);
            }
        }
        acc += part;
    }
    if (zl_pt_lane_live(R, tile, tid)) Dall[R.d_base + (int64_t)frame * zl_pt_nd(R) + (t - 1)] = acc;
}

__global__ void __launch_bounds__(ZL_PT_THREADS) zl_k_pitch_pick(const ZlPtRequest *__restrict__ reqs, int32_t nreq, const uint64_t *__restrict__ Dall,
                                                                 const ZlPtStat *__restrict__ stat, ZlPtFrame *__restrict__ out)
{
    __shared__ uint64_t sD[ZL_PT_MAX_LAGS];                        // d[t] at word t - 1
    __shared__ uint64_t sC[ZL_PT_MAX_LAGS];
    __shared__ uint64_t sRed[ZL_PT_WAVES_PER_BLOCK];
    const int32_t f = (int32_t)blockIdx.x;
    const ZlPtRequest R = reqs[zl_pt_find<false>(reqs, nreq, f)];
    const ZlPtStat st = stat[f];
    const int tid = threadIdx.x;
    const int32_t nd = zl_pt_nd(R);
    const uint64_t *d = Dall + R.d_base + (int64_t)(f - R.frame_base) * nd;
    // the lane's lags are consecutive: words [8 tid, 8 tid + 8)
    uint64_t own = 0;
#pragma unroll
    for (int k = 0; k < ZL_PT_PER_LANE; ++k) {
        const int32_t i = tid * ZL_PT_PER_LANE + k;
        const uint64_t v = i < nd ? d[i] : 0;
        if (i < nd) sD[i] = v;
        own += v;
    }
    uint64_t run = zl_pt_block_scan(own, sRed);
    const uint64_t none = (uint64_t)ZL_PT_MAX_LAGS;
    uint64_t first = none;
#pragma unroll
    for (int k = 0; k < ZL_PT_PER_LANE; ++k) {
        const int32_t i = tid * ZL_PT_PER_LANE + k, t = i + 1;
        if (i < nd) {
            run += sD[i];
            sC[i] = run;
            if (first == none && t >= R.tmin && t <= R.tmax && zl_pt_below(sD[i], t, R.threshold, run)) first = (uint64_t)t;
        }
    }
    const int32_t t0 = (int32_t)zl_pt_block_reduce<ZL_PT_MIN>(first, sRed);           // (the barriers inside also publish sD and sC)
    uint64_t stop = none;
    if (t0 < ZL_PT_MAX_LAGS) {
#pragma unroll
        for (int k = 0; k < ZL_PT_PER_LANE; ++k) {
            const int32_t t = tid * ZL_PT_PER_LANE + k + 1;
            if (stop == none && t >= t0 && t <= R.tmax && zl_pt_stops(sD[t - 1], sD[t], t, R.tmax)) stop = (uint64_t)t;      // sD[t]: d[t + 1], t + 1 <= nd
        }
    }
    const int32_t lag = (int32_t)zl_pt_block_reduce<ZL_PT_MIN>(stop, sRed);
    if (tid == 0) {
        const int32_t tk = st.silent || lag >= ZL_PT_MAX_LAGS ? 0 : lag;
        zl_pt_frame_record(st, sD, tk > 0 ? sC[tk - 1] : 0, tk, &out[f]);
    }
}

__global__ void __launch_bounds__(ZL_PT_THREADS) zl_k_pitch_vote(const ZlPtRequest *__restrict__ reqs, const ZlPtFrame *__restrict__ frames, ZlPtResult *__restrict__ out)
{
    __shared__ uint32_t sHist[ZL_PT_MAX_LAGS];
    __shared__ uint64_t sRed[ZL_PT_WAVES_PER_BLOCK];
    const ZlPtRequest R = reqs[blockIdx.x];
    const int tid = threadIdx.x;
    const ZlPtFrame *F = frames + R.frame_base;
    for (int32_t i = tid; i < ZL_PT_MAX_LAGS; i += ZL_PT_THREADS) sHist[i] = 0;
    __syncthreads();
    const bool mine = tid < R.frames;                              // a lane per frame: K <= ZL_PT_MAX_FRAMES
    const int32_t lag = mine ? F[tid].lag : 0, clarity = mine ? F[tid].clarity : 0;
    if (lag > 0) (void)atomicAdd(&sHist[lag], 1u);                 // lag <= t_max < ZL_PT_MAX_LAGS
    const int32_t V = (int32_t)zl_pt_block_reduce<ZL_PT_SUM>(lag > 0 ? 1u : 0u, sRed);             // (its barriers publish the histogram)
    // the lower median: the first bin at which the running count passes (V - 1) / 2
    uint64_t own = 0;
#pragma unroll
    for (int k = 0; k < ZL_PT_PER_LANE; ++k) own += sHist[tid * ZL_PT_PER_LANE + k];
    uint64_t run = zl_pt_block_scan(own, sRed);
    const uint64_t none = (uint64_t)ZL_PT_MAX_LAGS, rank = (uint64_t)((V > 0 ? V - 1 : 0) / 2);
    uint64_t bin = none;
#pragma unroll
    for (int k = 0; k < ZL_PT_PER_LANE; ++k) {
        run += sHist[tid * ZL_PT_PER_LANE + k];
        if (bin == none && V > 0 && run > rank) bin = (uint64_t)(tid * ZL_PT_PER_LANE + k);
    }
    const int32_t med = (int32_t)zl_pt_block_reduce<ZL_PT_MIN>(bin, sRed);
    const bool cons = lag > 0 && zl_pt_consistent(lag, med);
    const int32_t consistent = (int32_t)zl_pt_block_reduce<ZL_PT_SUM>(cons ? 1u : 0u, sRed);
    // the representative: the largest key; the keys are offset into unsigned order
    const uint64_t bias = (uint64_t)1 << 63;
    const uint64_t key = cons ? (uint64_t)zl_pt_key(clarity, tid) + bias : 0;
    const uint64_t best = zl_pt_block_reduce<ZL_PT_MAX>(key, sRed);
    if (tid == 0) {
        const int32_t rep = best == 0 ? -1 : 65535 - (int32_t)((best - bias) & 0xffffu);
        zl_pt_result(R.frames, V, consistent, rep, F, &out[blockIdx.x]);
    }
}

#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_pitch_diff(const ZlPtRequest *reqs, int32_t nreq, int64_t items, uint64_t *D, ZlPtStat *stat, hipStream_t s)
{
    if (nreq <= 0 || items <= 0) return 0;
    hipLaunchKernelGGL(zl_k_pitch_diff, dim3((unsigned)items), dim3(ZL_PT_THREADS), 0, s, reqs, nreq, D, stat);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_pitch_pick(const ZlPtRequest *reqs, int32_t nreq, int64_t frames, const uint64_t *D, const ZlPtStat *stat, ZlPtFrame *out, hipStream_t s)
{
    if (nreq <= 0 || frames <= 0) return 0;
    hipLaunchKernelGGL(zl_k_pitch_pick, dim3((unsigned)frames), dim3(ZL_PT_THREADS), 0, s, reqs, nreq, D, stat, out);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_pitch_vote(const ZlPtRequest *reqs, int32_t nreq, const ZlPtFrame *frames, ZlPtResult *out, hipStream_t s)
{
    if (nreq <= 0) return 0;
    hipLaunchKernelGGL(zl_k_pitch_vote, dim3((unsigned)nreq), dim3(ZL_PT_THREADS), 0, s, reqs, frames, out);
    ZL_LAUNCH_CHECK();
    return 0;
}
