// zl_kernels.hip -- HIP kernels of the sampler engine, written for gfx950 (CDNA4, wave64).
//
//   K0 zl_k0_apply_ops   device half of SamplerChannel::handleCommand (SamplerSynth.cpp:187-230)
//   K1 zl_k1_plan        per-voice control plan of SamplerSynthVoice::process (:174-270), zl_plan.h
//   K1c zl_k1c_assemble  segment streams -> per-block plan records, multi-segment blocks -> per-frame control
//                        (lane-parallel)
//   K1o zl_k1o_order     K2's block order sorted by loop phase (zl_order.h)
//   K2 zl_k2_render      gather + interpolate + gain/ADSR/pan + voice->bus sum (:198-221,
//                        SamplerSynth.cpp:134-140); HBM-bound, no MFMA (about 22 flop per 8 bytes)
//   K3 zl_k3_finalize    ordered sum of mix-group partials + AudioLevels block scan
//                        (AudioLevels.cpp:361-383) + report finalisation (:265-267)
//   zl_k_levels_tick     AudioLevels decay / hold tick (AudioLevels.cpp:359-360,395-396)
//   zl_k_passthrough     JackPassthrough fan-out (JackPassthrough.cpp:55-113)
//   zl_k_interleave      planar -> interleaved source upload (SamplerSynthSound.cpp:45-47 layout choice)
//
// Build: hipcc --offload-arch=gfx950 -ffp-contract=off (the oracle defines an un-fused rounding
// sequence; see zl_render.h).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstddef>
#include "zl_types.h"
#include "zl_plan.h"
#include "zl_render.h"
#include "zl_order.h"
#include "zl_pair.h"
#include "zl_kernels.h"

// ------------------------------------------------------------------------------------------------
// One clip-parameter edit (zlhip_clip_set) -> the HBM clip table, by the 64 lanes of a wave, word by word.  The record sits in
// mapped host memory; the table is read by the planner at the start of the plan window that follows (zl_plan.h, begin).
static __device__ __forceinline__ void zl_apply_clip_edit(const ZlBatch &A, const ZlClipEdit *ed, int lane)
{
    static_assert(offsetof(ZlClip, slice_pos) == ZL_CLIP_HEAD_BYTES && sizeof(ZlClip) % 16 == 0 && offsetof(ZlClipEdit, c) % 16 == 0, "clip record layout");
    const int clip = ed->clip;
    const int n16 = ed->full ? (int)(sizeof(ZlClip) / 16) : ZL_CLIP_HEAD_BYTES / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(&ed->c);
    uint4 *dst = reinterpret_cast<uint4 *>(const_cast<ZlClip *>(A.clips) + clip);
    for (int w = lane; w < n16; w += 64) dst[w] = src[w];
}

// workgroups [0, ceil(n_op_ranges / 64)): one lane per voice with operations; the following n_clip_edits workgroups: one edit each
__global__ void zl_k0_apply_ops(const ZlBatch A)
{
    const int opGroups = (A.n_op_ranges + 63) / 64;
    if ((int)blockIdx.x >= opGroups) {
        zl_apply_clip_edit(A, A.clip_edits + ((int)blockIdx.x - opGroups), (int)threadIdx.x);
        return;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_op_ranges) return;
    const ZlOpRange rg = A.op_ranges[i];
    ZlVoiceState st = A.voices[rg.voice];
    for (int j = 0; j < rg.count; ++j) zl_apply_op(st, A.ops[rg.first + j]);
    A.voices[rg.voice] = st;
}

// ------------------------------------------------------------------------------------------------
// K1c body for one wave: block k of the wave's 64 voices (one lane each).  Blocks with more than two position
// segments are expanded into per-frame control by the whole wave, lanes over frames.
static __device__ __forceinline__ void zl_k1c_block(const ZlBatch &A, ZlAssembler &as, int v, int lane, int k, ZlBlockPlan *rec = nullptr)
{
    int idx0 = 0, base0 = 0, n_active = 0;
    const int nseg = as.block(A, k, idx0, base0, n_active, rec);
    unsigned long long m = __ballot(nseg > 2);
    while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const int vv = __shfl(v, l, 64), ii = __shfl(idx0, l, 64), bb = __shfl(base0, l, 64), na = __shfl(n_active, l, 64);
        // a slot of the window's control pool for this (block, voice); none left: the block is marked and K2 recomputes it
        int slot = 0;
        if (lane == 0) slot = zl_expand_slot(A, (size_t)k * A.V + vv, ii, bb);
        slot = __shfl(slot, 0, 64);
        if (slot < 0) continue;
        ZlSegStream ss;
        ss.init(A, vv, A.runs[vv]);
        const size_t base = (size_t)slot * (size_t)A.N;
        for (int f = lane; f < A.N; f += 64) {
            float env;
            A.ctl_P[base + f] = zl_expand_frame(ss, A.N, k, ii, bb, f < na ? f : 0, env);
            A.ctl_env[base + f] = env;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K1: one lane per voice; the block clocks are staged in LDS so the per-block step of the planner
// makes no dependent global load.  Cost is O(linear runs + events) per voice, not O(blocks) (zl_plan.h).
#define ZL_K1_CLOCKS 256     // (12 KB of LDS: a planner workgroup must fit next to the render kernel's workgroups on a CU -- with 1024 clocks it did not)
__global__ void __launch_bounds__(64) zl_k1_plan(const ZlBatch A, int force_slow)
{
    __shared__ ZlClock s_clk[ZL_K1_CLOCKS];
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = v < A.V;
    ZlPlanner pl;
    if (mine) pl.begin(A, v, force_slow);
    // Only beat-locked loops test the block clocks as they go (:227-241).  A wave without one plans its whole window in one sweep
    // with the clocks where they are, in global memory -- they are read at a voice's first block and in simulated blocks only --
    // instead of stage by stage: an iteration ends at the end of the staged clocks, and a window of 8192 64-frame blocks would cut
    // every run into 8 (planning 96 voices: 0.21 -> 0.0x ms per window).
    const bool needClocks = mine && pl.valid && pl.st.playing && pl.clockMode;
    if (!A.inline_clock && __ballot(needClocks) == 0ull) {
        if (mine) while (pl.t < A.K * A.N) pl.iterate(A, A.K, A.clocks, 0, force_slow);
    } else
    for (int kb = 0; kb < A.K; kb += ZL_K1_CLOCKS) {
        const int nk = (A.K - kb < ZL_K1_CLOCKS) ? A.K - kb : ZL_K1_CLOCKS;
        // every voice of this wave has reached the end of the window (idle, stopped, or a periodic loop whose remaining
        // passes are implied): the rest of the clocks is not needed.  (The workgroup is one wavefront; written as a
        // skipped body rather than a break, which crashes the register allocator of this compiler.)
        const bool lane_done = !mine || !(pl.valid && pl.st.playing) || pl.t >= A.K * A.N;
        if (__ballot(!lane_done) != 0ull) {
            __syncthreads();
            if (A.inline_clock) {
                if (threadIdx.x == 0) s_clk[0] = A.clock0;         // a single real-time block: no clock upload
            } else {
                const uint4 *g = reinterpret_cast<const uint4 *>(A.clocks + kb);
                uint4 *sh = reinterpret_cast<uint4 *>(s_clk);
                for (int i = threadIdx.x; i < nk * (int)(sizeof(ZlClock) / 16); i += blockDim.x) sh[i] = g[i];
            }
            __syncthreads();
            if (mine) {
                // idle voices leave at once (ZlRunList::dead_from); the others run the planner's state machine, whose
                // iterations are the same straight-line code for every lane (zl_plan.h)
                while (pl.t < (kb + nk) * A.N) pl.iterate(A, kb + nk, s_clk, kb, force_slow);
            }
        }
    }
    if (mine) {
        pl.end(A);
        if (A.stats) {
            if (pl.stats.source_bytes)  atomicAdd(&A.stats->source_bytes, pl.stats.source_bytes);
            if (pl.stats.slow_blocks)   atomicAdd(&A.stats->slow_blocks, pl.stats.slow_blocks);
            if (pl.stats.active_frames) atomicAdd(&A.stats->active_frames, pl.stats.active_frames);
        }
    }
    if (A.fuse_assemble) {
        // a single block: K1c's work for the wave's voices is done here (their records were written by this wave)
        __threadfence();
        ZlAssembler as;
        as.begin(A, mine ? v : 0, 0, mine ? A.K : 0);
        for (int k = 0; k < A.K; ++k) zl_k1c_block(A, as, v, threadIdx.x, k);
    }
}

// K1c: segment streams -> per-block plan records.  One lane per voice (coalesced 16-byte plan stores across the
// wave), ZL_K1C_BLOCKS consecutive blocks per wave (one binary search per lane, then a forward walk).  Blocks with
// more than two position segments (the block after a loop restart at a small position crosses ~log2(N) binades)
// are expanded into per-frame control by the whole wave, lanes over frames, so that K2 keeps one pipelined path.
#define ZL_K1C_BLOCKS 8
// Few voices = few waves, each walking its blocks one after the other: engines with fewer than 512 voices give a lane 2
// blocks instead of 8 (four times the waves, a quarter of the latency; the kernel is hidden behind K2 only if it is short)
static inline int zl_k1c_blocks_per_lane(const ZlBatch &A) { return A.V >= 512 ? ZL_K1C_BLOCKS : 2; }
__global__ void __launch_bounds__(64) zl_k1c_assemble(const ZlBatch A, int blocks_per_lane)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x;
    const bool mine = v < A.V;
    const int kbeg = blockIdx.y * blocks_per_lane;
    const int kend = kbeg + blocks_per_lane < A.K ? kbeg + blocks_per_lane : A.K;
    ZlAssembler as;
    as.begin(A, mine ? v : 0, kbeg, mine ? kend : kbeg);
    if (!(A.ongrid & ZL_ONGRID_SCALAR)) {
        for (int k = kbeg; k < kend; ++k) zl_k1c_block(A, as, v, lane, k);
        return;
    }
    // A window whose launch is zl_k2_pair_phase_render with ZL_K2_PAIR_SCALAR on: the scalar records (zl_render.h).  The lane holds the
    // voice-block's plan as it stores it; the class is the text the pair kernels' staging reads (zl_voice_block_class, mode 0), so a
    // chunk's bit is set exactly where staging would class it (cc & 132) == 132.  Every (block, voice) of the window gets its word and
    // every (block, group) its 16 bits, the blocks without a record of K1c's included: nothing of an earlier window is left to read.
    const ZlVoiceConst vc = A.vconst[mine ? v : 0];
    uint64_t *tab = zl_batch_pair_tab(A);
    uint16_t *bits = reinterpret_cast<uint16_t *>(tab + zl_pair_tab_fast(A.K, A.V));
    const int G = (A.V + 63) / 64;
    if (mine && kbeg == 0) tab[zl_pair_tab_pan(A.K, A.V) + (size_t)v] = *reinterpret_cast<const uint64_t *>(&vc.lpan);
    for (int k = kbeg; k < kend; ++k) {
        ZlBlockPlan pl;
        zl_k1c_block(A, as, v, lane, k, &pl);
        const int cls = zl_voice_block_class(0u, A.ongrid, A.trace, A.N, vc, pl);
        const bool fast = mine && zl_voice_block_fast(cls);
        if (mine) tab[(size_t)k * A.V + (size_t)v] = fast ? zl_ongrid_addr0((uint64_t)reinterpret_cast<uintptr_t>(A.arena), vc.src_offset, pl.P0, (cls & 16) != 0) : 0ull;
        const unsigned long long mf = __ballot(fast), mm = __ballot(fast && (cls & 16));
        if (lane == 0) bits[(size_t)k * G + blockIdx.x] = (uint16_t)zl_pair_fast_bits(mf, mm);
    }
}

// K1o: K2's launch order of the window's blocks, sorted by the loop phase of each z-slot's key voice (zl_order.h).  One
// workgroup per z-slot: a counting sort over at most ZL_ORDER_MAXBKT buckets in LDS.  It runs beside a rendering K2 (the
// planner's free wave slot, 9 KB of LDS), so it is small: 4 waves of at most 96 registers, 34 us at 8192 blocks.  Then each
// bucket's segment is put in the order of the exact phase (below).  Without a key voice, or when the window is no longer than
// the key voice's pass, the slot's order is the identity.
// a segment of n <= M packed words (zl_order_pack: non-negative as ints), sorted ascending in registers by a bitonic network and stored as their
// low 16 bits; the slots past n hold INT_MAX and stay behind
template <int M>
static __device__ __forceinline__ void zl_k1o_sort_segment(int32_t *seg, int n)
{
    int w[M];
#pragma unroll
    for (int i = 0; i < M; ++i) w[i] = i < n ? seg[i] : INT_MAX;
#pragma unroll
    for (int size = 2; size <= M; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const int j = i ^ stride;
                if (j > i) {
                    const int lo = w[i] < w[j] ? w[i] : w[j], hi = w[i] < w[j] ? w[j] : w[i];
                    const bool up = (i & size) == 0;
                    w[i] = up ? lo : hi; w[j] = up ? hi : lo;
                }
            }
#pragma unroll
    for (int i = 0; i < M; ++i) if (i < n) seg[i] = w[i] & 0xffff;
}

__global__ void __launch_bounds__(256) zl_k1o_order(const ZlBatch A, int32_t *order, int norun)
{
    __shared__ int s_hist[ZL_ORDER_MAXBKT];
    __shared__ int s_part[256];
    __shared__ int s_key, s_end;
    const int tid = threadIdx.x, K = A.K;
    int vb, ve;
    zl_order_slot_voices((int)blockIdx.x, A.NB, A.VPB, A.V, vb, ve);
    int32_t *out = order + (size_t)blockIdx.x * K;
    if (tid == 0) { s_key = INT_MAX; s_end = 0; }
    __syncthreads();
    // the same pass over the slot's run lists leaves the tail behind the table (zl_order.h): the slot's run_end -- INT_MAX with
    // ZL_K2_STAGE_NORUN=0: staging then fetches the run lists in every block -- and each voice's dead_from, dense
    for (int v = vb + tid; v < ve; v += 256) {
        if (zl_order_is_key(A.runs[v], K)) atomicMin(&s_key, v);
        const int e = zl_order_run_end(A.runs[v]);
        if (e > 0) atomicMax(&s_end, e);
        order[zl_order_tail_dead((int)gridDim.x, K, v)] = A.runs[v].dead_from;
    }
    __syncthreads();
    if (tid == 0) order[zl_order_tail_run_end((int)gridDim.x, K, (int)blockIdx.x)] = norun ? s_end : INT_MAX;
    ZlOrderKey key;
    if (s_key == INT_MAX || !zl_order_setup(A.runs[s_key], K, A.N, key)) {
        for (int k = tid; k < K; k += 256) out[k] = k;
        return;
    }
    for (int b = tid; b < key.nbkt; b += 256) s_hist[b] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += 256) atomicAdd(&s_hist[zl_order_bucket(key, k)], 1);
    __syncthreads();
    // exclusive scan of the histogram: a run of buckets per thread, the runs' sums scanned across the workgroup
    const int per = (key.nbkt + 255) / 256, b0 = tid * per, b1 = b0 + per < key.nbkt ? b0 + per : key.nbkt;
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += s_hist[b];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int t = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += t;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    for (int b = b0; b < b1; ++b) { const int c = s_hist[b]; s_hist[b] = run; run += c; }
    __syncthreads();
    // (the blocks of one bucket land in any order: every bijection renders the same bits)
    const bool sorts = zl_order_sorts(key, K);
    for (int k = tid; k < K; k += 256) out[atomicAdd(&s_hist[zl_order_bucket(key, k)], 1)] = sorts ? (int)zl_order_pack(key, k) : k;
    if (!sorts) return;
    __syncthreads();
    // inside a bucket: by exact phase, ties by block number (zl_order.h) -- neighbours in the order share a workgroup (ZL_K2_PAIR_LAPS).  One
    // thread per bucket (s_hist[b] is now the end of its segment): the segment's packed words into registers with independent loads, a
    // sorting network of constant indices, and back as block numbers.  A longer segment is only unpacked.
    for (int b = tid; b < key.nbkt; b += 256) {
        const int s = b ? s_hist[b - 1] : 0, n = s_hist[b] - s;
        if (n <= 32) zl_k1o_sort_segment<32>(out + s, n);
        else if (n <= ZL_ORDER_SORT_MAX) zl_k1o_sort_segment<ZL_ORDER_SORT_MAX>(out + s, n);
        else for (int i = 0; i < n; ++i) out[s + i] &= 0xffff;
    }
}

// ------------------------------------------------------------------------------------------------
// K2: one workgroup = one (bus, mix group, block); one lane = one output frame.  The voices of the
// group are walked sequentially in voice order, so the per-frame sum has the reference's order
// (SamplerSynth.cpp:136-140) and lives in two registers.  Every per-voice record is wave-uniform
// (scalar loads); the only vector memory traffic is the 16-byte two-tap stereo gather and the
// final coalesced store.
static __device__ __forceinline__ int zl_sample_to_peak_int(float x)
{
    // (int)fabsf(131072.f * x), AudioLevels.cpp:356,367, with the oracle's definition of the cases C leaves open: NaN -> 0, 2^31 and above
    // (and infinity) -> INT_MAX.  That is what v_cvt_i32_f32 does by itself (truncation, saturation, NaN -> 0): one instruction with the
    // |.| source modifier instead of two compares and three exec-masked branches per sample
    const float v = 131072.0f * x;
    int r;
    asm("v_cvt_i32_f32_e64 %0, |%1|" : "=v"(r) : "v"(v));
    return r;
}

// Wavefront reductions on the VALU (DPP row shifts / broadcasts, no LDS round trips): quad permutes, row_shr 4 and 8
// leave each 16-lane row's result in its last lane, row_bcast 15 / 31 carry it across the rows; the result of the
// whole wave is in lane 63.  `ident` fills lanes without a source (0 for max over non-negative ints and for sums).
template <int CTRL, int ROWMASK>
static __device__ __forceinline__ int zl_dpp_i(int ident, int v) { return __builtin_amdgcn_update_dpp(ident, v, CTRL, ROWMASK, 0xf, false); }
static __device__ __forceinline__ int zl_wave_max_nonneg(int v)
{
    int t;
    t = zl_dpp_i<0xB1, 0xf>(0, v);  v = t > v ? t : v;             // quad_perm [1,0,3,2]
    t = zl_dpp_i<0x4E, 0xf>(0, v);  v = t > v ? t : v;             // quad_perm [2,3,0,1]
    t = zl_dpp_i<0x114, 0xf>(0, v); v = t > v ? t : v;             // row_shr 4
    t = zl_dpp_i<0x118, 0xf>(0, v); v = t > v ? t : v;             // row_shr 8
    t = zl_dpp_i<0x142, 0xa>(0, v); v = t > v ? t : v;             // row_bcast 15 -> rows 1, 3
    t = zl_dpp_i<0x143, 0xc>(0, v); v = t > v ? t : v;             // row_bcast 31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}
static __device__ __forceinline__ float zl_wave_sum(float x)
{
    int v = __float_as_int(x), t;
    t = zl_dpp_i<0xB1, 0xf>(0, v);  v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    t = zl_dpp_i<0x4E, 0xf>(0, v);  v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    t = zl_dpp_i<0x114, 0xf>(0, v); v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    t = zl_dpp_i<0x118, 0xf>(0, v); v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    t = zl_dpp_i<0x142, 0xa>(0, v); v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    t = zl_dpp_i<0x143, 0xc>(0, v); v = __float_as_int(__int_as_float(v) + __int_as_float(t));
    return __int_as_float(__builtin_amdgcn_readlane(v, 63));
}

// the four reductions of one bus's fused level scan (two integer peaks, two sums of squares) in ONE instruction sequence: the same
// DPP trees as zl_wave_max_nonneg / zl_wave_sum -- same operands, same order, same bits -- one instruction per step and value (the row
// broadcasts write their rows in place), the four chains interleaved so that no step waits out the DPP read-after-write hazard of its
// own predecessor (2 wait states: three other instructions stand between).  What the compiler makes of the four separate calls is
// ~50 VALU + ~20 s_nop per bus and wave; this is 24 + 4 v_readlane.  (s_nop 4 in front: 5 wait states cover every hazard a DPP
// read can have with the code before the block, which the compiler's hazard recogniser does not look into.)  All 64 lanes active.
#define ZL_DPP4(ctrl) "v_max_i32_dpp %0, %0, %0 " ctrl "\n\tv_max_i32_dpp %1, %1, %1 " ctrl "\n\tv_add_f32_dpp %2, %2, %2 " ctrl "\n\tv_add_f32_dpp %3, %3, %3 " ctrl "\n\t"
static __device__ __forceinline__ void zl_wave_levels4(int &pkL, int &pkR, float &sqL, float &sqR)
{
    int a = pkL, b = pkR, ra, rb;
    float c = sqL, d = sqR, rc, rd;
    asm("s_nop 4\n\t"
        ZL_DPP4("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_bcast:15 row_mask:0xa bank_mask:0xf")
        ZL_DPP4("row_bcast:31 row_mask:0xc bank_mask:0xf")
        "s_nop 0\n\t"
        "v_readlane_b32 %4, %0, 63\n\tv_readlane_b32 %5, %1, 63\n\tv_readlane_b32 %6, %2, 63\n\tv_readlane_b32 %7, %3, 63"
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "=s"(ra), "=s"(rb), "=s"(rc), "=s"(rd));
    pkL = ra; pkR = rb; sqL = rc; sqR = rd;
}
// The twin for two frames per lane (zl_k2_pair_body): a 64-frame tile sits in HALF a wave, lane j' of the half holding the tile's elements
// 2 j' and 2 j' + 1.  Level 1 of the tile's balanced tree is the caller's in-lane add / max; levels 2 to 6 are the same five DPP steps without
// the last one (row_bcast:31 would join the wave's two tiles), each with the operands the 64-lane tree gives that level.  The results of the
// wave's tiles 0 / 1 are in lanes 31 / 63.
static __device__ __forceinline__ void zl_wave_levels4_pair(int pkL, int pkR, float sqL, float sqR, int (&opkL)[2], int (&opkR)[2], float (&osqL)[2], float (&osqR)[2])
{
    int a = pkL, b = pkR, ra0, rb0, ra1, rb1;
    float c = sqL, d = sqR, rc0, rd0, rc1, rd1;
    asm("s_nop 4\n\t"
        ZL_DPP4("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        ZL_DPP4("row_bcast:15 row_mask:0xa bank_mask:0xf")
        "s_nop 0\n\t"
        "v_readlane_b32 %4, %0, 31\n\tv_readlane_b32 %5, %1, 31\n\tv_readlane_b32 %6, %2, 31\n\tv_readlane_b32 %7, %3, 31\n\t"
        "v_readlane_b32 %8, %0, 63\n\tv_readlane_b32 %9, %1, 63\n\tv_readlane_b32 %10, %2, 63\n\tv_readlane_b32 %11, %3, 63"
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "=s"(ra0), "=s"(rb0), "=s"(rc0), "=s"(rd0), "=s"(ra1), "=s"(rb1), "=s"(rc1), "=s"(rd1));
    opkL[0] = ra0; opkR[0] = rb0; osqL[0] = rc0; osqR[0] = rd0;
    opkL[1] = ra1; opkR[1] = rb1; osqL[1] = rc1; osqR[1] = rd1;
}
#undef ZL_DPP4

// maximum of a wave's non-negative floats (they order like their bit patterns), wave-uniform
static __device__ __forceinline__ float zl_wave_max(float x) { return __int_as_float(zl_wave_max_nonneg(__float_as_int(x))); }

// 16-byte gather of the two interpolation taps of both channels (interleaved stereo), 8-byte aligned
typedef float zl_f4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef float zl_f2a4 __attribute__((ext_vector_type(2), aligned(4)));

#define ZL_K2_CHUNK 128      // voice records staged in LDS per pass
#define ZL_K2_MAXNB 16       // narrow buses per workgroup (128 voices / the minimum bus width of 8)
#ifndef ZL_K2_U
#define ZL_K2_U     8        // gathers in flight per wavefront
#endif
#ifndef ZL_K2_U_ONGRID
// loads in flight per wavefront in the on-grid chunk (2 registers a voice): ZL_K2_U, or twice that (two such chunks in a row go as one).
// 16 measured and NOT shipped: + 2 % on the headline, but the time-order headline kernel gains scratch memory, the 64- / 128-frame kernels go
// to 100 bytes of it and the FIX_DELAY kernels from 5 to 4 waves per SIMD (profiles/round6_ongrid_bench.txt)
#define ZL_K2_U_ONGRID 8
#endif
#ifndef ZL_K2_U_HERMITE
#define ZL_K2_U_HERMITE 4    // voices per chunk with 4-tap interpolation (two 16-byte gathers per voice)
#endif
#ifndef ZL_K2_WAVES_LINEAR
// linear mode, one block per workgroup (the headline shape): waves per SIMD asked of the register allocator.  The LDS cap of
// zl_launch_render holds this kernel at 5 workgroups per CU = 5 waves per SIMD whatever its registers: with 5 the allocator may use
// 96 registers instead of 80 and the kernel gains 0.5 % (headline) to 2 % (64-voice engines) -- profiles/round3_k2_roll_ab.txt
#define ZL_K2_WAVES_LINEAR 5
#endif
#ifndef ZL_K2_PREFETCH_BUS
// narrow buses: issue the next bus's gathers before the finished bus's epilogue (1).  Measured and NOT shipped: 1-2 % slower than 0 on 64- / 96-voice
// engines (profiles/round4_levels_epilogue_ab.txt) -- the epilogue's stores share vmcnt with the gathers, so the first mix waits for all of them
#define ZL_K2_PREFETCH_BUS 0
#endif
#ifndef ZL_K2_MINWAVES
#define ZL_K2_MINWAVES 1      // __launch_bounds__ minimum waves per SIMD (caps the VGPR budget)
#endif

// 16-byte gather of the interpolation taps: interleaved stereo [L0 R0 L1 R1] or mono [x0 x1 . .]
typedef float zl_f4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float zl_f2a4b __attribute__((ext_vector_type(2), aligned(4)));

struct ZlK2Tap { ZlTaps t; float alpha, env; int flags; };   // flags: 1 act, 2 inb, 4 stereo, 16 wide

// One chunk of U consecutive voices for one lane (= one output frame).  Branch-free per voice so the
// U gathers (and, for CTL chunks, the U per-frame control loads before them) are issued back to back
// and stay in flight together; the voices are then mixed and accumulated in voice order.
// CTL = the chunk contains a block with per-frame control (envelope not in steady sustain, or a
// block expanded by K1c); regular voices of such a chunk read a dummy control word.
// SIMPLE chunks (the steady state): every voice of the chunk plays the whole block from one position segment, in
// sustain, from a stereo source.  No per-voice predicates are needed, which halves the VALU work.
// Packed (l, r) arithmetic of zl_mix_frame for the simple chunks: both channels go through the same expression, so
// the two lanes of a float2 are the reference's l and r sequences, evaluated by v_pk_mul_f32 / v_pk_add_f32 (the
// kernel's VALU budget is ~49 lane-operations per voice-sample at the HBM roofline; un-fused, -ffp-contract=off).
typedef float zl_f2 __attribute__((ext_vector_type(2)));

// unit-step blocks (playback at the source rate inside an exact run): integer part of P0 and the constant fraction
// + the gain products (gain * envelope) * volume of the Hermite mode's whole-sample gain (zl_render.h), one number per voice-block in sustain
// The gain products are read in the Hermite mode only, and no voice is on-grid there (zl_voice_ongrid): in every other mode their
// eight bytes hold, for a voice classed on-grid, the byte address of the block's frame 0 in the arena (zl_unit_record) -- the one
// thing the on-grid chunks read of the voice besides its pan pair.
// (alt: a voice-block with one loop restart on the grid, zl_k2_stage_unit)
struct ZlUnit { int ipos; union { float alpha; int alt; }; union { struct { float gpl, gpr; }; uint64_t addr0; }; };
static_assert(sizeof(ZlUnit) == 16, "one 16-byte LDS record per voice");

// the ZlUnit of a staged voice-block (cls: zl_k2_stage_class).  addr0 = arena + 4 src_offset + 8 ipos (4 ipos mono) in 64-bit unsigned
// arithmetic: the offset of a source in a grown arena segment is relative to the first segment and wraps modulo 2^64, as the pointer
// arithmetic of the two-tap chunks does
template <uint32_t MODE>
static __device__ __forceinline__ ZlUnit zl_unit_record(const ZlBatch &A, const ZlVoiceConst &vc, const ZlBlockPlan &pl, int cls)
{
    ZlUnit un;
    un.ipos = (int)pl.P0; un.alpha = (float)(pl.P0 - (double)un.ipos);
    if (MODE & ZL_MODE_HERMITE) {
        un.gpl = (vc.lgain * pl.env) * vc.clip_volume; un.gpr = (vc.rgain * pl.env) * vc.clip_volume;
    } else {
        const uint64_t frame0 = (uint64_t)(uint32_t)un.ipos << ((cls & 16) ? 2 : 3);
        un.addr0 = (cls & 128) ? (uint64_t)reinterpret_cast<uintptr_t>(A.arena) + (vc.src_offset << 2) + frame0 : 0ull;
    }
    return un;
}

// zl_hermite_weights / zl_hermite4 (zl_render.h) with both channels in one register pair: the weights are scalar work shared by
// the channels, the four multiply-adds are v_pk_fma_f32 (one rounding per fused operation, as fmaf)
static __device__ __forceinline__ zl_f2 zl_fma2(zl_f2 a, zl_f2 b, zl_f2 c) { return __builtin_elementwise_fma(a, b, c); }
static __device__ __forceinline__ zl_f2 zl_hermite4_pk(zl_f2 y0, zl_f2 y1, zl_f2 y2, zl_f2 y3, float a)
{
    const ZlHermiteW w = zl_hermite_weights(a);
    return zl_fma2((zl_f2){w.w3, w.w3}, y3, zl_fma2((zl_f2){w.w2, w.w2}, y2, zl_fma2((zl_f2){w.w1, w.w1}, y1, (zl_f2){w.w0, w.w0} * y0)));
}

// gprod (Hermite mode only): (gain * envelope) * volume of both channels, formed by the caller (per voice-block in sustain)
template <uint32_t MODE>
static __device__ __forceinline__ zl_f2 zl_mix_frame_pk(zl_f2 xm, zl_f2 x0, zl_f2 x1, zl_f2 x2, float alpha, bool inb, bool wide,
                                                         zl_f2 gain, float env, float vol, zl_f2 pan, zl_f2 gprod = (zl_f2){0.0f, 0.0f})
{
    const float invAlpha = 1.0f - alpha;                         // :200
    zl_f2 lr;
    if (MODE & ZL_MODE_HERMITE) {
        const zl_f2 h = zl_hermite4_pk(xm, x0, x1, x2, alpha);
        const zl_f2 lin = x0 * invAlpha + x1 * alpha;
        lr = (wide ? h : lin) * gprod;                              // whole-sample gain, the product formed first (zl_render.h)
    } else if (MODE & ZL_MODE_FIX_GAIN) {
        lr = (x0 * invAlpha + x1 * alpha) * gain * env * vol;
    } else {
        lr = x0 * invAlpha + x1 * alpha * gain * env * vol;      // :204-205, quirk Q1
    }
    if (!inb) lr = (zl_f2){0.0f, 0.0f};                          // stereo source: r = l = 0 out of range
    const float mSignal = 0.5f * (lr.x + lr.y);                  // :208
    const float sSignal = lr.x - lr.y;                           // :209
    return pan * mSignal + (zl_f2){sSignal, -sSignal};           // :210-211
}

// ZL_K2_PK_LINEAR / ZL_K2_PK_HERMITE: evaluate the simple chunks with the packed float2 arithmetic above (1) or with
// the scalar zl_mix_frame (0).  Same results bit for bit; the choice is a measured one.
#ifndef ZL_K2_PK_LINEAR
#define ZL_K2_PK_LINEAR 0
#endif
#ifndef ZL_K2_PK_HERMITE
#define ZL_K2_PK_HERMITE 1
#endif

// the gathers of one simple chunk, in flight: issued by zl_k2_simple_issue, consumed by zl_k2_simple_mix
template <bool HERM, int U> struct ZlSimpleTaps { zl_f4a4 d[U], e[HERM ? U : 1]; float alpha[U]; int widem; };

// first half of a simple chunk: the U positions and the U gathers, issued back to back.
// INT ("interior"): every frame of the block lies inside the source for every voice of the chunk (checked per voice at
// staging from the block's first and last position) -- no bounds guard, no tap selects, no read of the duration.
template <uint32_t MODE, bool SEG2, bool UNIT, bool INT, int U>
static __device__ __forceinline__ void zl_k2_simple_issue(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                           int c0, int f, double fd, ZlSimpleTaps<(MODE & ZL_MODE_HERMITE) != 0, U> &T)
{
    constexpr bool HERM = (MODE & ZL_MODE_HERMITE) != 0;
    T.widem = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        double P;
        if (SEG2) {                                               // a binade crossing or loop restart inside the block
            const bool seg1 = f >= s_plan[i].n1;
            P = fma((double)(f - (seg1 ? s_plan[i].n1 : 0)), seg1 ? s_plan[i].step1 : s_plan[i].step, seg1 ? s_plan[i].P1 : s_plan[i].P0);
        } else if (!UNIT) {
            P = fma(fd, s_plan[i].step, s_plan[i].P0);            // exact, see zl_plan.h
        }
        // :198-199 -- P >= 0 here, so pos = floor(P) and alpha = (float)(P - pos) = (float)fract(P), both exact
        int pos;
        if (UNIT) {
            // step == 1 inside an exact run: every frame has the fractional part of P0 and the integer part moves by f
            pos = s_unit[i].ipos + f;
            T.alpha[u] = s_unit[i].alpha;
        } else {
            pos = (int)P;
            T.alpha[u] = (float)__builtin_amdgcn_fract(P);
        }
        const int dur = INT ? 0 : s_vc[i].sample_duration;
        const bool inb = INT || dur > pos;                        // :204 guard (Q5)
        // out of range: gather the zero padding behind the source (8 frames, written by zl_k_interleave), so that
        // l = r = 0 falls out of the arithmetic (0 * finite = +-0, +0 + -0 = +0) without a select per channel;
        // voices with a non-finite gain are not "simple"
        int p = inb ? pos : dur + 1;
        const uint64_t so = s_vc[i].src_offset;
        const float *src = A.arena + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(so >> 32)) << 32)
                                      | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)so));
        if (HERM) {
            // taps pos-1 .. pos+2 as two 16-byte loads; at the source edges (not wide) the pair pos, pos+1 comes first
            const bool wide = INT || (inb && pos >= 1 && pos + 2 <= dur);
            p -= wide ? 1 : 0;
            // (uniform 64-bit base + 32-bit byte offset: the scalar-base form of global_load, no 64-bit VALU address)
            const uint32_t ob = (uint32_t)p << 3;
            T.d[u] = *reinterpret_cast<const zl_f4a4 *>(reinterpret_cast<const char *>(src) + ob);
            T.e[u] = *reinterpret_cast<const zl_f4a4 *>(reinterpret_cast<const char *>(src) + ob + 16u);   // inside the arena padding at the end
            T.widem |= wide ? (1 << u) : 0;
        } else {
            T.d[u] = *reinterpret_cast<const zl_f4a4 *>(reinterpret_cast<const char *>(src) + ((uint32_t)p << 3));
        }
    }
}

// second half: the voices mixed and accumulated in voice order
template <uint32_t MODE, bool INT, int U>
static __device__ __forceinline__ void zl_k2_simple_mix(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                         int c0, int vfirst, bool wantPeak, const ZlSimpleTaps<(MODE & ZL_MODE_HERMITE) != 0, U> &T,
                                                         float &accL, float &accR)
{
    constexpr bool HERM = (MODE & ZL_MODE_HERMITE) != 0;
    constexpr bool PK = HERM ? (ZL_K2_PK_HERMITE != 0) : (ZL_K2_PK_LINEAR != 0);
    zl_f2 acc = {accL, accR};
    // every lane of the wave has all four Hermite taps inside its source (true except in the blocks at a loop's ends):
    // the wave-uniform fast form needs no tap selects and no linear alternative
    const bool allWide = HERM && PK && (INT || __all(T.widem == (1 << U) - 1));
    if (allWide) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = c0 + u;
            const zl_f2 o = zl_mix_frame_pk<MODE>((zl_f2){T.d[u].x, T.d[u].y}, (zl_f2){T.d[u].z, T.d[u].w}, (zl_f2){T.e[HERM ? u : 0].x, T.e[HERM ? u : 0].y},
                                                  (zl_f2){T.e[HERM ? u : 0].z, T.e[HERM ? u : 0].w}, T.alpha[u], true, true,
                                                  (zl_f2){s_vc[i].lgain, s_vc[i].rgain}, s_plan[i].env, s_vc[i].clip_volume,
                                                  (zl_f2){s_vc[i].lpan, s_vc[i].rpan}, (zl_f2){s_unit[i].gpl, s_unit[i].gpr});
            acc += o;
            if (wantPeak) {
                const float ng = o.x + o.y;
                float pk = ng > 0.0f ? ng : 0.0f;
                pk = zl_wave_max(pk);
                if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
            }
        }
        accL = acc.x; accR = acc.y;
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const bool wide = INT || ((T.widem >> u) & 1);
        float l, r;
        if (PK) {
            zl_f2 xm, x0, x1, x2;
            if (HERM) {
                xm = (zl_f2){T.d[u].x, T.d[u].y};
                x0 = wide ? (zl_f2){T.d[u].z, T.d[u].w} : (zl_f2){T.d[u].x, T.d[u].y};
                x1 = wide ? (zl_f2){T.e[u].x, T.e[u].y} : (zl_f2){T.d[u].z, T.d[u].w};
                x2 = (zl_f2){T.e[u].z, T.e[u].w};
            } else {
                x0 = (zl_f2){T.d[u].x, T.d[u].y}; x1 = (zl_f2){T.d[u].z, T.d[u].w};
                xm = x0; x2 = x1;
            }
            const zl_f2 o = zl_mix_frame_pk<MODE>(xm, x0, x1, x2, T.alpha[u], true, wide,
                                                  (zl_f2){s_vc[i].lgain, s_vc[i].rgain}, s_plan[i].env, s_vc[i].clip_volume,
                                                  (zl_f2){s_vc[i].lpan, s_vc[i].rpan}, (zl_f2){s_unit[i].gpl, s_unit[i].gpr});
            acc += o;                                             // :218-221 (index shift applied at the store)
            l = o.x; r = o.y;
        } else {
            ZlTaps t;
            if (HERM) {
                t.xml = T.d[u].x; t.xmr = T.d[u].y;
                t.x0l = wide ? T.d[u].z : T.d[u].x; t.x0r = wide ? T.d[u].w : T.d[u].y;
                t.x1l = wide ? T.e[u].x : T.d[u].z; t.x1r = wide ? T.e[u].y : T.d[u].w;
                t.x2l = T.e[u].z; t.x2r = T.e[u].w;
            } else {
                t.x0l = T.d[u].x; t.x0r = T.d[u].y; t.x1l = T.d[u].z; t.x1r = T.d[u].w;
                t.xml = t.xmr = t.x2l = t.x2r = 0.0f;
            }
            zl_mix_frame<MODE>(t, T.alpha[u], true, wide, true, s_vc[i].lgain, s_vc[i].rgain, s_plan[i].env,
                               s_vc[i].clip_volume, s_vc[i].lpan, s_vc[i].rpan, l, r);
            accL += l; accR += r;                                 // :218-221 (index shift applied at the store)
        }
        if (wantPeak) {                                           // :213-216, signed peak from 0 (Q6)
            const float ng = l + r;
            float pk = ng > 0.0f ? ng : 0.0f;
            pk = zl_wave_max(pk);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
    if (PK) { accL = acc.x; accR = acc.y; }
}

template <uint32_t MODE, bool SEG2, bool UNIT, bool INT, int U>
static __device__ __forceinline__ void zl_k2_chunk_simple(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                           int c0, int vfirst, int f, double fd, bool wantPeak, float &accL, float &accR)
{
    ZlSimpleTaps<(MODE & ZL_MODE_HERMITE) != 0, U> T;
    zl_k2_simple_issue<MODE, SEG2, UNIT, INT, U>(A, s_plan, s_vc, s_unit, c0, f, fd, T);
    zl_k2_simple_mix<MODE, INT, U>(A, s_plan, s_vc, s_unit, c0, vfirst, wantPeak, T, accL, accR);
}

// ON-GRID chunks (zl_render.h, zl_voice_ongrid): every voice of the chunk plays at its own rate from an integer position inside a
// source known to be finite.  alpha = 0 in every frame, so the lane loads its OWN frame only -- one 8-byte load per voice (4 bytes
// mono), 512 contiguous bytes per wave instead of a 1 KiB overlapping gather -- and mixes it with zl_mix_frame_ongrid: no second tap,
// no gain chain, no read of the gains from LDS.  U loads in flight, the voices accumulated in voice order, the report as in
// zl_k2_simple_mix.  Same bus and reports as the two-tap form, bit for bit.
//
// ONE ADDRESS PER VOICE: staging leaves the byte address of the block's frame 0 in the voice's ZlUnit (zl_unit_record), so the chunk reads one
// 8-byte LDS word per voice, makes it the load's scalar base with two v_readfirstlane, and every load of the lane shares ONE vector offset
// (8 f bytes, 4 f mono) formed before the loop.  PEAK = the workgroup renders the call's last block (wave-uniform, chosen once by the caller):
// the report path is a template parameter so that the steady-state instantiation is one straight-line block.  It keeps the scalar text
// (it runs in the workgroups of one block per call).
//
// ZL_K2_ONGRID_PK: the mix of an on-grid frame in packed f32 (1, zl_mix_acc_ongrid_pk) or as the scalar text of zl_mix_frame_ongrid (0).  The same
// bits either way: each half of v_pk_add_f32 / v_pk_mul_f32 is the IEEE single operation of v_add_f32 / v_mul_f32, nothing is fused, and a - b
// is a + (-b) by a source modifier (zl_render.h, zl_mix_frame_ongrid_pk, is the sequence restated for the CPU tier).  The compiler does not find
// this packing (it packs across frames and pays for it in v_mov_b32), hence the inline assembly; it is five instructions a frame for nine:
//   (l + r, l - r)            v_pk_add_f32 on the loaded pair with itself, neg_hi
//   0.5 (l + r)               v_mul_f32 on the low half, in place
//   (lpan m, rpan m)          v_pk_mul_f32, the low half of (m, s) in both lanes
//   (lpan m + s, rpan m - s)  v_pk_add_f32, the high half of (m, s) in both lanes, neg_hi
//   acc (L, R) += ...         v_pk_add_f32
#ifndef ZL_K2_ONGRID_PK
#define ZL_K2_ONGRID_PK 1
#endif
// (x.lo + x.hi, x.lo - x.hi); the _lo / _hi forms take both operands from ONE half: (x + x, x - x), the frame of a mono source
static __device__ __forceinline__ zl_f2 zl_pk_sumdiff(zl_f2 x)
{
    zl_f2 r; asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(x)); return r;
}
static __device__ __forceinline__ zl_f2 zl_pk_sumdiff_lo(zl_f2 x)
{
    zl_f2 r; asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(x)); return r;
}
static __device__ __forceinline__ zl_f2 zl_pk_sumdiff_hi(zl_f2 x)
{
    zl_f2 r; asm("v_pk_add_f32 %0, %1, %1 op_sel:[1,1] op_sel_hi:[1,1] neg_hi:[0,1]" : "=v"(r) : "v"(x)); return r;
}
// (pan.lo * ms.lo, pan.hi * ms.lo)
static __device__ __forceinline__ zl_f2 zl_pk_pan(zl_f2 pan, zl_f2 ms)
{
    zl_f2 r; asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(pan), "v"(ms)); return r;
}
// (a.lo + ms.hi, a.hi - ms.hi)
static __device__ __forceinline__ zl_f2 zl_pk_side(zl_f2 a, zl_f2 ms)
{
    zl_f2 r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(ms)); return r;
}
static __device__ __forceinline__ zl_f2 zl_pk_add(zl_f2 a, zl_f2 b)
{
    zl_f2 r; asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
// :208-211 and :218-221 of one on-grid frame: acc (L, R) += zl_mix_frame_ongrid(x.lo, x.hi, pan.lo, pan.hi).  SEL = 0: x is the frame (l, r);
// 1 / 2: x holds two frames of a mono source and the frame is its low / high half (r = l, :205)
template <int SEL>
static __device__ __forceinline__ void zl_mix_acc_ongrid_pk(zl_f2 &acc, zl_f2 x, zl_f2 pan)
{
    zl_f2 ms = SEL == 0 ? zl_pk_sumdiff(x) : SEL == 1 ? zl_pk_sumdiff_lo(x) : zl_pk_sumdiff_hi(x);
    ms.x = 0.5f * ms.x;                                           // :208
    acc = zl_pk_add(acc, zl_pk_side(zl_pk_pan(pan, ms), ms));     // :210-211, :218-221 (index shift applied at the store)
}

// the scalar base of a voice's loads: its frame-0 address out of LDS (wave-uniform), made scalar ...
static __device__ __forceinline__ uint64_t zl_k2_ongrid_base(const ZlUnit *s_unit, int i)
{
    const uint64_t a = s_unit[i].addr0;
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a);
}
// ... and the load from it: scalar 64-bit base + the lane's 32-bit byte offset, the scalar-base form of global_load (the address is an integer
// here, so the pointer is given its address space by hand: a generic pointer would make it a flat load behind a 64-bit vector add)
// The lane's byte offset is the same for every chunk of the block; left to itself the compiler widens it to 64 bits once, outside the loop over
// the chunks, and instruction selection -- which works block by block -- no longer sees "scalar base + zero-extended 32-bit offset": each load
// then gets a 64-bit vector add.  The empty statement makes the offset a value of the chunk's own block.
static __device__ __forceinline__ uint32_t zl_k2_ongrid_offset(uint32_t ob) { asm volatile("" : "+v"(ob)); return ob; }
template <typename T>
static __device__ __forceinline__ T zl_k2_ongrid_load(uint64_t base, uint32_t ob)
{
    return *reinterpret_cast<const __attribute__((address_space(1))) T *>(base + (uint64_t)ob);
}

template <bool MONO, int U, bool PEAK>
static __device__ __forceinline__ void zl_k2_chunk_ongrid(const ZlBatch &A, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                           int c0, int vfirst, int f, float &accL, float &accR)
{
    zl_f2 d2[MONO ? 1 : U];
    float d1[MONO ? U : 1];
    const uint32_t ob = zl_k2_ongrid_offset((uint32_t)f << (MONO ? 2 : 3));   // interior: frame ipos + f is inside the source for every frame of the block
    zl_f2 pan[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t src = zl_k2_ongrid_base(s_unit, c0 + u);
        // (sources start on 16-byte boundaries: a stereo frame is 8-byte aligned)
        if (MONO) d1[u] = zl_k2_ongrid_load<float>(src, ob);
        else      d2[u] = zl_k2_ongrid_load<zl_f2>(src, ob);
        pan[u] = *reinterpret_cast<const zl_f2 *>(&s_vc[c0 + u].lpan);
    }
    // every load of the chunk is in flight before the first voice is mixed (without the per-voice branch the scheduler is free to pull each
    // voice's arithmetic up behind its load, and then every load waits for the one before it)
    __builtin_amdgcn_sched_barrier(0);
    if (ZL_K2_ONGRID_PK && !PEAK && !MONO) {
        zl_f2 acc = {accL, accR};
#pragma unroll
        for (int u = 0; u < U; ++u) zl_mix_acc_ongrid_pk<0>(acc, d2[u], pan[u]);
        accL = acc.x; accR = acc.y;
        return;
    }
    // (a mono frame is one register: building the pair (x, x) costs what the packing saves, so mono keeps the scalar text here)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        float l, r;
        zl_mix_frame_ongrid(MONO ? d1[u] : d2[u].x, MONO ? d1[u] : d2[u].y, pan[u].x, pan[u].y, l, r);
        accL += l; accR += r;                                     // :218-221 (index shift applied at the store)
        if (PEAK) {                                               // :213-216, signed peak from 0 (Q6)
            const float ng = l + r;
            float pk = ng > 0.0f ? ng : 0.0f;
            pk = zl_wave_max(pk);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
}

// (the chunk's source layout, wave-uniform like PEAK)
template <int U, bool PEAK>
static __device__ __forceinline__ void zl_k2_ongrid_dispatch(const ZlBatch &A, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                              int c0, int vfirst, int f, bool mono, float &accL, float &accR)
{
    if (mono) zl_k2_chunk_ongrid<true, U, PEAK>(A, s_vc, s_unit, c0, vfirst, f, accL, accR);
    else      zl_k2_chunk_ongrid<false, U, PEAK>(A, s_vc, s_unit, c0, vfirst, f, accL, accR);
}

// The on-grid chunk with TWO frames per lane (zl_k2_pair_body): the lane renders frames f0 (even) and f0 + 1.  The two frames of an on-grid
// voice are 16 contiguous bytes, 8-byte aligned -- the alignment of the two-tap gather -- so ONE 16-byte load [L0 R0 L1 R1] per voice serves
// two voice-samples (mono: 8 bytes [x0 x1]) and a wave's load is 1 KiB contiguous: half the load instructions per voice-sample, and the
// address, the two v_readfirstlane and the pan read are paid once per pair.  Interior means frame N - 1 is inside the source, so f0 + 1 is.
// Each frame keeps its own accumulator pair and is added to in voice order: per frame nothing about the summation changes.  The report peak
// is the larger of the two frames' before the wave maximum (a maximum does not depend on order).
#ifndef ZL_K2_U_PAIR
#define ZL_K2_U_PAIR 8       // loads in flight per wavefront in the pair chunk (4 registers a voice); 8 or 4
#endif
template <bool MONO, int U, bool PEAK>
static __device__ __forceinline__ void zl_k2_chunk_ongrid_pair(const ZlBatch &A, const ZlVoiceConst *s_vc, const ZlUnit *s_unit, int c0, int vfirst, int f0,
                                                                float &accL0, float &accR0, float &accL1, float &accR1)
{
    zl_f4a8 d4[MONO ? 1 : U];
    zl_f2   d2[MONO ? U : 1];
    const uint32_t ob = zl_k2_ongrid_offset((uint32_t)f0 << (MONO ? 2 : 3));   // interior: frames ipos + f0 and ipos + f0 + 1 are inside the source
    zl_f2 pan[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t src = zl_k2_ongrid_base(s_unit, c0 + u);
        if (MONO) d2[u] = zl_k2_ongrid_load<zl_f2a4b>(src, ob);
        else      d4[u] = zl_k2_ongrid_load<zl_f4a8>(src, ob);
        pan[u] = *reinterpret_cast<const zl_f2 *>(&s_vc[c0 + u].lpan);
    }
    __builtin_amdgcn_sched_barrier(0);                            // (all loads in flight before the first mix, as in zl_k2_chunk_ongrid)
    if (ZL_K2_ONGRID_PK && !PEAK) {
        // each frame's (L, R) accumulator is one register pair; a mono pair (x0, x1) feeds both frames by operand selection alone
        zl_f2 acc0 = {accL0, accR0}, acc1 = {accL1, accR1};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (MONO) {
                zl_mix_acc_ongrid_pk<1>(acc0, d2[u], pan[u]);
                zl_mix_acc_ongrid_pk<2>(acc1, d2[u], pan[u]);
            } else {
                zl_mix_acc_ongrid_pk<0>(acc0, __builtin_shufflevector(d4[u], d4[u], 0, 1), pan[u]);
                zl_mix_acc_ongrid_pk<0>(acc1, __builtin_shufflevector(d4[u], d4[u], 2, 3), pan[u]);
            }
        }
        accL0 = acc0.x; accR0 = acc0.y; accL1 = acc1.x; accR1 = acc1.y;
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const float lpan = pan[u].x, rpan = pan[u].y;
        float l0, r0, l1, r1;
        zl_mix_frame_ongrid(MONO ? d2[u].x : d4[u].x, MONO ? d2[u].x : d4[u].y, lpan, rpan, l0, r0);
        zl_mix_frame_ongrid(MONO ? d2[u].y : d4[u].z, MONO ? d2[u].y : d4[u].w, lpan, rpan, l1, r1);
        accL0 += l0; accR0 += r0;                                 // :218-221 (index shift applied at the store)
        accL1 += l1; accR1 += r1;
        if (PEAK) {                                               // :213-216, signed peak from 0 (Q6)
            const float ng0 = l0 + r0, ng1 = l1 + r1;
            const float pk0 = ng0 > 0.0f ? ng0 : 0.0f, pk1 = ng1 > 0.0f ? ng1 : 0.0f;
            const float pk = zl_wave_max(pk1 > pk0 ? pk1 : pk0);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
}

// The pair chunk whose voices are all on-grid and at least one of them RESTARTS ITS LOOP inside the block (chunk class 256: zl_render.h,
// zl_voice_ongrid2).  Frame f of such a voice reads P0 + f below n1 and P1 + (f - n1) from n1 on, both from the same source; the other voices
// of the chunk have n1 = INT_MAX.  Per voice the lane issues the pair's 16-byte load from the segment of its first frame and one 8-byte load
// for the frame a pair that straddles an odd n1 takes from the second segment -- every other lane repeats its own first frame there, so no
// address leaves the source (zl_ongrid2_lane).  Both loads go from the source's first byte with a 32-bit byte offset: the two segments
// lie on either side of each other, and a source is shorter than 4 GiB (zl_k2_stage_class).  Straight-line like zl_k2_chunk_ongrid_pair:
// every load in flight before the first mix, then zl_mix_acc_ongrid_pk per frame in voice order into the same four accumulators.  The
// call's last block (the report path) keeps the two-tap chunk functions.
#ifndef ZL_K2_U_PAIR_WRAP
#define ZL_K2_U_PAIR_WRAP 8  // voices per pass of this chunk (6 data registers a voice); 8 or 4
#endif
template <bool MONO, int U>
static __device__ __forceinline__ void zl_k2_chunk_ongrid_pair_wrap(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                                     int c0, int f0, float &accL0, float &accR0, float &accL1, float &accR1)
{
    zl_f4a8 x4[MONO ? 1 : U];
    zl_f2   y2[MONO ? 1 : U];
    zl_f2   x2[MONO ? U : 1];
    float   y1[MONO ? U : 1];
    zl_f2 pan[U];
    bool straddle[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const ZlWrapLane w = zl_ongrid2_lane(s_unit[i].ipos, s_unit[i].alt, s_plan[i].n1, f0);
        const uint64_t so = s_vc[i].src_offset << 2;
        const uint64_t src = (uint64_t)reinterpret_cast<uintptr_t>(A.arena)
                           + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(so >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)so));
        const uint32_t ox = (uint32_t)w.x << (MONO ? 2 : 3), oy = (uint32_t)w.y << (MONO ? 2 : 3);
        if (MONO) { x2[u] = zl_k2_ongrid_load<zl_f2a4b>(src, ox); y1[u] = zl_k2_ongrid_load<float>(src, oy); }
        else      { x4[u] = zl_k2_ongrid_load<zl_f4a8>(src, ox);  y2[u] = zl_k2_ongrid_load<zl_f2>(src, oy); }
        pan[u] = *reinterpret_cast<const zl_f2 *>(&s_vc[i].lpan);
        straddle[u] = w.straddle;
    }
    __builtin_amdgcn_sched_barrier(0);                            // (all loads in flight before the first mix)
    if (!ZL_K2_ONGRID_PK) {                                       // the scalar text of the same frames, as in zl_k2_chunk_ongrid_pair
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float a0 = MONO ? x2[u].x : x4[u].x, b0 = MONO ? x2[u].x : x4[u].y;
            const float a1 = MONO ? (straddle[u] ? y1[u] : x2[u].y) : (straddle[u] ? y2[u].x : x4[u].z);
            const float b1 = MONO ? a1 : (straddle[u] ? y2[u].y : x4[u].w);
            float l0, r0, l1, r1;
            zl_mix_frame_ongrid(a0, b0, pan[u].x, pan[u].y, l0, r0);
            zl_mix_frame_ongrid(a1, b1, pan[u].x, pan[u].y, l1, r1);
            accL0 += l0; accR0 += r0;                             // :218-221 (index shift applied at the store)
            accL1 += l1; accR1 += r1;
        }
        return;
    }
    zl_f2 acc0 = {accL0, accR0}, acc1 = {accL1, accR1};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (MONO) {
            const zl_f2 d = {x2[u].x, straddle[u] ? y1[u] : x2[u].y};
            zl_mix_acc_ongrid_pk<1>(acc0, d, pan[u]);
            zl_mix_acc_ongrid_pk<2>(acc1, d, pan[u]);
        } else {
            const zl_f2 d1 = {straddle[u] ? y2[u].x : x4[u].z, straddle[u] ? y2[u].y : x4[u].w};
            zl_mix_acc_ongrid_pk<0>(acc0, __builtin_shufflevector(x4[u], x4[u], 0, 1), pan[u]);
            zl_mix_acc_ongrid_pk<0>(acc1, d1, pan[u]);
        }
    }
    accL0 = acc0.x; accR0 = acc0.y; accL1 = acc1.x; accR1 = acc1.y;
}

// UNIT + INT chunks with SHARED taps (ZL_K2_UNIT_SHARE=1): at the playback rate inside an exact run, lane f + 1's first tap IS lane
// f's second (pos = ipos + f), so every lane gathers only its OWN frame -- 8 bytes instead of 16 (16 instead of 32 with four
// taps) -- and takes its neighbours' from their registers: v_mov_b32_dpp wave_shl:1 / wave_shr:1 (lane i reads lane i + 1 / i - 1;
// the lane at the end of the wave keeps the `old` operand).  The taps a wave does not hold (frame + 1 of lane 63; frame - 1 of
// lane 0 and frames + 1, + 2 of lane 63 with four taps) come from ONE extra load executed by those lanes only.  Half (a quarter)
// of the bytes through the texture addresser, the same operands in the same order: bit-identical results.
#ifndef ZL_K2_UNIT_SHARE
#define ZL_K2_UNIT_SHARE 0
#endif
#define ZL_DPP_WAVE_SHL1 0x130
#define ZL_DPP_WAVE_SHR1 0x138
static __device__ __forceinline__ float zl_dpp_next(float old, float v)    // lane i <- lane i + 1; lane 63 <- old
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), ZL_DPP_WAVE_SHL1, 0xf, 0xf, false));
}
static __device__ __forceinline__ float zl_dpp_prev(float old, float v)    // lane i <- lane i - 1; lane 0 <- old
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), ZL_DPP_WAVE_SHR1, 0xf, 0xf, false));
}

template <uint32_t MODE, int U>
static __device__ __forceinline__ void zl_k2_chunk_unit_shared(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                                int c0, int vfirst, int f, bool wantPeak, float &accL, float &accR)
{
    constexpr bool HERM = (MODE & ZL_MODE_HERMITE) != 0;
    const int lane = (int)(threadIdx.x & 63u);
    zl_f2a4b b[U];                                                // the lane's own frame (L, R) of every voice
    zl_f2a4b ex2[HERM ? 1 : U];                                   // linear: frame + 1 of lane 63
    zl_f4a4  ex4[HERM ? U : 1];                                   // four taps: frames - 1, 0 of lane 0; frames + 1, + 2 of lane 63
    const char *src[U];
    uint32_t ob[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const int pos = s_unit[i].ipos + f;
        const uint64_t so = s_vc[i].src_offset;
        src[u] = reinterpret_cast<const char *>(A.arena + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(so >> 32)) << 32)
                                                            | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)so)));
        ob[u] = (uint32_t)pos << 3;
        b[u] = *reinterpret_cast<const zl_f2a4b *>(src[u] + ob[u]);
    }
    if (HERM) {
        if (lane == 0 || lane == 63) {
#pragma unroll
            for (int u = 0; u < U; ++u) ex4[u] = *reinterpret_cast<const zl_f4a4 *>(src[u] + (lane == 0 ? ob[u] - 8u : ob[u] + 8u));
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) ex4[u] = (zl_f4a4){0.0f, 0.0f, 0.0f, 0.0f};
        }
    } else {
        if (lane == 63) {
#pragma unroll
            for (int u = 0; u < U; ++u) ex2[u] = *reinterpret_cast<const zl_f2a4b *>(src[u] + ob[u] + 8u);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) ex2[u] = (zl_f2a4b){0.0f, 0.0f};
        }
    }
    zl_f2 acc = {accL, accR};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const float alpha = s_unit[i].alpha;
        float l, r;
        if (HERM) {
            const zl_f2 x0 = {b[u].x, b[u].y};
            const zl_f2 xm = {zl_dpp_prev(ex4[u].x, b[u].x), zl_dpp_prev(ex4[u].y, b[u].y)};
            const zl_f2 x1 = {zl_dpp_next(ex4[u].x, b[u].x), zl_dpp_next(ex4[u].y, b[u].y)};
            const zl_f2 x2 = {zl_dpp_next(ex4[u].z, x1.x), zl_dpp_next(ex4[u].w, x1.y)};
            const zl_f2 o = zl_mix_frame_pk<MODE>(xm, x0, x1, x2, alpha, true, true, (zl_f2){s_vc[i].lgain, s_vc[i].rgain}, s_plan[i].env, s_vc[i].clip_volume,
                                                  (zl_f2){s_vc[i].lpan, s_vc[i].rpan}, (zl_f2){s_unit[i].gpl, s_unit[i].gpr});
            acc += o;
            l = o.x; r = o.y;
        } else {
            ZlTaps t;
            t.x0l = b[u].x; t.x0r = b[u].y;
            t.x1l = zl_dpp_next(ex2[u].x, b[u].x); t.x1r = zl_dpp_next(ex2[u].y, b[u].y);
            t.xml = t.xmr = t.x2l = t.x2r = 0.0f;
            zl_mix_frame<MODE>(t, alpha, true, true, true, s_vc[i].lgain, s_vc[i].rgain, s_plan[i].env, s_vc[i].clip_volume, s_vc[i].lpan, s_vc[i].rpan, l, r);
            acc.x += l; acc.y += r;
        }
        if (wantPeak) {                                           // :213-216, signed peak from 0 (Q6)
            const float ng = l + r;
            float pk = ng > 0.0f ? ng : 0.0f;
            pk = zl_wave_max(pk);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
    accL = acc.x; accR = acc.y;
}

// The same for chunks of mono sources: an 8-byte gather [x0 x1] (16 bytes [x-1 x0 x1 x2] for Hermite), r = l (:205, Q4).
template <uint32_t MODE, bool SEG2, bool UNIT, bool INT, int U>
static __device__ __forceinline__ void zl_k2_chunk_simple_mono(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlUnit *s_unit,
                                                                int c0, int vfirst, int f, double fd, bool wantPeak, float &accL, float &accR)
{
    constexpr bool HERM = (MODE & ZL_MODE_HERMITE) != 0;
    zl_f4a4 d4[HERM ? U : 1];
    zl_f2a4b d2[HERM ? 1 : U];
    float alpha[U];
    int   widem = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        double P;
        if (SEG2) {
            const bool seg1 = f >= s_plan[i].n1;
            P = fma((double)(f - (seg1 ? s_plan[i].n1 : 0)), seg1 ? s_plan[i].step1 : s_plan[i].step, seg1 ? s_plan[i].P1 : s_plan[i].P0);
        } else if (!UNIT) {
            P = fma(fd, s_plan[i].step, s_plan[i].P0);            // exact, see zl_plan.h
        }
        int pos;                                                  // :198-199 (P >= 0)
        if (UNIT) { pos = s_unit[i].ipos + f; alpha[u] = s_unit[i].alpha; }
        else      { pos = (int)P; alpha[u] = (float)__builtin_amdgcn_fract(P); }
        const int dur = INT ? 0 : s_vc[i].sample_duration;
        const bool inb = INT || dur > pos;                        // :204 guard (Q5)
        int p = inb ? pos : dur + 1;                              // out of range: the zero padding behind the source
        const uint64_t so = s_vc[i].src_offset;
        const float *src = A.arena + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(so >> 32)) << 32)
                                      | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)so));
        if (HERM) {
            const bool wide = INT || (inb && pos >= 1 && pos + 2 <= dur);
            p -= wide ? 1 : 0;
            d4[u] = *reinterpret_cast<const zl_f4a4 *>(reinterpret_cast<const char *>(src) + ((uint32_t)p << 2));
            widem |= wide ? (1 << u) : 0;
        } else {
            d2[u] = *reinterpret_cast<const zl_f2a4b *>(reinterpret_cast<const char *>(src) + ((uint32_t)p << 2));
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const bool wide = INT || ((widem >> u) & 1);
        ZlTaps t;
        t.x0r = t.x1r = t.xmr = t.x2r = 0.0f;
        if (HERM) {
            t.xml = d4[u].x;
            t.x0l = wide ? d4[u].y : d4[u].x;
            t.x1l = wide ? d4[u].z : d4[u].y;
            t.x2l = d4[u].w;
        } else {
            t.x0l = d2[u].x; t.x1l = d2[u].y;
            t.xml = t.x2l = 0.0f;
        }
        float l, r;
        zl_mix_frame<MODE>(t, alpha[u], true, wide, false, s_vc[i].lgain, s_vc[i].rgain, s_plan[i].env,
                           s_vc[i].clip_volume, s_vc[i].lpan, s_vc[i].rpan, l, r);
        accL += l; accR += r;                                     // :218-221 (index shift applied at the store)
        if (wantPeak) {                                           // :213-216, signed peak from 0 (Q6)
            const float ng = l + r;
            float pk = ng > 0.0f ? ng : 0.0f;
            pk = zl_wave_max(pk);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-staged source windows (north_star: "one wavefront per voice-tile with source samples staged in LDS").
// For a (voice, block) whose frames advance along one exact line, the 64 frames of a wavefront read the contiguous source
// window [pos(first) - tb, pos(last) + ta] (tb / ta = taps before / after: 0 / 1 linear, 1 / 2 Hermite).  The wave fetches
// that window ONCE with a single LDS-DMA instruction (global_load_lds_dwordx4: lane i moves bytes [16 i, 16 i + 16) of the
// window straight into LDS, no register in between; lanes past the window's end are masked off) into a slot of its own
// ring, ZL_ST_D voices deep, and its lanes then read their taps from LDS.  Against the register gather this moves each
// source byte through the texture path once instead of 2x (linear) or 4x (Hermite: two overlapping 16-byte gathers per
// lane), and keeps ZL_ST_D - ZL_ST_U .. ZL_ST_D voices of every wave in flight without holding them in VGPRs.
// Windows are private to a wave: no barrier, the wave's own counted s_waitcnt vmcnt orders its reads behind its DMA.
#ifndef ZL_ST_SLOT
#define ZL_ST_SLOT 1024      // bytes per ring slot = one LDS-DMA piece: windows of up to 128 stereo frames (ratio <= 1.95)
#endif
#ifndef ZL_ST_D
#define ZL_ST_D 6            // ring depth in voices (slots per wave); measured: 6 > 10 > 16 (occupancy beats depth, profiles/round2_b_*)
#endif
#ifndef ZL_ST_U
#define ZL_ST_U 2            // voices per staged compute step
#endif
#ifndef ZL_ST_CHUNK
#define ZL_ST_CHUNK 64       // voice records per pass in the staged variant (64 or 128)
#endif
struct ZlWin { int a; int n16; };   // window of one (voice, wave): first source frame (even: 16-byte aligned), 16-byte pieces; n16 == 0: not staged
extern __shared__ __attribute__((aligned(16))) char zl_dyn_lds[];

static __device__ __forceinline__ uint32_t zl_lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)p;
}

// One LDS-DMA piece.  Lane address gaddr (the window's base + this lane's 16 bytes) -> LDS at dst (wave-uniform LDS byte
// address, in M0) + lane * 16, for the lanes with lane16 < nbytes.  The compiler neither sees the load nor counts it: the
// caller waits with zl_wait_vm<N>().  s_waitcnt lgkmcnt(0) first: every LDS read this wave has issued (the previous tenant of
// the slot among them) has returned before the DMA may overwrite it.  M0 is compiler-reserved: saved and restored.
static __device__ __forceinline__ void zl_glds_piece(const char *gaddr, uint32_t lane16, uint32_t nbytes, uint32_t dst)
{
#ifdef ZL_ST_DIAG_NODMA      // timing-only diagnostic build: no DMA (the taps read whatever the ring holds)
    return;
#endif
    unsigned keep; unsigned long long save;
    asm volatile("s_waitcnt lgkmcnt(0)\n\t"
                 "s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %5\n\t"
                 "v_cmp_lt_u32 vcc, %3, %4\n\t"
                 "s_and_saveexec_b64 %1, vcc\n\t"
                 "global_load_lds_dwordx4 %2, off\n\t"
                 "s_mov_b64 exec, %1\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(save)
                 : "v"(gaddr), "v"(lane16), "v"(nbytes), "s"(dst)
                 : "memory", "vcc", "scc");
}
template <int N> static __device__ __forceinline__ void zl_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// What a lane needs of a staged voice besides its taps: wave-uniform values, read from the staged records ONE step ahead
// (they do not depend on the DMA), so that a step's only exposed LDS round trip is the tap read itself.
struct ZlStParams {
    double P0, step;
    int    a;                 // first source frame of this wave's window
    float  env, vol;
    zl_f2  gain, pan, gprod;  // (l, r) pairs
};
static __device__ __forceinline__ ZlStParams zl_st_params(const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc, const ZlWin *s_win, int i)
{
    ZlStParams q;
    q.P0 = s_plan[i].P0; q.step = s_plan[i].step; q.env = s_plan[i].env;
    q.a = s_win[i * 4].a;
    q.gain = (zl_f2){s_vc[i].lgain, s_vc[i].rgain}; q.vol = s_vc[i].clip_volume; q.pan = (zl_f2){s_vc[i].lpan, s_vc[i].rpan};
    q.gprod = (q.gain * q.env) * q.vol;                           // Hermite mode's whole-sample gain (zl_render.h)
    return q;
}
// The DMA of voice j of the pass, as per-lane values (no scalar round trip): lane address and bytes of the window.  Voices
// that are not staged fetch 16 bytes from the start of the arena (always there) by one lane, so that the wave's count of
// outstanding DMAs stays uniform.
struct ZlStDma { const char *g; uint32_t nbytes; };
static __device__ __forceinline__ ZlStDma zl_st_dma(const ZlBatch &A, const ZlVoiceConst *s_vc, const ZlWin *s_win, int j, uint32_t lane16)
{
    const ZlWin wn = s_win[j * 4];
    const uint64_t so = s_vc[j].src_offset;
    ZlStDma d;
    d.g = reinterpret_cast<const char *>(A.arena) + (wn.n16 ? (so << 2) + ((uint64_t)(uint32_t)wn.a << 3) + lane16 : 0ull);
    d.nbytes = wn.n16 ? (uint32_t)wn.n16 << 4 : 16u;
    return d;
}

// The taps of one staged voice for this lane, from ring slot `slot` of the wave.
struct ZlStTaps { zl_f2 xm, x0, x1, x2; float alpha; };
template <uint32_t MODE>
static __device__ __forceinline__ ZlStTaps zl_st_taps(const ZlStParams &q, const char *ring, int slot, double fd)
{
    constexpr bool HERM = (MODE & ZL_MODE_HERMITE) != 0;
    ZlStTaps t;
    const double P = fma(fd, q.step, q.P0);                       // exact, see zl_plan.h
    const int pos = (int)P;                                       // :198-199 (P >= 0)
    t.alpha = (float)__builtin_amdgcn_fract(P);
    const char *p = ring + slot * ZL_ST_SLOT + ((pos - (HERM ? 1 : 0) - q.a) << 3);
    if (HERM) {
        t.xm = *reinterpret_cast<const zl_f2 *>(p);      t.x0 = *reinterpret_cast<const zl_f2 *>(p + 8);
        t.x1 = *reinterpret_cast<const zl_f2 *>(p + 16); t.x2 = *reinterpret_cast<const zl_f2 *>(p + 24);
    } else {
        t.x0 = *reinterpret_cast<const zl_f2 *>(p); t.x1 = *reinterpret_cast<const zl_f2 *>(p + 8);
        t.xm = t.x0; t.x2 = t.x1;
    }
    return t;
}
// :200-221 of one staged voice ("interior": all taps inside the source; stereo, whole block, sustain) -- the same arithmetic
// as the interior variant of zl_k2_chunk_simple.
template <uint32_t MODE>
static __device__ __forceinline__ void zl_st_mix(const ZlBatch &A, const ZlStParams &q, const ZlStTaps &t, int voice, bool wantPeak, zl_f2 &acc)
{
    float l, r;
    if (MODE & ZL_MODE_HERMITE) {
        const zl_f2 o = zl_mix_frame_pk<MODE>(t.xm, t.x0, t.x1, t.x2, t.alpha, true, true, q.gain, q.env, q.vol, q.pan, q.gprod);
        acc += o;
        l = o.x; r = o.y;
    } else {
        ZlTaps tt;
        tt.x0l = t.x0.x; tt.x0r = t.x0.y; tt.x1l = t.x1.x; tt.x1r = t.x1.y;
        tt.xml = tt.xmr = tt.x2l = tt.x2r = 0.0f;
        zl_mix_frame<MODE>(tt, t.alpha, true, false, true, q.gain.x, q.gain.y, q.env, q.vol, q.pan.x, q.pan.y, l, r);
        acc.x += l; acc.y += r;                                   // :218-221 (index shift applied at the store)
    }
    if (wantPeak) {                                               // :213-216, signed peak from 0 (Q6)
        const float ng = l + r;
        float pk = ng > 0.0f ? ng : 0.0f;
        pk = zl_wave_max(pk);
        if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[voice].peak_bits, __float_as_uint(pk));
    }
}

template <uint32_t MODE, bool CTL, int U>
static __device__ __forceinline__ void zl_k2_chunk(const ZlBatch &A, const ZlBlockPlan *s_plan, const ZlVoiceConst *s_vc,
                                                    const int *s_cls, int c0, size_t pbase, int vfirst, int f, bool wantPeak,
                                                    float &accL, float &accR)
{
    const int N = A.N;
    ZlK2Tap tap[U];
    double Pc[U];
    float  Ec[U];
    if (CTL) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = c0 + u;
            const bool ctl = s_cls[i] & 2;
            const bool act = (s_cls[i] & 1) && f < s_plan[i].n_active;
            if (__builtin_expect(ctl && (s_plan[i].flags & (ZL_PLAN_NOSLOT_SIM | ZL_PLAN_NOSLOT_EXPAND)), 0)) {
                // the window's control pool was exhausted when this block was planned: recompute its control (zl_plan.h)
                zl_slow_control(A, s_plan[i], vfirst + i, (int)(pbase / (size_t)A.V), act ? f : 0, Pc[u], Ec[u]);
            } else {
                const size_t off = ctl ? (size_t)(int)s_plan[i].step * (size_t)N + (act ? f : 0) : 0;   // the block's slot; regular voices: word 0 (always valid)
                Pc[u] = A.ctl_P[off];
                Ec[u] = A.ctl_env[off];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const int cls = s_cls[i];
        const bool on = cls & 1;
        const bool act = on && f < s_plan[i].n_active;
        const int fe = act ? f : 0;                               // lanes past the voice's end gather a safe address
        const bool seg1 = fe >= s_plan[i].n1;                     // second linear segment of the block
        const double P0 = seg1 ? s_plan[i].P1 : s_plan[i].P0;
        const double st = seg1 ? s_plan[i].step1 : s_plan[i].step;
        double P = fma((double)(fe - (seg1 ? s_plan[i].n1 : 0)), st, P0);            // exact, see zl_plan.h
        tap[u].env = (float)fma((double)(fe - (seg1 ? s_plan[i].n1 : 0)), (double)(seg1 ? s_plan[i].estep1 : s_plan[i].estep0),
                                (double)(seg1 ? s_plan[i].E1 : s_plan[i].env));    // exact fp32 envelope ramp (0 slope in sustain)
        if (CTL) { if (cls & 2) P = Pc[u]; }
        int pos;
        zl_split_position(P, pos, tap[u].alpha);                  // :198-199
        const int dur = s_vc[i].sample_duration;
        const bool stereo = s_vc[i].channels > 1;
        const bool inb = on && (dur > pos) && (pos >= 0);         // :204 guard (Q5)
        const bool wide = (MODE & ZL_MODE_HERMITE) && inb && (pos - 1 >= 0) && (pos + 2 <= dur);
        const int p = inb ? pos : 0;
        const uint64_t so = on ? s_vc[i].src_offset : 0;
        const float *src = A.arena + (((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(so >> 32)) << 32)
                                      | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)so));
        const size_t e0 = stereo ? 2 * (size_t)p : (size_t)p;
        const zl_f4a4 d = *reinterpret_cast<const zl_f4a4 *>(src + e0);
        tap[u].t.x0l = d.x;
        tap[u].t.x0r = stereo ? d.y : 0.0f;
        tap[u].t.x1l = stereo ? d.z : d.y;
        tap[u].t.x1r = stereo ? d.w : 0.0f;
        if (MODE & ZL_MODE_HERMITE) {
            const size_t em = stereo ? 2 * (size_t)(wide ? p - 1 : p) : (size_t)(wide ? p - 1 : p);
            const size_t e2 = stereo ? 2 * (size_t)(wide ? p + 2 : p) : (size_t)(wide ? p + 2 : p);
            const zl_f2a4b m = *reinterpret_cast<const zl_f2a4b *>(src + em);
            const zl_f2a4b n = *reinterpret_cast<const zl_f2a4b *>(src + e2);
            tap[u].t.xml = m.x; tap[u].t.xmr = stereo ? m.y : 0.0f;
            tap[u].t.x2l = n.x; tap[u].t.x2r = stereo ? n.y : 0.0f;
        } else {
            tap[u].t.xml = tap[u].t.xmr = tap[u].t.x2l = tap[u].t.x2r = 0.0f;
        }
        tap[u].flags = (act ? 1 : 0) | (inb ? 2 : 0) | (stereo ? 4 : 0) | (wide ? 16 : 0);
        if (A.trace && on) A.pos_trace[(pbase + i) * (size_t)N + f] = act ? pos : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = c0 + u;
        const int tf = tap[u].flags;
        const bool act = tf & 1;
        float env = tap[u].env;
        if (CTL) { if (s_cls[i] & 2) env = Ec[u]; }
        float l, r;
        zl_mix_frame<MODE>(tap[u].t, tap[u].alpha, tf & 2, tf & 16, tf & 4, s_vc[i].lgain, s_vc[i].rgain, env,
                           s_vc[i].clip_volume, s_vc[i].lpan, s_vc[i].rpan, l, r);
        if (act) { accL += l; accR += r; }                        // :218-221 (index shift applied at the store)
        if (wantPeak) {                                           // :213-216, signed peak from 0 (Q6)
            const float ng = l + r;
            float pk = (act && ng > 0.0f) ? ng : 0.0f;
            pk = zl_wave_max(pk);
            if ((threadIdx.x & 63) == 0 && pk > 0.0f) atomicMax(&A.reports[vfirst + i].peak_bits, __float_as_uint(pk));
        }
    }
}

// The staging pass of zl_k2_body below, as functions, for zl_k2_pair_body.  (zl_k2_body keeps its own text: calling these from it moved the
// register allocation of two existing kernels -- zl_k2_phase_render<2> gained a private segment -- and those kernels are to stay as they are.
// Compiled again since, so that nobody need repeat it: with zl_k2_body calling zl_k2_stage_load / _class / _chunks, 72 of the 99 kernels of
// this file change; zl_k2_phase_render<2> goes from 0 to 36 bytes of scratch; the headline kernel's SGPR spills go from 122 to 117, and
// zl_k_rt_loop<0, wide>'s from 402 to 338 with 20 -> 12 bytes of scratch.  K2 sits at the SGPR limit: any change to its text moves the allocation.)
// The record of voice vb + i in block kk (i >= nv: a slot behind the pass's last voice, which gets the neutral record); every load the record
// may need is issued at once.
// RUNS = false: a block that no inline run of the workgroup's voices reaches (k >= run_end, the word K1o leaves behind the order table,
// zl_order.h).  The run list -- 160 of the 240 bytes of a voice-block, every lane in cache lines of its own -- is not touched: cov is
// false, and dead_from comes from the dense copy in the table's tail (dead_tail[v], one coalesced load).  The rest is the same text.
template <bool RUNS>
static __device__ __forceinline__ void zl_k2_stage_load(const ZlBatch &A, int kk, int vb, int i, int nv, ZlVoiceConst &vc, ZlBlockPlan &pl, const int32_t *dead_tail)
{
    const int N = A.N, V = A.V;
    zl_plan_clear(pl);
    vc.src_offset = 0; vc.sample_duration = 0; vc.channels = 2;
    vc.lgain = vc.rgain = vc.clip_volume = vc.lpan = vc.rpan = vc.env = 0.0f; vc.pad[0] = vc.pad[1] = 0;
    if (i < nv) {
        vc = A.vconst[vb + i];                             // K1 leaves a neutral record for voices that do not play
        if (kk < A.K) {
            // zl_plan_lookup (implied by a run, explicit, or idle) with the run list AND the explicit record's header and first segment
            // fetched together: ONE memory round trip per prologue where "look at the runs, then fetch the record" is two in a row (most
            // blocks of a long window are explicit: a voice has ZL_MAXRUNS inline runs, a 2 s loop in a 43 s window restarts twenty times).
            // The record of a block that a run covers is never written: its bits lose every select below.
            const ZlRunList *rl = &A.runs[vb + i];
            const size_t pidx = (size_t)kk * V + (size_t)(vb + i);
            const ZlPlanHdr ph = A.plan_hdr[pidx];
            const ZlPlanSeg0 ps = A.plan_seg0[pidx];
            const int rn = RUNS ? rl->n : 0, dead = RUNS ? rl->dead_from : dead_tail[vb + i];
            bool cov = false; double rP = 0.0, rstep = 0.0; int rk0 = 0;
            if (RUNS) {
#pragma unroll
                for (int j = 0; j < ZL_MAXRUNS; ++j) {
                    const ZlRun r = rl->r[j];
                    const bool hit = !cov && j < rn && kk >= r.k0 && kk < r.k1;
                    rP = hit ? r.P : rP; rstep = hit ? r.step : rstep; rk0 = hit ? r.k0 : rk0;
                    cov = cov || hit;
                }
            }
            if (kk < dead) {
                pl.flags = cov ? (int32_t)ZL_PLAN_ACTIVE : ph.flags; pl.n_active = cov ? N : ph.n_active; pl.nseg = cov ? 1 : ph.nseg;
                pl.env = cov ? vc.env : ph.env;
                pl.P0 = cov ? fma((double)((kk - rk0) * N), rstep, rP) : ps.P0;   // exact: inside the linear run
                pl.step = cov ? rstep : ps.step;
                if (!cov && ((((ph.nseg >= 2 || (ph.flags & ZL_PLAN_ENV)) && !(ph.flags & ZL_PLAN_SLOW)) || (ph.flags & (ZL_PLAN_NOSLOT_SIM | ZL_PLAN_NOSLOT_EXPAND))))) {
                    const ZlPlanSeg1 s1 = A.plan_seg1[pidx];
                    pl.P1 = s1.P1; pl.step1 = s1.step1; pl.n1 = s1.n1; pl.estep0 = s1.estep0; pl.E1 = s1.E1; pl.estep1 = s1.estep1;
                }
            }
        }
    }
}

// ... and its class bits: 1 = plays this block, 2 = per-frame control, and the bits of the simple forms described inside
template <uint32_t MODE>
static __device__ __forceinline__ int zl_k2_stage_class(const ZlBatch &A, const ZlVoiceConst &vc, const ZlBlockPlan &pl)
{
    // 4 = "simple": whole block, sustain (and no debug trace); 8 = it has a second position segment; 16 = mono source; 32 = unit step;
    // 64 = "interior"; 128 = "on-grid": zl_k2_chunk_ongrid mixes it from one tap; 256 = "on-grid with one loop restart":
    // zl_k2_chunk_ongrid_pair_wrap mixes each frame from the first tap of its own segment.  The text is zl_render.h's, which K1c reads too
    // when it leaves the scalar records of a window (zl_k1c_scalar)
    return zl_voice_block_class(MODE, A.ongrid, A.trace, A.N, vc, pl);
}

// ... its ZlUnit: zl_unit_record's, and for a voice-block of class 256, whose record no chunk function reads (a chunk with a two-segment
// voice is never UNIT), alt = P1 - n1 in the place of alpha -- what zl_ongrid2_lane adds to a frame of the second segment.  An on-grid
// voice of one segment has alpha = +0.0f there, which reads as alt = 0.  zl_unit_record is shared with zl_k2_body and gets the class
// without bit 256: given a wider range of its argument, the compiler writes the `cls & 128` test of EVERY caller another way, and
// zl_k2_body's kernels are to keep their instructions.
template <uint32_t MODE>
static __device__ __forceinline__ ZlUnit zl_k2_stage_unit(const ZlBatch &A, const ZlVoiceConst &vc, const ZlBlockPlan &pl, int cls)
{
    ZlUnit un = zl_unit_record<MODE>(A, vc, pl, cls & 255);
    if (cls & 256) un.alt = (int)pl.P1 - pl.n1;
    return un;
}

// ... and the class of each chunk of U voices of the pass, from the classes of the wave's 64 voices (voice i of the pass = this lane's)
template <int U>
static __device__ __forceinline__ void zl_k2_stage_chunks(int cls, int i, int *s_chunk)
{
    // class of each chunk of U voices: OR of bits 1, 2, 8; 4 = every voice simple and of one source layout, 16 = all
    // mono (ballots over the wave's 64 voices)
    const unsigned long long m1 = __ballot(cls & 1), m2 = __ballot(cls & 2), m4 = __ballot(cls & 4), m8 = __ballot(cls & 8),
                             m16 = __ballot(cls & 16), m32 = __ballot(cls & 32), m64 = __ballot(cls & 64), m128 = __ballot(cls & 128);
    // 256 = every voice on-grid in either form (voice bits 128, 256), one source layout, and at least one voice with a loop restart
    const unsigned long long m256 = __ballot(cls & 256), many = __ballot(cls & 384);
    const int lane = i & 63;
    if (lane < 64 / U) {
        const unsigned long long full = (1ull << U) - 1ull;
        const int sh = lane * U;
        const unsigned long long mono = (m16 >> sh) & full;
        const int cc = (((m1 >> sh) & full) ? 1 : 0) | (((m2 >> sh) & full) ? 2 : 0) | (((m8 >> sh) & full) ? 8 : 0)
                     | (((((m4 >> sh) & full) == full) && (mono == 0 || mono == full)) ? 4 : 0) | (mono == full ? 16 : 0)
                     | ((((m32 >> sh) & full) == full) ? 32 : 0) | ((((m64 >> sh) & full) == full) ? 64 : 0) | ((((m128 >> sh) & full) == full) ? 128 : 0)
                     | (((((many >> sh) & full) == full) && ((m256 >> sh) & full) != 0 && (mono == 0 || mono == full)) ? 256 : 0);
        s_chunk[(i >> 6) * (64 / U) + lane] = cc;
    }
}

// BPW = blocks per workgroup.  Blocks shorter than 256 frames are rendered 256 / N at a time (BPW = 2 or 4: the 256
// threads are BPW groups of N frames), so the per-workgroup fixed costs -- launch, staging of the voice records -- are
// paid once per 256 frames whatever the block size is.  A wavefront never straddles two blocks (BPW > 1 only for N = 64 or 128).
// ST = the variant with LDS-staged source windows (zl_st_* above): its occupancy is set by the ring in LDS (2-3
// workgroups per CU), so it may take the registers of 3 waves per SIMD.
// (the body is a device function so that the persistent real-time kernel below can run it too: bx / by / bz / gdx / gdy stand for
// blockIdx.x / .y / .z and gridDim.x / .y of the batch launch)
// REPORTS: the workgroups of a call's last block also publish its per-voice reports (batch launches; the resident kernel has its own)
// ORD: launch slots are mapped through A.order (phase order, zl_k2_phase_render; one block per workgroup, register gathers)
template <uint32_t MODE, int BPW, bool ST, bool REPORTS = true, bool ORD = false>
static __device__ __forceinline__ void zl_k2_body(const ZlBatch &A, const unsigned bx, const unsigned by, const unsigned bz, const unsigned gdx, const unsigned gdy)
{
    constexpr int U = (MODE & ZL_MODE_HERMITE) ? ZL_K2_U_HERMITE : ZL_K2_U;
    // voice records staged per pass (the staged variant trades them for ring space; four 64-frame blocks per workgroup stage
    // 4 x the block records: 64 voices per pass keep the workgroup at 25 KB of LDS -- 5 workgroups per CU instead of 3 at 50 KB)
    constexpr int CH = ST ? ZL_ST_CHUNK : (BPW == 4 ? 64 : ZL_K2_CHUNK);
    __shared__ ZlWin s_win_[ST ? CH * 4 : 1];             // [voice][wave of the workgroup]
    __shared__ unsigned long long s_stmask_[ST ? BPW * (CH / 64) : 1];   // per block: which voices of the pass are staged
    __shared__ ZlBlockPlan  s_plan_[BPW][CH];
    __shared__ ZlVoiceConst s_vc[CH];
    __shared__ int s_cls_[BPW][CH];                   // per voice: 1 = plays this block, 2 = per-frame control
    __shared__ int s_chunk_[BPW][CH / U];             // class of each chunk of U voices
    __shared__ ZlUnit s_unit_[BPW][CH];
    __shared__ int   s_pk[2][ZL_K2_MAXNB][4];         // fused level scan: per-wave partial results of each of the workgroup's buses
    __shared__ float s_sq[2][ZL_K2_MAXNB][4];

    const int N = A.N, V = A.V;
    const int blk = (BPW > 1) ? (int)threadIdx.x / N : 0;          // which of the workgroup's blocks this lane renders
    const int f = (BPW > 1) ? (int)threadIdx.x - blk * N : (int)(bx * blockDim.x + threadIdx.x);   // frame inside the block
    // XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin in launch order, so launch slot y runs on XCD
    // y % 8; giving XCD x the contiguous blocks [x * KY / 8, (x + 1) * KY / 8) lets neighbouring blocks (which share the
    // cache line at their common edge of every source) meet in the same L2
    // Split tail (narrow buses, set by zl_launch_render): a launch ends when its last workgroups do, and those start one workgroup lifetime before
    // the end whatever the machine does meanwhile -- the launch's last blocks are therefore rendered by tail_split workgroups each, a few buses per
    // workgroup: a quarter of the lifetime, a quarter of the time the machine drains.  Slots [0, tail_from) are the blocks in front of them.
    const bool tailed = BPW == 1 && !ST && REPORTS && A.tail_from > 0;
    const bool inTail = tailed && (int)by >= A.tail_from;
    const int tj = inTail ? (int)by - A.tail_from : 0;
    const int ky = tailed ? A.tail_from : (int)gdy, xq = ky >> 3, xr = ky & 7, xx = (int)(by & 7u);
    const int ys = inTail ? A.tail_from + tj / A.tail_split
                          : xx * xq + (xx < xr ? xx : xr) + (int)(by >> 3);      // a bijection of [0, ky) for every ky
    // Phase order (A.order, K1o, zl_order.h): slot ys of z-slot bz renders block order[bz][ys] -- the blocks sorted by the loop phase
    // of the slot's key voice, so XCD x holds an eighth of the loop's phases and the repeats of one phase, which read the same
    // source lines, run together in its L2.  (The split tail exists only with one z-slot: bz == 0 there too.)
    static_assert(!ORD || (BPW == 1 && !ST && REPORTS), "the phase order is a batch launch of one block per workgroup");
    const int yb = ORD ? A.order[(size_t)bz * A.K + ys] : ys;
    const int k = yb * BPW + blk;
    const bool live = k < A.K;                                     // the last workgroup may hold fewer than BPW blocks
    const ZlBlockPlan *s_plan = s_plan_[blk];
    const int *s_cls = s_cls_[blk];
    const int *s_chunk = s_chunk_[blk];
    const ZlUnit *s_unit = s_unit_[blk];
    // Narrow buses (the reference's 8 voices per channel): one workgroup renders A.NB whole buses, one after the other,
    // from ONE staging pass over their NB * VPB <= 128 voices -- the gathers of consecutive buses keep flowing and the
    // fixed costs per workgroup are shared.  NB == 1: one (bus, mix group) per workgroup.
    const int NB = inTail ? A.tail_nb : A.NB;
    const int zz = inTail ? tj % A.tail_split : (int)bz;          // (a split tail exists only where one workgroup holds all the buses: bz == 0)
    const int bus0 = (NB > 1) ? zz * NB : zz / A.groups;
    const int g    = (NB > 1) ? 0 : zz - bus0 * A.groups;
    const int v0 = bus0 * A.VPB + g * A.G;
    const int vlim = (NB > 1) ? ((bus0 + NB) * A.VPB < V ? (bus0 + NB) * A.VPB : V) : (bus0 + 1) * A.VPB;
    const int v1 = (NB > 1) ? vlim : ((v0 + A.G < vlim) ? v0 + A.G : vlim);
    // the report covers the last block of the call (the same for every lane of a wave -- a wave is a 64-frame tile of one block --
    // and said so: the per-voice test is then a scalar branch instead of two vector instructions)
    const bool wantPeak = __builtin_amdgcn_readfirstlane((int)(live && (A.k0 + k == A.Ktot - 1))) != 0;
    // A block length that is no multiple of 64 (JACK periods of 16 or 32 frames, 441, 480 ...) leaves the last wave of a block with
    // lanes behind the block's end: they recompute the block's LAST frame -- every position, control word and tap they touch is
    // one a real frame touches -- and nothing of theirs is stored, scanned or reported (a duplicate of an existing value does not
    // move a maximum).  `f` below is the lane's own frame (stores, masks), `fc` the frame it computes.
    const int fc = f < N ? f : N - 1;
    const double fd = (double)fc;
#ifdef ZL_STAMPS
    unsigned long long zl_t0 = __builtin_amdgcn_s_memrealtime(), zl_t1 = 0, zl_paths = 0;
#endif

    float accL = 0.0f, accR = 0.0f;
    int curBus = bus0, busEnd = (bus0 + 1) * A.VPB;               // NB > 1: the bus being summed and its end in voice numbers

    // the finished mix of one bus (or mix group): bus row / partials row, and the fused AudioLevels block scan
    auto store_bus = [&](int bus) {
        float *outL, *outR;
        if (A.groups == 1) {
            const long long KN = (long long)A.Ktot * N;
            outL = A.bus + (long long)bus * (A.bus_stride ? A.bus_stride : 2 * KN) + (long long)(A.k0 + k) * N;
            outR = outL + (A.ch_stride ? A.ch_stride : KN);
        } else {
            outL = A.partials + ((((size_t)k * A.B + bus) * A.groups + g) * 2) * (size_t)N;
            outR = outL + N;
        }
        bool written = false;
        if (live) {
            if (MODE & ZL_MODE_FIX_DELAY) {
                written = f < N;
                if (written) { outL[f] = accL; outR[f] = accR; }
            } else {
                // quirk Q2: the reference pre-increments its output pointers, so frame f lands in out[f+1],
                // out[0] stays 0 and the sample of the last frame falls outside the buffer (dropped)
                written = f + 1 < N;
                if (written) { outL[f + 1] = accL; outR[f + 1] = accR; }
                if (f == 0)  { outL[0] = 0.0f;    outR[0] = 0.0f; }
            }
            if (A.host_out && A.groups == 1) {
                // offline bounce: the same samples once more, into the caller's page-locked host buffer (stores over PCIe; a wave's
                // 64 frames are 256 contiguous bytes per row), in the recorder's 16-bit format if asked (zl_pcm16)
                const size_t fo = (size_t)(A.host_k0 + A.k0 + k) * N;
                const int at = (MODE & ZL_MODE_FIX_DELAY) ? f : f + 1;
                if (A.host_fmt == 1) {
                    uint32_t *o = static_cast<uint32_t *>(A.host_out) + (size_t)bus * (size_t)A.host_total + fo;
                    if (at < N) __builtin_nontemporal_store((uint32_t)(uint16_t)zl_pcm16(accL) | ((uint32_t)(uint16_t)zl_pcm16(accR) << 16), o + at);
                    if (!(MODE & ZL_MODE_FIX_DELAY) && f == 0) __builtin_nontemporal_store(0u, o);
                } else {
                    float *oL = static_cast<float *>(A.host_out) + ((size_t)bus * 2) * (size_t)A.host_total + fo, *oR = oL + A.host_total;
                    if (at < N) { __builtin_nontemporal_store(accL, oL + at); __builtin_nontemporal_store(accR, oR + at); }
                    if (!(MODE & ZL_MODE_FIX_DELAY) && f == 0) { __builtin_nontemporal_store(0.0f, oL); __builtin_nontemporal_store(0.0f, oR); }
                }
            }
            if (A.fan && A.groups == 1) {
                // fused JackPassthrough fan-out of the finished bus (JackPassthrough.cpp:45-115): three more stereo pairs
                // written from the registers that hold the mix -- no second pass over the bus
                const size_t KN = (size_t)A.Ktot * N;
                const ZlPassParams pp = A.pass_inline ? A.pass0 : A.pass[bus];
                float *o = A.fan + ((size_t)bus * 6) * KN + (size_t)(A.k0 + k) * N;
                float lm, rm; zl_pass_pan(pp, lm, rm);
                const float amounts[3] = { pp.dry, pp.fx1, pp.fx2 };
                const int fo = (MODE & ZL_MODE_FIX_DELAY) ? f : f + 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ol, orr;
                    zl_pass_pair(pp, amounts[c], lm, rm, accL, accR, ol, orr);
                    if (fo < N) { o[(size_t)(2 * c) * KN + fo] = ol; o[(size_t)(2 * c + 1) * KN + fo] = orr; }
                    if (!(MODE & ZL_MODE_FIX_DELAY) && f == 0) {   // the bus holds 0 in frame 0 (Q2)
                        zl_pass_pair(pp, amounts[c], lm, rm, 0.0f, 0.0f, ol, orr);
                        o[(size_t)(2 * c) * KN] = ol; o[(size_t)(2 * c + 1) * KN] = orr;
                    }
                }
            }
        }
        // ---- fused AudioLevels block scan (AudioLevels.cpp:361-383) when this workgroup holds the final mix of its
        //      whole block(s) (no mix groups, one frame tile): saves the K3 launch and its re-read of the bus
        if (A.groups == 1 && (gdx == 1 || A.tile_accum) && A.levels) {
            const float aL = written ? accL : 0.0f, aR = written ? accR : 0.0f;      // (a lane without a frame of its own scans a zero)
            int pkL = zl_sample_to_peak_int(aL), pkR = zl_sample_to_peak_int(aR);
            float sqL = aL * aL, sqR = aR * aR;
            zl_wave_levels4(pkL, pkR, sqL, sqR);
            // each wave leaves its partial result of this bus; they are combined once, after the last bus (no barrier here)
            const int w = threadIdx.x >> 6, bi = bus - bus0;
            if ((threadIdx.x & 63) == 0) { s_pk[0][bi][w] = pkL; s_pk[1][bi][w] = pkR; s_sq[0][bi][w] = sqL; s_sq[1][bi][w] = sqR; }
        }
    };
    // the block levels of the workgroup's buses from the per-wave partial results: one lane per (bus, block)
    auto combine_levels = [&](int nbus) {
        if (!(A.groups == 1 && (gdx == 1 || A.tile_accum) && A.levels)) return;
        __syncthreads();
        for (int idx = threadIdx.x; idx < nbus * BPW; idx += blockDim.x) {
            const int bi = idx / BPW, b = idx - bi * BPW;
            const int kk = yb * BPW + b;
            if (kk >= A.K) continue;
            // the waves of block b: all of the workgroup's (BPW == 1) or N / 64 of them
            const int w0 = (BPW > 1) ? b * (N >> 6) : 0;
            const int nw = (BPW > 1) ? (N >> 6) : (int)((blockDim.x + 63) >> 6);
            ZlBlockLevels lv; lv.peak_l = 0; lv.peak_r = 0; lv.sumsq_l = 0.0f; lv.sumsq_r = 0.0f;
            // a later frame tile of a block this workgroup walks tile by tile: carry on from what this very lane stored after the tile before
            // (read past the vector L1: agent-scope loads)
            if (bx > 0) {
                ZlBlockLevels *pl = &A.levels[(size_t)kk * A.B + bus0 + bi];
                lv.peak_l = __hip_atomic_load(&pl->peak_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lv.peak_r = __hip_atomic_load(&pl->peak_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lv.sumsq_l = __hip_atomic_load(&pl->sumsq_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lv.sumsq_r = __hip_atomic_load(&pl->sumsq_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            for (int i = w0; i < w0 + nw; ++i) {
                lv.peak_l = s_pk[0][bi][i] > lv.peak_l ? s_pk[0][bi][i] : lv.peak_l;
                lv.peak_r = s_pk[1][bi][i] > lv.peak_r ? s_pk[1][bi][i] : lv.peak_r;
                lv.sumsq_l += s_sq[0][bi][i]; lv.sumsq_r += s_sq[1][bi][i];
            }
            A.levels[(size_t)kk * A.B + bus0 + bi] = lv;
        }
    };

    int vbase = v0;                                               // first voice of the staging pass under way
    // gathers issued ahead of a bus's epilogue (linear modes; with four taps they would be 64 registers)
    constexpr bool PF = !ST && !(MODE & ZL_MODE_HERMITE) && ZL_K2_PREFETCH_BUS;
    // after a chunk of U voices: if it held the last voice of a narrow bus (VPB is a multiple of the chunk size there), write that
    // bus and start the next one
    auto chunk_end = [&](int c) {
        if (NB > 1 && vbase + c + U == busEnd) {
            store_bus(curBus);
            accL = 0.0f; accR = 0.0f;
            ++curBus; busEnd += A.VPB;
        }
    };
    for (int vb = v0; vb < v1; vb += CH) {
        const int nv = (v1 - vb < CH) ? v1 - vb : CH;
        vbase = vb;
        // ---- stage the per-voice records of this pass in LDS: one lane per (block, voice) issues every load it may
        //      need at once (voice constants, run list; plan header + first segment when no run covers the block), so
        //      the prologue is one memory round trip (two for blocks with a second segment) and one barrier
        // (the barrier keeps a pass from overwriting records that another wave still reads: nothing to wait for before the FIRST pass of a
        // batch workgroup -- its first wave issues the staging loads while the others are still being launched; the resident kernel runs
        // this body once per cycle and keeps the barrier)
        if (!REPORTS || vb != v0) __syncthreads();
#ifdef ZL_STAMPS
        const unsigned long long zl_ta = __builtin_amdgcn_s_memrealtime();
        unsigned long long zl_tb = zl_ta;
#endif
        for (int idx = threadIdx.x; idx < BPW * CH; idx += blockDim.x) {   // whole waves: blockDim.x is a multiple of 64
            const int b = idx / CH, i = idx - b * CH;
            const int kk = yb * BPW + b;
            ZlVoiceConst vc;
            ZlBlockPlan pl;
            zl_plan_clear(pl);
            vc.src_offset = 0; vc.sample_duration = 0; vc.channels = 2;
            vc.lgain = vc.rgain = vc.clip_volume = vc.lpan = vc.rpan = vc.env = 0.0f; vc.pad[0] = vc.pad[1] = 0;
            if (i < nv) {
                vc = A.vconst[vb + i];                             // K1 leaves a neutral record for voices that do not play
                if (kk < A.K) {
                    // zl_plan_lookup (implied by a run, explicit, or idle) with the run list AND the explicit record's header and first segment
                    // fetched together: ONE memory round trip per prologue where "look at the runs, then fetch the record" is two in a row (most
                    // blocks of a long window are explicit: a voice has ZL_MAXRUNS inline runs, a 2 s loop in a 43 s window restarts twenty times).
                    // The record of a block that a run covers is never written: its bits lose every select below.
                    const ZlRunList *rl = &A.runs[vb + i];
                    const size_t pidx = (size_t)kk * V + (size_t)(vb + i);
                    const ZlPlanHdr ph = A.plan_hdr[pidx];
                    const ZlPlanSeg0 ps = A.plan_seg0[pidx];
                    const int rn = rl->n, dead = rl->dead_from;
                    bool cov = false; double rP = 0.0, rstep = 0.0; int rk0 = 0;
#pragma unroll
                    for (int j = 0; j < ZL_MAXRUNS; ++j) {
                        const ZlRun r = rl->r[j];
                        const bool hit = !cov && j < rn && kk >= r.k0 && kk < r.k1;
                        rP = hit ? r.P : rP; rstep = hit ? r.step : rstep; rk0 = hit ? r.k0 : rk0;
                        cov = cov || hit;
                    }
                    if (kk < dead) {
                        pl.flags = cov ? (int32_t)ZL_PLAN_ACTIVE : ph.flags; pl.n_active = cov ? N : ph.n_active; pl.nseg = cov ? 1 : ph.nseg;
                        pl.env = cov ? vc.env : ph.env;
                        pl.P0 = cov ? fma((double)((kk - rk0) * N), rstep, rP) : ps.P0;   // exact: inside the linear run
                        pl.step = cov ? rstep : ps.step;
                        if (!cov && ((((ph.nseg >= 2 || (ph.flags & ZL_PLAN_ENV)) && !(ph.flags & ZL_PLAN_SLOW)) || (ph.flags & (ZL_PLAN_NOSLOT_SIM | ZL_PLAN_NOSLOT_EXPAND))))) {
                            const ZlPlanSeg1 s1 = A.plan_seg1[pidx];
                            pl.P1 = s1.P1; pl.step1 = s1.step1; pl.n1 = s1.n1; pl.estep0 = s1.estep0; pl.E1 = s1.E1; pl.estep1 = s1.estep1;
                        }
                    }
                }
            }
#ifdef ZL_STAMPS
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            zl_tb = __builtin_amdgcn_s_memrealtime();
#endif
            int cls = (pl.flags & ZL_PLAN_ACTIVE) ? (1 | ((pl.flags & ZL_PLAN_SLOW) ? 2 : 0)) : 0;
            // 4 = "simple": whole block, sustain (and no debug trace); 8 = it has a second position segment; 16 = mono source
            const float gprod = vc.lgain * vc.rgain * vc.clip_volume * pl.env;     // finite iff every factor is (or one is 0 * inf = NaN)
            // (sources of 4 GiB and more take the general path: the simple paths address a source with 32-bit byte offsets)
            if (cls == 1 && pl.nseg <= 2 && !(pl.flags & ZL_PLAN_ENV) && pl.n_active == N && (vc.channels == 1 || vc.channels == 2) && !A.trace
                && (gprod - gprod) == 0.0f && (uint32_t)vc.sample_duration < 0x1ffffff0u)
            {
                // 64 = "interior": first and last position of the block (P0 and P0 + (N-1) step, step > 0) leave room for
                // every tap: pos + 1 <= duration (pos >= 1 and pos + 2 <= duration with 4 taps)
                constexpr bool HM = (MODE & ZL_MODE_HERMITE) != 0;
                const double Pmax = fma((double)(N - 1), pl.step, pl.P0);
                const bool interior = pl.nseg == 1 && pl.P0 >= (HM ? 1.0 : 0.0) && Pmax < (double)(vc.sample_duration - (HM ? 1 : 0));
                cls |= 4 | (pl.nseg == 2 ? 8 : 0) | (vc.channels == 1 ? 16 : 0) | ((pl.nseg == 1 && pl.step == 1.0 && pl.P0 < 1073741824.0) ? 32 : 0)
                     | (interior ? 64 : 0);
                // 128 = "on-grid": a unit-step interior block from an integer position of a source known to be finite -- alpha = 0 in
                // every frame, the second tap only adds a signed zero (zl_render.h): zl_k2_chunk_ongrid mixes it from one tap
                cls |= zl_voice_ongrid(MODE, A.ongrid, true, (cls & 32) != 0, interior, pl.P0, pl.step, vc.pad[0]) ? 128 : 0;
            }
            if (ST) {
                // windows of the block's waves (BPW == 1: the workgroup's four frame tiles; else the N / 64 waves of block b).
                // Staged: an interior stereo voice on one line whose window fits a slot for every wave.
                constexpr int WPB = 4 / BPW;
                constexpr int TB = (MODE & ZL_MODE_HERMITE) ? 1 : 0, TA = (MODE & ZL_MODE_HERMITE) ? 2 : 1;
                const bool cand = (cls & (4 | 8 | 16 | 64)) == (4 | 64) && (uint32_t)vc.sample_duration < 0x0ffffff0u;
                int a[WPB], n16[WPB];
                bool fits = cand;
#pragma unroll
                for (int w = 0; w < WPB; ++w) {
                    const int f0 = (BPW > 1) ? 64 * w : (int)bx * 256 + 64 * w;
                    const int first = (int)fma((double)f0, pl.step, pl.P0) - TB, last = (int)fma((double)(f0 + 63), pl.step, pl.P0) + TA;
                    a[w] = first & ~1;                             // even frame = 16-byte aligned in the arena
                    n16[w] = (last - a[w] + 2) >> 1;               // 16-byte pieces covering frames [a, last]
                    fits = fits && n16[w] >= 1 && n16[w] <= ZL_ST_SLOT / 16;
                }
#pragma unroll
                for (int w = 0; w < WPB; ++w) { ZlWin wn; wn.a = fits ? a[w] : 0; wn.n16 = fits ? n16[w] : 0; s_win_[i * 4 + b * WPB + w] = wn; }
                const unsigned long long fm = __ballot(fits);      // the wave's 64 voices are one block's voices [64 m, 64 m + 64)
                if ((i & 63) == 0) s_stmask_[b * (CH / 64) + (i >> 6)] = fm;
            }
            s_unit_[b][i] = zl_unit_record<MODE>(A, vc, pl, cls);
            if (b == 0) s_vc[i] = vc;
            s_plan_[b][i] = pl;                   // idle slots: a harmless record with no active frame
            s_cls_[b][i] = cls;
            // class of each chunk of U voices: OR of bits 1, 2, 8; 4 = every voice simple and of one source layout, 16 = all
            // mono (ballots over the wave's 64 voices)
            const unsigned long long m1 = __ballot(cls & 1), m2 = __ballot(cls & 2), m4 = __ballot(cls & 4), m8 = __ballot(cls & 8),
                                     m16 = __ballot(cls & 16), m32 = __ballot(cls & 32), m64 = __ballot(cls & 64), m128 = __ballot(cls & 128);
            const int lane = i & 63;
            if (lane < 64 / U) {
                const unsigned long long full = (1ull << U) - 1ull;
                const int sh = lane * U;
                const unsigned long long mono = (m16 >> sh) & full;
                const int cc = (((m1 >> sh) & full) ? 1 : 0) | (((m2 >> sh) & full) ? 2 : 0) | (((m8 >> sh) & full) ? 8 : 0)
                             | (((((m4 >> sh) & full) == full) && (mono == 0 || mono == full)) ? 4 : 0) | (mono == full ? 16 : 0)
                             | ((((m32 >> sh) & full) == full) ? 32 : 0) | ((((m64 >> sh) & full) == full) ? 64 : 0) | ((((m128 >> sh) & full) == full) ? 128 : 0);
                s_chunk_[b][(i >> 6) * (64 / U) + lane] = cc;
            }
        }
        __syncthreads();
#ifdef ZL_STAMPS
        zl_t1 = __builtin_amdgcn_s_memrealtime();
        zl_paths = ((zl_ta - zl_t0) & 0xffffull) | (((zl_tb - zl_t0) & 0xffffull) << 16);   // prologue break-down: first barrier, loads landed (10 ns ticks)
#endif
        const size_t pbase = (size_t)k * V + vb;
        if (ST) {
            // ---- LDS-staged pass: the wave's ring runs ZL_ST_D voices ahead of its compute.  Voice j of the pass owns slot j mod
            //      ZL_ST_D.  Before the step over voices [c0, c0 + US) everything up to voice c0 + US - 1 must have landed: at most
            //      the D - US youngest DMAs (voices c0 + US .. c0 + D - 1) may be outstanding.  Voices that are not staged (loop
            //      ends, events, mono, ...) take a one-lane dummy DMA so that the count stays uniform, and are rendered by the
            //      general single-voice path -- in voice order, as always.  A step's wave-uniform inputs (the next voices'
            //      parameters, the next DMAs' addresses) are read one step ahead, into registers.
            constexpr int D = ZL_ST_D, US = ZL_ST_U;
            static_assert(D % US == 0 && D > US && D <= 60 && 8 % US == 0, "ring shape");
            const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            const char *ring = zl_dyn_lds + wave * (D * ZL_ST_SLOT);
            const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)zl_lds_addr(ring));
            const ZlWin *s_win = s_win_ + wave;                    // entry of voice i: s_win[i * 4]
            const uint32_t lane16 = (threadIdx.x & 63u) << 4;
            unsigned long long stm[CH / 64];
#pragma unroll
            for (int m = 0; m < CH / 64; ++m) {
                const unsigned long long x = s_stmask_[blk * (CH / 64) + m];
                stm[m] = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)x);
            }
            const int nvR = (nv + US - 1) / US * US;
            for (int j = 0; j < D && j < nv; ++j) {
                const ZlStDma d = zl_st_dma(A, s_vc, s_win, j, lane16);
                zl_glds_piece(d.g, lane16, d.nbytes, ring_lds + (uint32_t)j * ZL_ST_SLOT);
            }
            // parameters in two register sets that swap roles every step (no copies); the per-voice DMA descriptors likewise
            ZlStParams pa[US], pb[US];
#pragma unroll
            for (int u = 0; u < US; ++u) pa[u] = zl_st_params(s_plan, s_vc, s_win, u);           // (records of idle slots are harmless)
            int slot0 = 0;
            // one step over voices [c0, c0 + US): `cur` was read one step ago, `nxt` is read now for the following step
            auto step = [&](int c0, const ZlStParams (&cur)[US], ZlStParams (&nxt)[US]) {
                if (c0 + D < nv) zl_wait_vm<D - US>(); else zl_wait_vm<0>();     // (past that point nothing more is issued)
                const unsigned long long mw = (CH > 64 && c0 >= 64) ? stm[(CH / 64) - 1] : stm[0];
                const unsigned sm = (unsigned)(mw >> (c0 & 63)) & ((1u << US) - 1u);
                int slot[US];
#pragma unroll
                for (int u = 0; u < US; ++u) { slot[u] = slot0 + u; slot[u] -= slot[u] >= D ? D : 0; }
                ZlStDma dma[US];
                if (sm == (1u << US) - 1u) {
                    ZlStTaps t[US];
#pragma unroll
                    for (int u = 0; u < US; ++u) t[u] = zl_st_taps<MODE>(cur[u], ring, slot[u], fd);
                    // one step ahead, while the taps travel: the next voices' parameters and the next DMAs' addresses
#pragma unroll
                    for (int u = 0; u < US; ++u) {
                        nxt[u] = zl_st_params(s_plan, s_vc, s_win, c0 + US + u < CH ? c0 + US + u : CH - 1);
                        dma[u] = zl_st_dma(A, s_vc, s_win, c0 + D + u < CH ? c0 + D + u : CH - 1, lane16);
                    }
                    zl_f2 acc = {accL, accR};
#ifdef ZL_ST_DIAG_NOMIX     // timing-only diagnostic build: taps are read, nothing is computed
#pragma unroll
                    for (int u = 0; u < US; ++u) acc += t[u].xm + t[u].x2;
#else
#pragma unroll
                    for (int u = 0; u < US; ++u) zl_st_mix<MODE>(A, cur[u], t[u], vb + c0 + u, wantPeak, acc);
#endif
                    accL = acc.x; accR = acc.y;
                } else {
#pragma unroll
                    for (int u = 0; u < US; ++u) {
                        const int i = c0 + u;
                        if (i < nv) {
                            const int cl = __builtin_amdgcn_readfirstlane(s_cls[i]);
                            if ((sm >> u) & 1u) {
                                const ZlStTaps t = zl_st_taps<MODE>(cur[u], ring, slot[u], fd);
                                zl_f2 ac = {accL, accR};
                                zl_st_mix<MODE>(A, cur[u], t, vb + i, wantPeak, ac);
                                accL = ac.x; accR = ac.y;
                            } else if (cl == 0) { }                                                       // idle (SamplerSynth.cpp:137)
                            else if (cl & 2) zl_k2_chunk<MODE, true, 1>(A, s_plan, s_vc, s_cls, i, pbase, vb, fc, wantPeak, accL, accR);
                            else zl_k2_chunk<MODE, false, 1>(A, s_plan, s_vc, s_cls, i, pbase, vb, fc, wantPeak, accL, accR);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < US; ++u) {
                        nxt[u] = zl_st_params(s_plan, s_vc, s_win, c0 + US + u < CH ? c0 + US + u : CH - 1);
                        dma[u] = zl_st_dma(A, s_vc, s_win, c0 + D + u < CH ? c0 + D + u : CH - 1, lane16);
                    }
                }
                if (NB > 1 && vb + c0 + US == busEnd) {
                    // that step held the last voice of a bus (bus widths are multiples of 8 and US divides 8): write it, start the next
                    store_bus(curBus);
                    accL = 0.0f; accR = 0.0f;
                    ++curBus; busEnd += A.VPB;
                }
#pragma unroll
                for (int u = 0; u < US; ++u)
                    if (c0 + D + u < nv) zl_glds_piece(dma[u].g, lane16, dma[u].nbytes, ring_lds + (uint32_t)slot[u] * ZL_ST_SLOT);
                slot0 += US; slot0 -= slot0 >= D ? D : 0;
            };
            for (int c0 = 0; c0 < nvR; c0 += 2 * US) {
                step(c0, pa, pb);
                if (c0 + US < nvR) step(c0 + US, pb, pa);
            }
        } else
        for (int c0 = 0; c0 < nv; ) {
            // (no voice is on-grid in the Hermite and FIX_GAIN modes, zl_voice_ongrid: their kernels do not carry the chunk)
            constexpr bool OG = (MODE & (ZL_MODE_HERMITE | ZL_MODE_FIX_GAIN)) == 0;
            const int cc = __builtin_amdgcn_readfirstlane(s_chunk[c0 / U]);
            if (cc == 0) {                                        // nobody in this chunk plays (SamplerSynth.cpp:137)
            } else if (OG && (cc & 132) == 132) {
                // every voice of the chunk on-grid (which implies simple, unit, interior) and of one source layout
                // (ZL_K2_U_ONGRID = 2 U: two such chunks in a row, inside one bus, go as one -- twice the loads in flight)
                const int cn = (ZL_K2_U_ONGRID > U && c0 + 2 * U <= nv && !(NB > 1 && vbase + c0 + U == busEnd))
                                   ? __builtin_amdgcn_readfirstlane(s_chunk[c0 / U + 1]) : 0;
                if (ZL_K2_U_ONGRID > U && (cn & 132) == 132 && ((cn ^ cc) & 16) == 0) {
                    if (wantPeak)     zl_k2_ongrid_dispatch<2 * U, true>(A, s_vc, s_unit, c0, vb, fc, (cc & 16) != 0, accL, accR);
                    else              zl_k2_ongrid_dispatch<2 * U, false>(A, s_vc, s_unit, c0, vb, fc, (cc & 16) != 0, accL, accR);
                    c0 += U;
                }
                else if (wantPeak)    zl_k2_ongrid_dispatch<U, true>(A, s_vc, s_unit, c0, vb, fc, (cc & 16) != 0, accL, accR);
                else                  zl_k2_ongrid_dispatch<U, false>(A, s_vc, s_unit, c0, vb, fc, (cc & 16) != 0, accL, accR);
            } else if ((cc & 124) == 100) {
                // (the shared-tap form needs a wave's lanes to be consecutive frames of one block: true for every launch shape --
                // a wave is a 64-frame tile of its block)
                if (ZL_K2_UNIT_SHARE) zl_k2_chunk_unit_shared<MODE, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, wantPeak, accL, accR);
                else zl_k2_chunk_simple<MODE, false, true, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            }
            else if ((cc & 92) == 68)   zl_k2_chunk_simple<MODE, false, false, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 28) == 4)    zl_k2_chunk_simple<MODE, false, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 20) == 4)    zl_k2_chunk_simple<MODE, true, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 124) == 116) zl_k2_chunk_simple_mono<MODE, false, true, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 92) == 84)   zl_k2_chunk_simple_mono<MODE, false, false, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 28) == 20)   zl_k2_chunk_simple_mono<MODE, false, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else if ((cc & 20) == 20)   zl_k2_chunk_simple_mono<MODE, true, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
            else {
                // general chunks (events, second segments, mixed layouts, per-frame control) are rare: run them as
                // two half-chunks so their extra per-voice registers do not set the kernel's register budget
                constexpr int H = U / 2;
                for (int h = 0; h < U; h += H) {
                    if (cc & 2) zl_k2_chunk<MODE, true, H>(A, s_plan, s_vc, s_cls, c0 + h, pbase, vb, fc, wantPeak, accL, accR);
                    else        zl_k2_chunk<MODE, false, H>(A, s_plan, s_vc, s_cls, c0 + h, pbase, vb, fc, wantPeak, accL, accR);
                }
            }
            // narrow buses: the chunk that ends a bus is followed by that bus's epilogue (store, level scan: ~100 instructions in a
            // dependent chain).  The NEXT bus's gathers go out first -- they travel while the epilogue runs -- when its first chunk is
            // of the steady-state kind (stereo, interior, one segment); with the reference's 8 voices per bus this inner loop walks
            // all the workgroup's buses.  (The taps in flight live only inside this loop: no register is held for them elsewhere.)
            while (PF && NB > 1 && vbase + c0 + U == busEnd && c0 + U < nv) {
                const int nc = __builtin_amdgcn_readfirstlane(s_chunk[c0 / U + 1]);
                const bool unit = (nc & 124) == 100;
                if (!unit && (nc & 92) != 68) break;
                ZlSimpleTaps<(MODE & ZL_MODE_HERMITE) != 0, U> pf;
                if (unit) zl_k2_simple_issue<MODE, false, true, true, U>(A, s_plan, s_vc, s_unit, c0 + U, fc, fd, pf);
                else      zl_k2_simple_issue<MODE, false, false, true, U>(A, s_plan, s_vc, s_unit, c0 + U, fc, fd, pf);
                chunk_end(c0);
                c0 += U;
                zl_k2_simple_mix<MODE, true, U>(A, s_plan, s_vc, s_unit, c0, vb, wantPeak, pf, accL, accR);
            }
            chunk_end(c0);
            c0 += U;
        }
    }

#ifdef ZL_STAMPS
    if (threadIdx.x == 0 && A.pos_trace) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(A.pos_trace) + 4 * ((size_t)bz * gdy + by);
        st[0] = zl_t0; st[1] = zl_t1; st[2] = __builtin_amdgcn_s_memrealtime();
        st[3] = zl_paths;
    }
#endif
    if (NB == 1) { store_bus(bus0); combine_levels(1); }
    else combine_levels(curBus - bus0);

    // ---- the call's reports (zl_k_reports' work), by the workgroups that hold the call's last block: this workgroup summed its buses
    //      whole, so its voices' peaks are complete once its own waves have issued their atomics (the barrier waits for them)
    if (REPORTS && A.fused_reports) {
        const int klast = A.Ktot - 1 - A.k0;                      // the call's last block in this window's numbering (uniform)
        if (klast >= 0 && klast < A.K && klast >= yb * BPW && klast < yb * BPW + BPW) {
            __syncthreads();
            for (int v = v0 + (int)threadIdx.x; v < v1; v += (int)blockDim.x) {
                // (a report is two 16-byte words: {playing, valid, peak bits, progress} {clip, pad, position}; the peak is read past the vector L1)
                const uint4 *src = reinterpret_cast<const uint4 *>(&A.reports[v]);
                uint4 a = src[0];
                const uint4 b = src[1];
                a.z = __hip_atomic_load(&A.reports[v].peak_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const float gn = __uint_as_float(a.z) * 0.5f;
                A.rep_gain[v] = gn;
                if (A.rep_host) { uint4 *dst = reinterpret_cast<uint4 *>(&A.rep_host[v]); dst[0] = a; dst[1] = b; A.rep_host_gain[v] = gn; }
            }
            if (bus0 == 0 && g == 0 && threadIdx.x == 0 && A.rep_host_stats) {
                const unsigned long long sb = A.stats->source_bytes, sl = A.stats->slow_blocks, af = A.stats->active_frames;
                A.rep_host_stats->source_bytes = sb; A.rep_host_stats->slow_blocks = sl; A.rep_host_stats->active_frames = af;
                A.stats->source_bytes = 0; A.stats->slow_blocks = 0; A.stats->active_frames = 0;   // cleared for the call that reuses this slot
            }
        }
    }
}

// the kernel: one workgroup = one (bus or group of narrow buses, mix group, block or BPW short blocks, frame tile)
// (faithful linear mode, one block per workgroup -- the headline shape: ZL_K2_WAVES_LINEAR = 5 waves per SIMD, which is what the LDS
// cap of the launch allows anyway.  Two 128-frame blocks per workgroup: 5 waves -- what its 28.8 KB of
// LDS allow -- instead of the 4 its 104 registers give: +2..3 % with 10 spilled registers, profiles/round2_e_k2_experiments.txt;
// four 64-frame blocks: likewise 5, with 64 voices per staging pass)
// (linear FIX_DELAY, one block per workgroup: the same 5 -- the allocator, left alone, takes 100 registers for the straight-line on-grid chunk
// and the kernel would fall from the 5 waves its LDS allows, and had, to 4)
template <uint32_t MODE, int BPW, bool ST>
__global__ void __launch_bounds__(256, ST ? 3 : (MODE & (ZL_MODE_HERMITE | ZL_MODE_FIX_DELAY)) == 0 ? (BPW == 1 ? ZL_K2_WAVES_LINEAR : 5)
                                              : ((MODE & ZL_MODE_HERMITE) == 0 && BPW == 1) ? ZL_K2_WAVES_LINEAR : ZL_K2_MINWAVES) zl_k2_render(const ZlBatch A)
{
    zl_k2_body<MODE, BPW, ST>(A, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y);
}

// the same render with the window's blocks in phase order (A.order, K1o).  A kernel of its own: the table's block number is one more
// scalar held through the whole body (SGPR spills 111 -> 115, all of them to VGPR lanes: the compiler reserves 36 bytes of private
// segment that no instruction touches), and launches without the order stay the kernel they were.
template <uint32_t MODE>
__global__ void __launch_bounds__(256, (MODE & ZL_MODE_HERMITE) == 0 ? ZL_K2_WAVES_LINEAR : ZL_K2_MINWAVES) zl_k2_phase_render(const ZlBatch A)
{
    zl_k2_body<MODE, 1, false, true, true>(A, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y);
}

// ------------------------------------------------------------------------------------------------
// K2 with TWO frames per lane (zl_k2_pair_render / zl_k2_pair_phase_render): the launches zl_pair_shape (zl_pair.h) lets through -- faithful
// linear mode, blocks of 256 frames, one bus per workgroup, no mix groups, no fan-out, no bounce, no trace, batches.  A workgroup is 128
// lanes; lane j renders frames 2 j and 2 j + 1 of its block.  What it buys is the on-grid chunk (zl_k2_chunk_ongrid_pair): the texture
// addresser's cost is per load instruction and lane whatever the width (profiles/round6_ongrid_pmc.txt), and this form issues half of
// them.  Every other chunk class runs through the one-frame chunk functions, once per frame of the lane -- the same operands in the same
// order, each frame into its own accumulator pair -- in a loop that is not unrolled: those chunks are rare (blocks at a loop's ends,
// envelopes, pitched voices) and cost what they cost in zl_k2_body.  Staging, store (Q2), level scan and reports are zl_k2_body's:
// the scan's defined order is kept by zl_wave_levels4_pair, a wave leaving the partial results of two 64-frame tiles.
#ifndef ZL_K2_PAIR_WAVES
// waves per SIMD the launch reaches: 8 two-wave workgroups per CU (the LDS cap of zl_launch_render), each wave with twice the
// bytes in flight of a zl_k2_body wave
#define ZL_K2_PAIR_WAVES 4
#endif
#define ZL_K2_PAIR_LDS 18432   // LDS per workgroup the launch pads to: 8 workgroups and the planner's 12 KB fit a CU's 160 KB, a ninth does not

// THE FAST WORKGROUP (ZL_K2_PAIR_SCALAR; the records: zl_render.h, written by K1c's zl_k1c_assemble).  Everything zl_k2_chunk_ongrid_pair reads of a
// voice is wave-uniform -- the address of the block's frame 0 and the pan pair -- so a workgroup whose bus is on-grid in every chunk of its
// block does not stage at all: no per-lane record loads, no class, no LDS records, no barrier, no v_readfirstlane.  Per chunk of 8 voices ONE
// scalar load brings the eight addresses (16 SGPRs) and one the eight pan pairs; the source loads take the SGPR pair as their scalar base and
// the packed multiply takes the pan pair from SGPRs.  The addresses of chunk c + 1 are asked for behind the source loads of chunk c, so a miss
// on the streamed table waits behind them.  The loads, the order of the voices and the mix are zl_k2_chunk_ongrid_pair's: the same bits.
// Scalar LOADS only; nothing is written through the scalar path.
typedef uint64_t zl_u64x8 __attribute__((ext_vector_type(8)));
typedef float zl_f16 __attribute__((ext_vector_type(16)));
#define ZL_CONST_AS __attribute__((address_space(4)))
// (lpan m, rpan m) with the pan pair in SGPRs
static __device__ __forceinline__ zl_f2 zl_pk_pan_s(zl_f2 pan, zl_f2 ms)
{
    zl_f2 r; asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "s"(pan), "v"(ms)); return r;
}
// zl_mix_acc_ongrid_pk with that multiply: the same five operations on the same operands
template <int SEL>
static __device__ __forceinline__ void zl_mix_acc_ongrid_pk_s(zl_f2 &acc, zl_f2 x, zl_f2 pan)
{
    zl_f2 ms = SEL == 0 ? zl_pk_sumdiff(x) : SEL == 1 ? zl_pk_sumdiff_lo(x) : zl_pk_sumdiff_hi(x);
    ms.x = 0.5f * ms.x;                                           // :208
    acc = zl_pk_add(acc, zl_pk_side(zl_pk_pan_s(pan, ms), ms));   // :210-211, :218-221 (index shift applied at the store)
}
// addr = the addr0 words of the bus's first voice in this block, pan = its pan word; nch chunks of 8 voices, all of one layout
template <bool MONO>
static __device__ __forceinline__ void zl_k2_pair_fast(const uint64_t *addr, const uint64_t *pan, int nch, int f0,
                                                       float &accL0, float &accR0, float &accL1, float &accR1)
{
    constexpr int U = 8;
    const ZL_CONST_AS zl_u64x8 *at = reinterpret_cast<const ZL_CONST_AS zl_u64x8 *>(reinterpret_cast<uintptr_t>(addr));
    const ZL_CONST_AS zl_f16 *pt = reinterpret_cast<const ZL_CONST_AS zl_f16 *>(reinterpret_cast<uintptr_t>(pan));
    zl_f2 acc0 = {accL0, accR0}, acc1 = {accL1, accR1};
    zl_u64x8 a = at[0];
    for (int c = 0; c < nch; ++c) {
        zl_f4a8 d4[MONO ? 1 : U];
        zl_f2   d2[MONO ? U : 1];
        const uint32_t ob = zl_k2_ongrid_offset((uint32_t)f0 << (MONO ? 2 : 3));   // interior: frames ipos + f0 and ipos + f0 + 1 are inside the source
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (MONO) d2[u] = zl_k2_ongrid_load<zl_f2a4b>(a[u], ob);
            else      d4[u] = zl_k2_ongrid_load<zl_f4a8>(a[u], ob);
        }
        const zl_f16 p = pt[c];
        a = at[c + 1 < nch ? c + 1 : c];                          // the next chunk's addresses, behind this chunk's source loads
        __builtin_amdgcn_sched_barrier(0);                        // (all loads in flight before the first mix, as in zl_k2_chunk_ongrid_pair)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const zl_f2 pu = {p[2 * u], p[2 * u + 1]};
            if (MONO) {
                zl_mix_acc_ongrid_pk_s<1>(acc0, d2[u], pu);
                zl_mix_acc_ongrid_pk_s<2>(acc1, d2[u], pu);
            } else {
                zl_mix_acc_ongrid_pk_s<0>(acc0, __builtin_shufflevector(d4[u], d4[u], 0, 1), pu);
                zl_mix_acc_ongrid_pk_s<0>(acc1, __builtin_shufflevector(d4[u], d4[u], 2, 3), pu);
            }
        }
    }
    accL0 = acc0.x; accR0 = acc0.y; accL1 = acc1.x; accR1 = acc1.y;
}
// THE TWO-SLOT WALK (ZL_K2_PAIR_LAPS; zl_launch.h): a workgroup that holds two neighbouring slots of its bus's phase order renders both blocks in
// one pass over the voices.  Neighbours in the phase order read, voice for voice, nearly the same source lines (the key voice's windows lie less
// than a bucket apart), and each re-read of a line by another workgroup is a fresh L2-to-L1 transfer: here block B's load of voice u is issued
// directly behind block A's, so it finds A's lines in, or on their way into, this CU's L1.  Four voices per step: 2 x 4 addresses, 2 x 4 next
// addresses and 4 pan pairs in SGPRs, eight source loads in flight as in zl_k2_pair_fast.  Each block mixes its voices in voice order into its own
// accumulator pairs through zl_mix_acc_ongrid_pk_s: the operations, operands and bits of zl_k2_pair_fast.  nst = steps of 4 voices.
typedef uint64_t zl_u64x4 __attribute__((ext_vector_type(4)));
typedef float zl_f8 __attribute__((ext_vector_type(8)));
template <bool MONO>
static __device__ __forceinline__ void zl_k2_pair_fast2(const uint64_t *addrA, const uint64_t *addrB, const uint64_t *pan, int nst, int f0,
                                                        float (&accA)[4], float (&accB)[4])
{
    constexpr int U = 4;
    const ZL_CONST_AS zl_u64x4 *atA = reinterpret_cast<const ZL_CONST_AS zl_u64x4 *>(reinterpret_cast<uintptr_t>(addrA));
    const ZL_CONST_AS zl_u64x4 *atB = reinterpret_cast<const ZL_CONST_AS zl_u64x4 *>(reinterpret_cast<uintptr_t>(addrB));
    const ZL_CONST_AS zl_f8 *pt = reinterpret_cast<const ZL_CONST_AS zl_f8 *>(reinterpret_cast<uintptr_t>(pan));
    zl_f2 a0 = {accA[0], accA[1]}, a1 = {accA[2], accA[3]}, b0 = {accB[0], accB[1]}, b1 = {accB[2], accB[3]};
    zl_u64x4 aA = atA[0], aB = atB[0];
    for (int c = 0; c < nst; ++c) {
        zl_f4a8 dA4[MONO ? 1 : U], dB4[MONO ? 1 : U];
        zl_f2   dA2[MONO ? U : 1], dB2[MONO ? U : 1];
        const uint32_t ob = zl_k2_ongrid_offset((uint32_t)f0 << (MONO ? 2 : 3));   // interior in both blocks (each passed the fast gate)
#pragma unroll
        for (int u = 0; u < U; ++u) {                             // A's and B's load of a voice adjacent in program order: that is the point
            if (MONO) { dA2[u] = zl_k2_ongrid_load<zl_f2a4b>(aA[u], ob); dB2[u] = zl_k2_ongrid_load<zl_f2a4b>(aB[u], ob); }
            else      { dA4[u] = zl_k2_ongrid_load<zl_f4a8>(aA[u], ob);  dB4[u] = zl_k2_ongrid_load<zl_f4a8>(aB[u], ob); }
        }
        const zl_f8 p = pt[c];
        const int cn = c + 1 < nst ? c + 1 : c;
        aA = atA[cn]; aB = atB[cn];                               // the next step's addresses, behind this step's source loads
        __builtin_amdgcn_sched_barrier(0);                        // (all loads in flight before the first mix, as in zl_k2_pair_fast)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const zl_f2 pu = {p[2 * u], p[2 * u + 1]};
            if (MONO) {
                zl_mix_acc_ongrid_pk_s<1>(a0, dA2[u], pu);
                zl_mix_acc_ongrid_pk_s<2>(a1, dA2[u], pu);
                zl_mix_acc_ongrid_pk_s<1>(b0, dB2[u], pu);
                zl_mix_acc_ongrid_pk_s<2>(b1, dB2[u], pu);
            } else {
                zl_mix_acc_ongrid_pk_s<0>(a0, __builtin_shufflevector(dA4[u], dA4[u], 0, 1), pu);
                zl_mix_acc_ongrid_pk_s<0>(a1, __builtin_shufflevector(dA4[u], dA4[u], 2, 3), pu);
                zl_mix_acc_ongrid_pk_s<0>(b0, __builtin_shufflevector(dB4[u], dB4[u], 0, 1), pu);
                zl_mix_acc_ongrid_pk_s<0>(b1, __builtin_shufflevector(dB4[u], dB4[u], 2, 3), pu);
            }
        }
    }
    accA[0] = a0.x; accA[1] = a0.y; accA[2] = a1.x; accA[3] = a1.y;
    accB[0] = b0.x; accB[1] = b0.y; accB[2] = b1.x; accB[3] = b1.y;
}
// May the workgroup of (block k, voices [v0, v1)) take it?  Every chunk bit of its voices set, and one layout for the whole bus (a bus of
// mono and stereo chunks stages: the walk is compiled once per layout).  1 = stereo, 2 = mono, 0 = no.  Scalar loads of 16-bit entries, two to a word.
static __device__ __forceinline__ int zl_k2_pair_fast_kind(const uint64_t *tab, int K, int V, int k, int v0, int v1)
{
    const ZL_CONST_AS uint32_t *bw = reinterpret_cast<const ZL_CONST_AS uint32_t *>(reinterpret_cast<uintptr_t>(tab + zl_pair_tab_fast(K, V)));
    const int G = (V + 63) / 64;
    bool all = true, anyMono = false, allMono = true;
    for (int g = v0 >> 6; g <= (v1 - 1) >> 6; ++g) {
        const size_t i = (size_t)k * (size_t)G + (size_t)g;
        const uint32_t w = (bw[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
        const uint32_t need = zl_pair_group_need(v0, v1, g);
        all = all && (w & need) == need;
        anyMono = anyMono || ((w >> 8) & need) != 0u;
        allMono = allMono && ((w >> 8) & need) == need;
    }
    return !all ? 0 : allMono ? 2 : anyMono ? 0 : 1;
}
template <bool ORD>
static __device__ __forceinline__ void zl_k2_pair_body(const ZlBatch &A)
{
    constexpr uint32_t MODE = 0;
    constexpr int U = ZL_K2_U, UP = ZL_K2_U_PAIR, UW = ZL_K2_U_PAIR_WRAP, CH = ZL_K2_CHUNK;
    static_assert(UP == U || 2 * UP == U, "the pair chunk walks a chunk class of U voices whole or in halves");
    static_assert(UW == U || 2 * UW == U, "and so does the chunk with loop restarts");
    __shared__ ZlBlockPlan  s_plan[CH];
    __shared__ ZlVoiceConst s_vc[CH];
    __shared__ int s_cls[CH];                         // per voice: 1 = plays this block, 2 = per-frame control
    __shared__ int s_chunk[CH / U];                   // class of each chunk of U voices
    __shared__ ZlUnit s_unit[CH];
    __shared__ int   s_pk[2][4];                      // fused level scan: the block's four 64-frame tiles (two per wave)
    __shared__ float s_sq[2][4];

    const int N = A.N, V = A.V;                                    // N == 256
    const int f0 = 2 * (int)threadIdx.x;
    // XCD-aware block order and phase order: as in zl_k2_body
    const unsigned by = blockIdx.y, bz = blockIdx.z;
    const int ky = (int)gridDim.y, xq = ky >> 3, xr = ky & 7, xx = (int)(by & 7u);
    const int ys = xx * xq + (xx < xr ? xx : xr) + (int)(by >> 3);
    // slots of the bus's order this workgroup holds: one, or -- a launch of ceil(K / 2) workgroups per bus (ZL_K2_PAIR_LAPS, zl_k2_launch; only
    // with the scalar records) -- slots 2 ys and 2 ys + 1, as many as exist.  The XCD mapping above is of workgroup numbers: an XCD still
    // gets a contiguous range of the order.
    const int laps = (ORD && (A.ongrid & ZL_ONGRID_SCALAR) && ky < A.K) ? 2 : 1;
    const int s0 = laps * ys, nb = !ORD || s0 + laps <= A.K ? laps : A.K - s0;
    const int bus = (int)bz;
    const int v0 = bus * A.VPB, vlim = (bus + 1) * A.VPB;
    const int v1 = (v0 + A.G < vlim) ? v0 + A.G : vlim;
    // the tail K1o leaves behind the table: from block run_end on, no voice of this bus has an inline run -- staging leaves the run lists alone
    const int32_t *dead_tail = ORD ? A.order + zl_order_tail_dead((int)gridDim.z, A.K, 0) : nullptr;
    const int run_end = ORD ? __builtin_amdgcn_readfirstlane(A.order[zl_order_tail_run_end((int)gridDim.z, A.K, (int)bz)]) : 0;

    // ---- the finished bus of block k.  Quirk Q2: frame f lands in out[f + 1], out[0] stays 0 and the sample of frame N - 1 is dropped
    auto finish = [&](int k, int f0, float accL0, float accR0, float accL1, float accR1) {
        const unsigned tx = (unsigned)f0 >> 1;                  // (the lane's number from the caller's own copy: see the block loop)
        const long long KN = (long long)A.Ktot * N;
        float *outL = A.bus + (long long)bus * (A.bus_stride ? A.bus_stride : 2 * KN) + (long long)(A.k0 + k) * N;
        float *outR = outL + (A.ch_stride ? A.ch_stride : KN);
        const bool written1 = f0 + 2 < N;
        outL[f0 + 1] = accL0; outR[f0 + 1] = accR0;
        if (written1) { outL[f0 + 2] = accL1; outR[f0 + 2] = accR1; }
        if (f0 == 0)  { outL[0] = 0.0f; outR[0] = 0.0f; }
        // ---- fused AudioLevels block scan (AudioLevels.cpp:361-383) in its defined order: tiles of 64 frames from out[1], a balanced
        //      pairwise tree inside a tile, tiles added in order.  This lane holds elements 2 j', 2 j' + 1 (j' = lane mod 32) of tile
        //      2 * wave + (lane >= 32): level 1 of the tree is the in-lane add, the rest zl_wave_levels4_pair.  The dropped frame scans as 0.
        if (A.levels) {
            const float bL = written1 ? accL1 : 0.0f, bR = written1 ? accR1 : 0.0f;
            const int pa = zl_sample_to_peak_int(accL0), pb = zl_sample_to_peak_int(bL), pc = zl_sample_to_peak_int(accR0), pd = zl_sample_to_peak_int(bR);
            int pkL[2], pkR[2]; float sqL[2], sqR[2];
            zl_wave_levels4_pair(pb > pa ? pb : pa, pd > pc ? pd : pc, accL0 * accL0 + bL * bL, accR0 * accR0 + bR * bR, pkL, pkR, sqL, sqR);
            const int w = (int)(tx >> 6) * 2;
            if ((tx & 63) == 0) {
                s_pk[0][w] = pkL[0]; s_pk[1][w] = pkR[0]; s_sq[0][w] = sqL[0]; s_sq[1][w] = sqR[0];
                s_pk[0][w + 1] = pkL[1]; s_pk[1][w + 1] = pkR[1]; s_sq[0][w + 1] = sqL[1]; s_sq[1][w + 1] = sqR[1];
            }
            __syncthreads();
            if (tx == 0) {
                ZlBlockLevels lv; lv.peak_l = 0; lv.peak_r = 0; lv.sumsq_l = 0.0f; lv.sumsq_r = 0.0f;
                for (int t = 0; t < 4; ++t) {
                    lv.peak_l = s_pk[0][t] > lv.peak_l ? s_pk[0][t] : lv.peak_l;
                    lv.peak_r = s_pk[1][t] > lv.peak_r ? s_pk[1][t] : lv.peak_r;
                    lv.sumsq_l += s_sq[0][t]; lv.sumsq_r += s_sq[1][t];
                }
                A.levels[(size_t)k * A.B + bus] = lv;
            }
        }
    };

    // ---- the two-slot walk (zl_k2_pair_fast2): both blocks pass the fast gate below -- behind run_end, neither the call's last block, every
    //      chunk of the bus fast -- with one layout.  Every other workgroup renders its blocks one after the other through the text below.
    if (ORD && nb == 2) {
        const int kA = __builtin_amdgcn_readfirstlane(A.order[(size_t)bz * A.K + s0]), kB = __builtin_amdgcn_readfirstlane(A.order[(size_t)bz * A.K + s0 + 1]);
        __builtin_assume(kA >= 0 && kA < 65536 && kB >= 0 && kB < 65536);
        if (zl_pair_laps_blocks(kA, kB, run_end, A.Ktot - 1 - A.k0)) {
            const int kindA = zl_k2_pair_fast_kind(zl_batch_pair_tab(A), A.K, V, kA, v0, v1);
            const int kindB = kindA != 0 ? zl_k2_pair_fast_kind(zl_batch_pair_tab(A), A.K, V, kB, v0, v1) : 0;
            if (zl_pair_laps_kind(kindA, kindB) != 0) {
                const uint64_t *addrA = zl_batch_pair_tab(A) + (size_t)kA * (size_t)V + (size_t)v0;
                const uint64_t *addrB = zl_batch_pair_tab(A) + (size_t)kB * (size_t)V + (size_t)v0;
                const uint64_t *pan = zl_batch_pair_tab(A) + zl_pair_tab_pan(A.K, V) + (size_t)v0;
                float accA[4] = {0.0f, 0.0f, 0.0f, 0.0f}, accB[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (kindA == 2) zl_k2_pair_fast2<true>(addrA, addrB, pan, (v1 - v0) >> 2, f0, accA, accB);
                else            zl_k2_pair_fast2<false>(addrA, addrB, pan, (v1 - v0) >> 2, f0, accA, accB);
                finish(kA, f0, accA[0], accA[1], accA[2], accA[3]);
                __syncthreads();                                  // (s_pk, s_sq are reused)
                finish(kB, f0, accB[0], accB[1], accB[2], accB[3]);
                return;
            }
        }
    }

#pragma nounroll
    for (int ib = 0; ib < nb; ++ib) {
    // (the lane's number as the loop body's own value: what is derived from it is formed per block, not held across the loop -- 103 registers
    // instead of 108.  tests/test_kernel_resources_pair.py allows 104 and fails if a compiler brings the count back up: look here first)
    unsigned tx = threadIdx.x;
    asm volatile("" : "+v"(tx));
    const int f0i = 2 * (int)tx;
    if (ib != 0) __syncthreads();                                  // (the second block restages: the first one's report path and level scan are done with LDS)
    const int k = ORD ? A.order[(size_t)bz * A.K + s0 + ib] : ys;
    __builtin_assume(k >= 0 && k < 65536);                         // (a launch slot's block: what the compiler knows of ys it may know of the table's entry)
    const bool wantPeak = __builtin_amdgcn_readfirstlane((int)(A.k0 + k == A.Ktot - 1)) != 0;
    const bool norun = ORD && __builtin_amdgcn_readfirstlane((int)(k >= run_end)) != 0;

    float accL0 = 0.0f, accR0 = 0.0f, accL1 = 0.0f, accR1 = 0.0f;
    // the fast workgroup (zl_k2_pair_fast): the window has the scalar records, every record of the block is an explicit one (norun), it is not
    // the call's last block (the report path reads s_plan) and every chunk of the bus is fast in this block.  Every other workgroup stages.
    int fastKind = 0;
    if (ORD && (A.ongrid & ZL_ONGRID_SCALAR) && norun && !wantPeak)
        fastKind = zl_k2_pair_fast_kind(zl_batch_pair_tab(A), A.K, V, __builtin_amdgcn_readfirstlane(k), v0, v1);
    if (fastKind != 0) {
        const uint64_t *addr = zl_batch_pair_tab(A) + (size_t)__builtin_amdgcn_readfirstlane(k) * (size_t)V + (size_t)v0;
        const uint64_t *pan = zl_batch_pair_tab(A) + zl_pair_tab_pan(A.K, V) + (size_t)v0;
        if (fastKind == 2) zl_k2_pair_fast<true>(addr, pan, (v1 - v0) >> 3, f0i, accL0, accR0, accL1, accR1);
        else               zl_k2_pair_fast<false>(addr, pan, (v1 - v0) >> 3, f0i, accL0, accR0, accL1, accR1);
    } else
    for (int vb = v0; vb < v1; vb += CH) {
        const int nv = (v1 - vb < CH) ? v1 - vb : CH;
        if (vb != v0) __syncthreads();                            // (nothing to wait for before the first pass)
        for (int i = tx; i < CH; i += blockDim.x) {
            ZlVoiceConst vc;
            ZlBlockPlan pl;
            if (norun) zl_k2_stage_load<false>(A, k, vb, i, nv, vc, pl, dead_tail);
            else       zl_k2_stage_load<true>(A, k, vb, i, nv, vc, pl, nullptr);
            const int cls = zl_k2_stage_class<MODE>(A, vc, pl);
            s_unit[i] = zl_k2_stage_unit<MODE>(A, vc, pl, cls);
            s_vc[i] = vc;
            s_plan[i] = pl;
            s_cls[i] = cls;
            zl_k2_stage_chunks<U>(cls, i, s_chunk);
        }
        __syncthreads();
        for (int c0 = 0; c0 < nv; c0 += U) {
            const int cc = __builtin_amdgcn_readfirstlane(s_chunk[c0 / U]);
            if (cc == 0) {                                        // nobody in this chunk plays (SamplerSynth.cpp:137)
            } else if ((cc & 132) == 132) {
                // every voice of the chunk on-grid and of one source layout
#pragma unroll
                for (int h = 0; h < U; h += UP) {
                    if (wantPeak) {
                        if (cc & 16) zl_k2_chunk_ongrid_pair<true, UP, true>(A, s_vc, s_unit, c0 + h, vb, f0i, accL0, accR0, accL1, accR1);
                        else         zl_k2_chunk_ongrid_pair<false, UP, true>(A, s_vc, s_unit, c0 + h, vb, f0i, accL0, accR0, accL1, accR1);
                    }
                    else if (cc & 16) zl_k2_chunk_ongrid_pair<true, UP, false>(A, s_vc, s_unit, c0 + h, vb, f0i, accL0, accR0, accL1, accR1);
                    else              zl_k2_chunk_ongrid_pair<false, UP, false>(A, s_vc, s_unit, c0 + h, vb, f0i, accL0, accR0, accL1, accR1);
                }
            } else if ((cc & 256) && !wantPeak) {
                // every voice on-grid, one or more of them with a loop restart inside the block (not in the call's last block)
#pragma unroll
                for (int h = 0; h < U; h += UW) {
                    if (cc & 16) zl_k2_chunk_ongrid_pair_wrap<true, UW>(A, s_plan, s_vc, s_unit, c0 + h, f0i, accL0, accR0, accL1, accR1);
                    else         zl_k2_chunk_ongrid_pair_wrap<false, UW>(A, s_plan, s_vc, s_unit, c0 + h, f0i, accL0, accR0, accL1, accR1);
                }
            } else {
                // the other classes: zl_k2_body's dispatch, one frame of the lane after the other
#pragma nounroll
                for (int h = 0; h < 2; ++h) {
                    const int fc = f0i + h;
                    const double fd = (double)fc;
                    float accL = h ? accL1 : accL0, accR = h ? accR1 : accR0;
                    if ((cc & 124) == 100)      zl_k2_chunk_simple<MODE, false, true, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 92) == 68)   zl_k2_chunk_simple<MODE, false, false, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 28) == 4)    zl_k2_chunk_simple<MODE, false, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 20) == 4)    zl_k2_chunk_simple<MODE, true, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 124) == 116) zl_k2_chunk_simple_mono<MODE, false, true, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 92) == 84)   zl_k2_chunk_simple_mono<MODE, false, false, true, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 28) == 20)   zl_k2_chunk_simple_mono<MODE, false, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else if ((cc & 20) == 20)   zl_k2_chunk_simple_mono<MODE, true, false, false, U>(A, s_plan, s_vc, s_unit, c0, vb, fc, fd, wantPeak, accL, accR);
                    else {
                        constexpr int H = U / 2;                  // (general chunks as two half-chunks, as in zl_k2_body)
                        const size_t pbase = (size_t)k * V + vb;
                        for (int q = 0; q < U; q += H) {
                            if (cc & 2) zl_k2_chunk<MODE, true, H>(A, s_plan, s_vc, s_cls, c0 + q, pbase, vb, fc, wantPeak, accL, accR);
                            else        zl_k2_chunk<MODE, false, H>(A, s_plan, s_vc, s_cls, c0 + q, pbase, vb, fc, wantPeak, accL, accR);
                        }
                    }
                    if (h) { accL1 = accL; accR1 = accR; } else { accL0 = accL; accR0 = accR; }
                }
            }
        }
    }

    finish(k, f0i, accL0, accR0, accL1, accR1);

    // ---- the call's reports, by the workgroups that hold the call's last block (as in zl_k2_body)
    if (A.fused_reports && A.k0 + k == A.Ktot - 1) {
        __syncthreads();
        for (int v = v0 + (int)tx; v < v1; v += (int)blockDim.x) {
            const uint4 *src = reinterpret_cast<const uint4 *>(&A.reports[v]);
            uint4 a = src[0];
            const uint4 b = src[1];
            a.z = __hip_atomic_load(&A.reports[v].peak_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float gn = __uint_as_float(a.z) * 0.5f;
            A.rep_gain[v] = gn;
            if (A.rep_host) { uint4 *dst = reinterpret_cast<uint4 *>(&A.rep_host[v]); dst[0] = a; dst[1] = b; A.rep_host_gain[v] = gn; }
        }
        if (bus == 0 && tx == 0 && A.rep_host_stats) {
            const unsigned long long sb = A.stats->source_bytes, sl = A.stats->slow_blocks, af = A.stats->active_frames;
            A.rep_host_stats->source_bytes = sb; A.rep_host_stats->slow_blocks = sl; A.rep_host_stats->active_frames = af;
            A.stats->source_bytes = 0; A.stats->slow_blocks = 0; A.stats->active_frames = 0;   // cleared for the call that reuses this slot
        }
    }
    }
}

__global__ void __launch_bounds__(128, ZL_K2_PAIR_WAVES) zl_k2_pair_render(const ZlBatch A) { zl_k2_pair_body<false>(A); }
__global__ void __launch_bounds__(128, ZL_K2_PAIR_WAVES) zl_k2_pair_phase_render(const ZlBatch A) { zl_k2_pair_body<true>(A); }

// ------------------------------------------------------------------------------------------------
// Resident real-time kernel: one workgroup PER BUS that stays on the GPU and renders a JACK cycle whenever the host
// posts one in the mailbox -- no kernel launch, no completion event, no command-processor packet per block.  A workgroup owns
// its bus: it applies the voice operations of the bus's voices (K0), plans them (K1 + K1c, one block), renders the bus (the K2
// body: the workgroup's lanes = the block's frames), and writes mix + reports straight into host memory.  Nothing is handed
// from one workgroup to another except the command: workgroup 0 watches the mailbox (host memory) and republishes each block in
// HBM with agent-scope atomics; the last workgroup to finish (an arrival counter) tells the host.  Only workgroup 0 decides to
// leave -- on a stop request or after idle_ticks (100 MHz) without a block -- and publishes that too, so every block is either
// rendered by all workgroups or by none, and every wave reaches the exit.
//
// WIDE (buses of 32 voices and more): one workgroup PER VOICE instead -- a single block has no other parallelism than its voices.
// Every workgroup renders its voice into the bus's partial rows (K2 body with one voice per mix group); the workgroup that is the
// last of its bus to arrive (a counter per bus, no waiting) sums the rows in voice order, 0 + v0 + v1 + ... -- the reference's
// order, bit for bit (K3 body) -- writes the bus into host memory and scans its levels.  The voice-operation ranges of the block
// are copied from host memory into HBM once, by workgroup 0 before it publishes the block (a thousand workgroups reading the
// same host memory would queue on PCIe).  Hand-offs between workgroups on different XCDs use agent-scope release / acquire fences.
static __device__ __forceinline__ void zl_k3_body(const ZlBatch &A, const float *bus_in, int k, int bus);
// (two waves per SIMD = two resident workgroups per CU: the budget the capacity rule of zl_engine.cpp rt_eligible counts on -- 256
// registers per lane, accumulation registers included)
template <uint32_t MODE, bool WIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) zl_k_rt_loop(const ZlBatch A0, ZlRtShared *sh, ZlRtDev *dev, unsigned long long first_seq, unsigned long long idle_ticks,
                                                    float *gain_out, ZlReport *host_reports, float *host_gain, ZlOpRange *dev_ranges, int vw)
{
    __shared__ unsigned long long s_cmd[ZL_RT_CMD_WORDS + 1];     // [0] = the block's sequence number (0 with s_go = 0: leave)
    __shared__ int s_go, s_last;
    __shared__ ZlClock s_clk0;
    __shared__ ZlPassParams s_pass;                               // JackPassthrough parameters of this workgroup's bus, as of version s_pass_seq
    __shared__ uint32_t s_pass_seq;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_pass_seq = 0u;
    const int z = blockIdx.x, W = gridDim.x;                       // one workgroup per bus (WIDE: per vw voices of one bus; vw divides VPB)
    const int vbeg = WIDE ? z * vw : z * A0.VPB, vend = WIDE ? vbeg + vw : vbeg + A0.VPB;
    unsigned long long last = first_seq;
    if (z == 0 && tid == 0) __hip_atomic_store(&sh->state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (;;) {
        if (tid == 0) {
            int go = 0;
            if (z == 0) {
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                for (;;) {
                    const unsigned long long q = __hip_atomic_load(&sh->cmd_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if (q != last) {
                        // (the host wrote the words, then cmd_seq with a release store.)  Narrow buses: the NUMBER goes out to the other
                        // workgroups at once; each of them reads the words itself.  Wide buses: published below, with the words and the ranges
                        if (!WIDE) __hip_atomic_store(&dev->pub_seq, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s_cmd[0] = q; go = 1;
                        break;
                    }
                    if (__hip_atomic_load(&sh->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) || __hip_atomic_load(&sh->yield, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                        || __builtin_amdgcn_s_memrealtime() - t0 > idle_ticks) {
                        __hip_atomic_store(&dev->pub_seq, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // everybody leaves
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
            } else {
                for (;;) {
                    const unsigned long long q = __hip_atomic_load(&dev->pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (q == ~0ull) break;
                    if (q != last) { s_cmd[0] = q; go = 1; break; }
                    if (WIDE) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(1);   // (a thousand pollers: longer naps)
                }
            }
            s_go = go;
        }
        __syncthreads();
        if (!s_go) break;
        // ---- the cycle's command words, ONE WORD PER LANE (one trip, all words in flight together; a single lane's system-scope loads
        //      would go out one after the other: 34 trips over PCIe): out of the mailbox in host memory (system scope, past the caches)
        //      -- every workgroup of a narrow engine, workgroup 0 of a wide one, which also leaves them in HBM for the others
        if (tid < ZL_RT_CMD_WORDS) {
            unsigned long long wv;
            if (!WIDE || z == 0) wv = __hip_atomic_load(&sh->cmd[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else                 wv = __hip_atomic_load(&dev->cmd[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (WIDE && z == 0) __hip_atomic_store(&dev->cmd[tid], wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_cmd[1 + tid] = wv;
        }
        __syncthreads();
        last = s_cmd[0];
        if (A0.rt_stamps && z == 0 && tid == 0) sh->stamps[0] = __builtin_amdgcn_s_memrealtime();
        ZlBatch A = A0;
        A.N = (int)(uint32_t)s_cmd[1]; A.n_op_ranges = (int)(uint32_t)(s_cmd[1] >> 32);
        A.ops = reinterpret_cast<const ZlVoiceOp *>((uintptr_t)s_cmd[2]); A.op_ranges = reinterpret_cast<const ZlOpRange *>((uintptr_t)s_cmd[3]);
        A.ctl_base = s_cmd[4];
        A.clock0.current_usecs = s_cmd[5]; A.clock0.next_usecs = s_cmd[6]; A.clock0.playhead = s_cmd[7]; A.clock0.playhead_usecs = s_cmd[8];
        A.clock0.subbeat_usecs = s_cmd[9]; A.clock0.usecs_per_frame = s_cmd[10];
        A.n_clip_edits = (int)(uint32_t)s_cmd[11]; A.clip_edits = reinterpret_cast<const ZlClipEdit *>((uintptr_t)s_cmd[12]);
        A.inline_clock = 1; A.fuse_assemble = 1;
        // ---- JackPassthrough fan-out of this cycle (JackPassthrough.cpp:45-115): asked for per cycle; the parameters of the workgroup's
        //      bus are kept in LDS across cycles and read again from the host's table (mapped memory: a trip over PCIe, issued here and
        //      needed at the store, after planning) only when the host moved the table's version -- a knob turned while playing
        // where the cycle's rows go: the engine's staging rows, or straight into the caller's page-locked buffers
        A.bus = reinterpret_cast<float *>((uintptr_t)s_cmd[13]); A.fan = reinterpret_cast<float *>((uintptr_t)s_cmd[14]);
        A.bus_stride = (long long)s_cmd[15]; A.ch_stride = (long long)s_cmd[16];
        const uint32_t fan_seq = (uint32_t)(s_cmd[11] >> 32);
        if (fan_seq == 0u) A.fan = nullptr;
        else if (tid < 64) {
            // (wave 0 only: its lanes read the version before lane 0 writes it -- program order inside one wave; one word per lane, one trip)
            const bool refresh = fan_seq != s_pass_seq;
            const int pb = (WIDE ? vbeg / A0.VPB : z);
            const uint32_t *src = reinterpret_cast<const uint32_t *>(A0.pass + pb);
            uint32_t *dst = reinterpret_cast<uint32_t *>(&s_pass);
            if (refresh && tid < (int)(sizeof(ZlPassParams) / 4)) dst[tid] = __hip_atomic_load(src + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (refresh && tid == 0) s_pass_seq = fan_seq;
        }
        A.pass_inline = 1;
        A.tile_accum = 1;                                          // this workgroup walks every frame tile of its block (below)
        if (WIDE && z == 0) {
            // workgroup 0: the block's operation ranges host memory -> HBM (behind a system-scope acquire: the host reuses its buffers
            // every block and plain loads may hit stale cached lines), then the block is published for the other workgroups
            if (A.n_op_ranges > 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                for (int i = tid; i < A.n_op_ranges; i += (int)blockDim.x) dev_ranges[i] = A.op_ranges[i];
            }
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&dev->pub_seq, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // ---- K0: the operations of this workgroup's voices (the ranges are sorted by voice).  Narrow buses read ranges and
        //      operations in host memory in place (system-scope acquire, as above); wide buses read the ranges from workgroup 0's
        //      copy in HBM (agent-scope acquire: it may sit in another XCD's L2) and only their own operations from host memory
        if (A.n_op_ranges > 0 || A.n_clip_edits > 0) {
            if (WIDE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        }
        // ---- the cycle's clip-parameter edits: EVERY workgroup writes all of them into the HBM clip table (the same bytes; a few per
        //      cycle at most).  A workgroup then plans from what it wrote itself -- its own XCD's L2 -- so no hand-off between
        //      workgroups is needed, and the table is complete in HBM when the kernel leaves.
        for (int i = tid >> 6; i < A.n_clip_edits; i += (int)(blockDim.x >> 6)) zl_apply_clip_edit(A, A.clip_edits + i, lane);
        // (the knob edits that came with the command: 8 words each, from LDS)
        if (tid < ZL_RT_INLINE_EDITS * (ZL_CLIP_HEAD_BYTES / 4)) {
            const int ei = tid / (ZL_CLIP_HEAD_BYTES / 4), wi = tid % (ZL_CLIP_HEAD_BYTES / 4);
            const unsigned long long *ew = &s_cmd[1 + ZL_RT_CMD_FIXED + ei * ZL_RT_EDIT_WORDS];
            const int clip = (int)(uint32_t)ew[0];
            if (clip >= 0) reinterpret_cast<uint32_t *>(const_cast<ZlClip *>(A.clips) + clip)[wi] = reinterpret_cast<const uint32_t *>(ew + 1)[wi];
        }
        const ZlOpRange *ranges = WIDE ? dev_ranges : A.op_ranges;
        for (int i = tid; i < A.n_op_ranges; i += (int)blockDim.x) {
            const ZlOpRange rg = ranges[i];
            if (rg.voice < vbeg || rg.voice >= vend) continue;
            ZlVoiceState st = A.voices[rg.voice];
            for (int j = 0; j < rg.count; ++j) zl_apply_op(st, A.ops[rg.first + j]);
            A.voices[rg.voice] = st;
        }
        if (tid == 0) s_clk0 = A.clock0;
        __threadfence_block();
        __syncthreads();
        if (A0.rt_stamps && z == 0 && tid == 0) sh->stamps[1] = __builtin_amdgcn_s_memrealtime();
        // ---- K1: one lane per voice of the workgroup, the single block of this cycle
        for (int v = vbeg + tid; v < vend; v += (int)blockDim.x) {
            ZlPlanner pl;
            // (inlined here: as calls, the planner object and the cycle's ZlBatch live in scratch memory, 1 KB per lane)
            [[clang::always_inline]] pl.begin(A, v, 0);
            while (pl.t < A.N) { [[clang::always_inline]] pl.iterate(A, 1, &s_clk0, 0, 0); }
            [[clang::always_inline]] pl.end(A);
        }
        __threadfence_block();
        __syncthreads();
        if (A0.rt_stamps && z == 0 && tid == 0) sh->stamps[2] = __builtin_amdgcn_s_memrealtime();
        // ---- K1c: plan records of the block, multi-segment blocks expanded by whole waves
        for (int v0 = vbeg; v0 < vend; v0 += (int)blockDim.x) {
            const int v = v0 + tid;
            const bool mine = v < vend;
            ZlAssembler as;
            [[clang::always_inline]] as.begin(A, mine ? v : vbeg, 0, mine ? 1 : 0);
            zl_k1c_block(A, as, v, lane, 0);
        }
        __threadfence_block();
        __syncthreads();
        if (A0.rt_stamps && z == 0 && tid == 0) sh->stamps[3] = __builtin_amdgcn_s_memrealtime();
        // ---- K2: this bus (WIDE: each of this workgroup's voices into its own partial row: A.groups = voices per bus, one voice per group).
        //      A block longer than the workgroup (JACK periods of 512, 1024 ... frames) is walked tile by tile.
        if (A.fan) A.pass0 = s_pass;                               // (written before the barriers above)
        const unsigned tiles = ((unsigned)A.N + blockDim.x - 1u) / blockDim.x;
        for (unsigned bx = 0; bx < tiles; ++bx) {
            if (WIDE) { for (int v = vbeg; v < vend; ++v) zl_k2_body<MODE, 1, false, false>(A, bx, 0u, (unsigned)v, tiles, 1u); }
            else zl_k2_body<MODE, 1, false, false>(A, bx, 0u, (unsigned)z, tiles, 1u);
            __threadfence_block();
            __syncthreads();
        }
        if (WIDE) {
            // ---- the bus: the last of its workgroups to get here sums the partial rows in voice order, writes the mix, scans the levels
            const int bus = vbeg / A.VPB;
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");     // this voice's partial rows, for a workgroup that may run on another XCD
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned int old = __hip_atomic_fetch_add(&dev->bus_arrive[bus], (unsigned int)vw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int lastOne = old + (unsigned int)vw == (unsigned int)A.VPB;
                if (lastOne) __hip_atomic_store(&dev->bus_arrive[bus], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_last = lastOne;
            }
            __syncthreads();
            if (s_last) {                                              // (uniform over the workgroup)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                zl_k3_body(A, nullptr, 0, bus);
            }
            __threadfence_block();
            __syncthreads();
        }
        if (A0.rt_stamps && z == 0 && tid == 0) sh->stamps[4] = __builtin_amdgcn_s_memrealtime();
        // ---- reports (gain = peakGain * 0.5f, SamplerSynthVoice.cpp:266) straight into host memory
        for (int v = vbeg + tid; v < vend; v += (int)blockDim.x) {
            const ZlReport r = A.reports[v];
            const float g = __uint_as_float(r.peak_bits) * 0.5f;
            gain_out[v] = g; host_reports[v] = r; host_gain[v] = g;
        }
        __syncthreads();                                           // every wave's stores are issued and waited for (workgroup release)
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");          // system scope: this bus's mix and reports (host memory), its levels (HBM)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (A0.rt_stamps && z == 0) sh->stamps[5] = __builtin_amdgcn_s_memrealtime();
            if (!WIDE) {
                // one workgroup per bus: each tells the host itself (the host waits for all of them) -- no counter round trip, no last-arrival store
                __hip_atomic_store(&sh->wg_done[z], (uint32_t)last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                const unsigned int old = __hip_atomic_fetch_add(&dev->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == (unsigned int)W - 1u) {                 // the last workgroup: the block is complete
                    __hip_atomic_store(&dev->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(&sh->done_seq, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
    if (z == 0 && tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&sh->state, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The AudioLevels scan of one (block, bus) row pair by ONE wave: integer peaks (AudioLevels.cpp:361-383) and the sums of
// squares of the RMS extension in their defined order (oracle/zl_oracle.c zlo_block_sumsq): tiles of 64 frames from frame
// `off` (1 with quirk Q2: frame 0 of a bus is the constant 0 and lane f of K2 holds out[f + 1]; 0 with FIX_DELAY), the
// wave's DPP tree inside a tile, tiles added in order -- the same bits as K2's fused scan.  Any N: a short last tile is padded with zeros.
static __device__ __forceinline__ ZlBlockLevels zl_scan_rows(const float *inL, const float *inR, int N, int off, int lane)
{
    int pkL = 0, pkR = 0; float sqL = 0.0f, sqR = 0.0f;
    if (off) {                                                     // the frames in front of the first tile (uniform loads)
        const float l0 = inL[0], r0 = inR[0];
        pkL = zl_sample_to_peak_int(l0); pkR = zl_sample_to_peak_int(r0);
        sqL = l0 * l0; sqR = r0 * r0;
    }
    for (int t0 = off; t0 < N; t0 += 64) {
        const int i = t0 + lane;
        const float l = i < N ? inL[i] : 0.0f, r = i < N ? inR[i] : 0.0f;
        const int a = zl_sample_to_peak_int(l), c = zl_sample_to_peak_int(r);
        pkL = a > pkL ? a : pkL; pkR = c > pkR ? c : pkR;
        sqL += zl_wave_sum(l * l); sqR += zl_wave_sum(r * r);      // wave-uniform running sums, tile order
    }
    ZlBlockLevels out;
    out.peak_l = zl_wave_max_nonneg(pkL); out.peak_r = zl_wave_max_nonneg(pkR); out.sumsq_l = sqL; out.sumsq_r = sqR;
    return out;
}

// ------------------------------------------------------------------------------------------------
// K3: one workgroup per (block, bus).  Sums the mix-group partials in group order (when there are
// any), writes the bus, and scans it for the AudioLevels integer peak and the RMS extension.
static __device__ __forceinline__ void zl_k3_body(const ZlBatch &A, const float *bus_in, int k, int bus)
{
    const int N = A.N;
    const size_t KN = (size_t)A.Ktot * N;
    float *outL = A.bus ? A.bus + (long long)bus * (A.bus_stride ? A.bus_stride : 2 * (long long)KN) + (long long)(A.k0 + k) * N : nullptr;
    float *outR = outL ? outL + (A.ch_stride ? A.ch_stride : (long long)KN) : nullptr;
    const float *inL = bus_in ? bus_in + ((size_t)bus * 2) * KN + (size_t)(A.k0 + k) * N : outL;
    const float *inR = bus_in ? inL + KN : outR;

    for (int f = threadIdx.x; f < N && A.groups > 1 && !bus_in; f += blockDim.x) {
        float l, r;
        {
            l = 0.0f; r = 0.0f;
            const float *p = A.partials + (((size_t)k * A.B + bus) * A.groups) * 2 * (size_t)N;
            // the adds are sequential (group order = the summation order), the loads are not: eight groups' partials are
            // requested at once (voices_per_task = 1 makes every voice a group and this loop 128 long)
            int g = 0;
            for (; g + 8 <= A.groups; g += 8) {
                float pl[8], pr[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { pl[u] = p[(size_t)u * 2 * N + f]; pr[u] = p[(size_t)u * 2 * N + N + f]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { l += pl[u]; r += pr[u]; }
                p += 16 * (size_t)N;
            }
            for (; g < A.groups; ++g) { l += p[f]; r += p[N + f]; p += 2 * (size_t)N; }
            outL[f] = l; outR[f] = r;
            if (A.fan) {                                           // fused JackPassthrough fan-out, as in K2
                const ZlPassParams pp = A.pass_inline ? A.pass0 : A.pass[bus];
                float *o = A.fan + ((size_t)bus * 6) * KN + (size_t)(A.k0 + k) * N;
                float lm, rm; zl_pass_pan(pp, lm, rm);
                const float amounts[3] = { pp.dry, pp.fx1, pp.fx2 };
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ol, orr;
                    zl_pass_pair(pp, amounts[c], lm, rm, l, r, ol, orr);
                    o[(size_t)(2 * c) * KN + f] = ol; o[(size_t)(2 * c + 1) * KN + f] = orr;
                }
            }
        }
    }
    // the rows of this (block, bus) are complete: wave 0 scans them in the defined order (zl_scan_rows) -- the workgroup
    // reads back its own stores (workgroup-scope fence + barrier; when nothing was summed the rows are the input's)
    if (A.groups > 1 && !bus_in) { __threadfence_block(); __syncthreads(); }
    if (threadIdx.x < 64) {
        const ZlBlockLevels lv = zl_scan_rows(inL, inR, N, (A.mode & ZL_MODE_FIX_DELAY) ? 0 : 1, (int)threadIdx.x);
        if (threadIdx.x == 0) A.levels[(size_t)k * A.B + bus] = lv;
    }
}
__global__ void __launch_bounds__(256) zl_k3_finalize(const ZlBatch A, const float *bus_in)
{
    zl_k3_body(A, bus_in, (int)blockIdx.x, (int)blockIdx.y);
}

// K3 without partials to sum (the scan of an existing bus: N > 256, or a bus reduced over several GPUs): one WAVE per
// (block, bus), reductions on the VALU -- no LDS, no barrier.
__global__ void __launch_bounds__(256) zl_k3_scan(const ZlBatch A, const float *bus)
{
    const int N = A.N;
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // (block, bus) pairs, bus fastest
    if (pair >= (long long)A.K * A.B) return;                                     // whole waves leave
    const int k = (int)(pair / A.B), b = (int)(pair - (long long)k * A.B);
    const int lane = threadIdx.x & 63;
    const long long KN = (long long)A.Ktot * N;
    const bool own = bus == A.bus;                                 // the call's own bus may have the caller's strides
    const float *inL = bus + (long long)b * (own && A.bus_stride ? A.bus_stride : 2 * KN) + (long long)(A.k0 + k) * N;
    const ZlBlockLevels out = zl_scan_rows(inL, inL + (own && A.ch_stride ? A.ch_stride : KN), N, (A.mode & ZL_MODE_FIX_DELAY) ? 0 : 1, lane);
    if (lane == 0) A.levels[(size_t)k * A.B + b] = out;
}

// ------------------------------------------------------------------------------------------------
// Multi-GPU exchange step: when a bus spans GPUs every rank receives, for its share of the bus, one piece
// per rank (all-to-all over the xGMI mesh).  This kernel sums the pieces IN RANK ORDER -- ((0 + p0) + p1) + ... per sample,
// the order of K3's mix-group sum and of the oracle's grouped mix, so the result is the same bits for any number of ranks --
// writes the reduced piece, and scans it for AudioLevels in the same pass: integer peak and sum of squares (defined order,
// zl_scan_rows) per unit.  A piece is a run of whole units; unit = the N frames of one (bus, channel, block).  One wave per
// unit; the loads of up to 8 pieces are in flight before the ordered adds.
__global__ void __launch_bounds__(256) zl_k_reduce_scan(const float *pieces, int npieces, long long stride, long long units, int N, int off,
                                                        float *out, ZlUnitLevels *lv)
{
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= units) return;                                        // whole waves leave
    const int lane = threadIdx.x & 63;
    const float *p0 = pieces + u * N;
    float *o = out + u * N;
    auto sum_at = [&](int idx) {
        float v = 0.0f;
        const float *p = p0 + idx;
        int r = 0;
        for (; r + 8 <= npieces; r += 8) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = p[(long long)(r + j) * stride];
#pragma unroll
            for (int j = 0; j < 8; ++j) v += x[j];
        }
        for (; r < npieces; ++r) v += p[(long long)r * stride];
        return v;
    };
    int pk = 0; float sq = 0.0f;
    if (off) {                                                     // the frame in front of the first tile (every lane: one address)
        const float v = sum_at(0);
        if (lane == 0) o[0] = v;
        pk = zl_sample_to_peak_int(v); sq = v * v;
    }
    for (int t0 = off; t0 < N; t0 += 64) {
        const int idx = t0 + lane;
        float v = 0.0f;
        if (idx < N) { v = sum_at(idx); o[idx] = v; }
        const int a = zl_sample_to_peak_int(v);
        pk = a > pk ? a : pk;
        sq += zl_wave_sum(v * v);                                  // wave-uniform running sum, tile order
    }
    pk = zl_wave_max_nonneg(pk);
    if (lane == 0) { ZlUnitLevels r; r.peak = pk; r.sumsq = sq; lv[u] = r; }
}

// Spanning-bus sum of an engine group (zlhip_group_*, span partition): every member rendered all buses with its slice of each bus's
// voices into a partial bus [B][2][K*N] on its own device.  One wave per (block, bus) pair, pair = k * B + b (the ZlBlockLevels order),
// both channels, so the wave writes its ZlBlockLevels whole.  Per sample it sums the NM members' partials IN RANK ORDER from 0,
// ((0 + p0) + p1) + ... -- K3's mix-group order and zl_k_reduce_scan's -- with all 2 * NM loads in flight before the ordered adds, stores
// the sum into the root's bus and scans it exactly as zl_scan_rows does (front frame with `off`, 64-frame tiles, zl_wave_sum per tile).
// Member r launches it on its own device for its share [p0, p1) of the pairs; the other members' partials are read over xGMI (peer
// access).  A pair is read and written by one wave only, so the root's own partial may be the output (summed in place).
template <int NM>
__global__ void __launch_bounds__(256) zl_k_group_reduce_scan(const ZlGroupReduceArgs a)
{
    const long long pair = a.p0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= a.p1) return;                                      // whole waves leave
    const int lane = threadIdx.x & 63;
    const int N = a.N;
    const int k = (int)(pair / a.B), b = (int)(pair - (long long)k * a.B);
    const long long KN = (long long)a.K * N;
    const long long rowL = (long long)b * 2 * KN + (long long)k * N, rowR = rowL + KN;
    auto sum2 = [&](int f, float &l, float &r) {
        float xl[NM], xr[NM];
#pragma unroll
        for (int j = 0; j < NM; ++j) { xl[j] = a.part[j][rowL + f]; xr[j] = a.part[j][rowR + f]; }
        l = 0.0f; r = 0.0f;
#pragma unroll
        for (int j = 0; j < NM; ++j) { l += xl[j]; r += xr[j]; }
    };
    int pkL = 0, pkR = 0; float sqL = 0.0f, sqR = 0.0f;
    if (a.off) {                                                   // the frame in front of the first tile (every lane: one address)
        float l, r;
        sum2(0, l, r);
        if (lane == 0) { a.out[rowL] = l; a.out[rowR] = r; }
        pkL = zl_sample_to_peak_int(l); pkR = zl_sample_to_peak_int(r);
        sqL = l * l; sqR = r * r;
    }
    for (int t0 = a.off; t0 < N; t0 += 64) {
        const int f = t0 + lane;
        float l = 0.0f, r = 0.0f;
        if (f < N) { sum2(f, l, r); a.out[rowL + f] = l; a.out[rowR + f] = r; }
        const int pa = zl_sample_to_peak_int(l), pc = zl_sample_to_peak_int(r);
        pkL = pa > pkL ? pa : pkL; pkR = pc > pkR ? pc : pkR;
        sqL += zl_wave_sum(l * l); sqR += zl_wave_sum(r * r);      // wave-uniform running sums, tile order
    }
    ZlBlockLevels o;
    o.peak_l = zl_wave_max_nonneg(pkL); o.peak_r = zl_wave_max_nonneg(pkR); o.sumsq_l = sqL; o.sumsq_r = sqR;
    if (lane == 0) a.levels[pair] = o;
}

// unit levels of a whole bus ([bus][channel][block], as the exchange gathers them) -> the engine's per-block levels
__global__ void zl_k_levels_import(const ZlUnitLevels *units, ZlBlockLevels *levels, int B, int K)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;           // (block, bus), bus fastest
    if (i >= B * K) return;
    const int k = i / B, b = i - k * B;
    const ZlUnitLevels l = units[((size_t)b * 2) * K + k], r = units[((size_t)b * 2 + 1) * K + k];
    ZlBlockLevels o; o.peak_l = l.peak; o.peak_r = r.peak; o.sumsq_l = l.sumsq; o.sumsq_r = r.sumsq;
    levels[i] = o;
}

// AudioLevels::timerCallback state update for every bus (AudioLevels.cpp:359-360, 367-383 via the
// block scan of K3, 385, 395-396).  dBFS conversion (log10f) stays on the host, as in the reference.
__global__ void zl_k_levels_tick(ZlLevelsState *state, const ZlBlockLevels *levels, int B, int N, int with_hold_bus)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ZlLevelsState s = state[b];
    s.peak_a = s.peak_a - 10000 > 0 ? s.peak_a - 10000 : 0;
    s.peak_b = s.peak_b - 10000 > 0 ? s.peak_b - 10000 : 0;
    if (levels) {
        const ZlBlockLevels lv = levels[b];
        s.peak_a = lv.peak_l > s.peak_a ? lv.peak_l : s.peak_a;
        s.peak_b = lv.peak_r > s.peak_b ? lv.peak_r : s.peak_b;
        s.sumsq_a = lv.sumsq_l; s.sumsq_b = lv.sumsq_r; s.frames = N;
    }
    if (b == with_hold_bus) {
        const float intToFloatMultiplier = 0.00000152587f;         // AudioLevels.cpp:349 (Q12)
        const float peakA = s.peak_a * intToFloatMultiplier, peakB = s.peak_b * intToFloatMultiplier;
        s.hold_a = (peakA >= s.hold_a) ? peakA : s.hold_a * 0.9f;
        s.hold_b = (peakB >= s.hold_b) ? peakB : s.hold_b * 0.9f;
    }
    state[b] = s;
}

// report finalisation: gain = peakGain * 0.5f (SamplerSynthVoice.cpp:266).  The call's results (reports, gains,
// statistics) are written straight into mapped host memory: no copy command sits between two calls on the stream.
__global__ void zl_k_reports(const ZlReport *reports, int V, float *gain_out, ZlReport *host_reports, float *host_gain,
                             const ZlBatchStats *stats, ZlBatchStats *host_stats)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0 && host_stats) {
        *host_stats = *stats;
        ZlBatchStats z; z.source_bytes = 0; z.slow_blocks = 0; z.active_frames = 0;
        *const_cast<ZlBatchStats *>(stats) = z;                    // cleared for the call that reuses this slot
    }
    if (v >= V) return;
    const ZlReport r = reports[v];
    const float g = __uint_as_float(r.peak_bits) * 0.5f;
    gain_out[v] = g;
    if (host_reports) { host_reports[v] = r; host_gain[v] = g; }
}

// ------------------------------------------------------------------------------------------------
// JackPassthrough: in [B][2][frames] -> out [B][6][frames].  Pure streaming (8 B read, 24 B written per bus frame):
// VEC = 4 frames per lane with 16-byte accesses when frames % 4 == 0 and the buffers are 16-byte aligned.
template <int VEC>
__global__ void __launch_bounds__(256) zl_k_passthrough(const ZlPassParams *params, const float *in, float *out, long long frames)
{
    const int bus = blockIdx.y;
    const ZlPassParams p = params[bus];
    const float *inL = in + (size_t)bus * 2 * frames, *inR = inL + frames;
    float *o = out + (size_t)bus * 6 * frames;
    const float amounts[3] = { p.dry, p.fx1, p.fx2 };
    float lm, rm; zl_pass_pan(p, lm, rm);
    const long long nvec = frames / VEC;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
        float sl[VEC], sr[VEC];
        if (VEC == 4) {
            const float4 a = reinterpret_cast<const float4 *>(inL)[i], b = reinterpret_cast<const float4 *>(inR)[i];
            sl[0] = a.x; sl[1 % VEC] = a.y; sl[2 % VEC] = a.z; sl[3 % VEC] = a.w;
            sr[0] = b.x; sr[1 % VEC] = b.y; sr[2 % VEC] = b.z; sr[3 % VEC] = b.w;
        } else { sl[0] = inL[i]; sr[0] = inR[i]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float ol[VEC], orr[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) zl_pass_pair(p, amounts[c], lm, rm, sl[j], sr[j], ol[j], orr[j]);
            float *oL = o + (size_t)(2 * c) * frames, *oR = oL + frames;
            if (VEC == 4) {
                reinterpret_cast<float4 *>(oL)[i] = make_float4(ol[0], ol[1 % VEC], ol[2 % VEC], ol[3 % VEC]);
                reinterpret_cast<float4 *>(oR)[i] = make_float4(orr[0], orr[1 % VEC], orr[2 % VEC], orr[3 % VEC]);
            } else { oL[i] = ol[0]; oR[i] = orr[0]; }
        }
    }
}

// Bounce delivery (zlhip_bounce): a rendered sub-batch [B][2][frames] fp32 leaves the device buffer for its place in the caller's
// buffer, whose rows are `total` frames long.  PCM = the recorder's 16-bit format (zl_render.h, zl_pcm16), [B][total][2]; otherwise
// the floats as they are, [B][2][total].  Four frames per lane: 16-byte loads, one (PCM) or two 16-byte stores.  The engine uses it
// for the 16-bit conversion into a device staging buffer (total = frames); the copy engine moves the rows to the host.
// VEC = 4: four frames per lane where rows, offset and length allow 16-byte accesses, and a per-frame tail for the last frames % 4 frames;
// VEC = 1: every frame on its own (rows or offsets that are no multiple of four frames: periods of 441 or 33 frames with odd windows).
template <bool PCM, int VEC>
__global__ void __launch_bounds__(256) zl_k_deliver(const float *bus, void *out, long long in_stride, long long off, long long frames, long long total)
{
    // frames [off, off + frames) of every bus row (rows are in_stride floats apart) -> the same frames of the output (rows of `total` frames)
    const int b = blockIdx.y;
    const float *Ls = bus + (size_t)b * 2 * in_stride + off, *Rs = bus + ((size_t)b * 2 + 1) * in_stride + off;
    auto pair = [](float a, float c) { return (uint32_t)(uint16_t)zl_pcm16(a) | ((uint32_t)(uint16_t)zl_pcm16(c) << 16); };
    const long long nvec = VEC == 4 ? frames / 4 : 0;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    if (VEC == 4) {
        const float4 *L = reinterpret_cast<const float4 *>(Ls), *R = reinterpret_cast<const float4 *>(Rs);
        for (long long i = tid; i < nvec; i += nth) {
            const float4 l = L[i], r = R[i];
            if (PCM) {
                reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + ((size_t)b * total + off) * 2)[i] = make_uint4(pair(l.x, r.x), pair(l.y, r.y), pair(l.z, r.z), pair(l.w, r.w));
            } else {
                float *o = static_cast<float *>(out) + (size_t)b * 2 * total + off;
                reinterpret_cast<float4 *>(o)[i] = l;
                reinterpret_cast<float4 *>(o + total)[i] = r;
            }
        }
    }
    for (long long i = nvec * 4 + tid; i < frames; i += nth) {     // the tail (VEC = 4: at most three frames), or everything (VEC = 1)
        const float l = Ls[i], r = Rs[i];
        if (PCM) reinterpret_cast<uint32_t *>(static_cast<int16_t *>(out) + ((size_t)b * total + off) * 2)[i] = pair(l, r);
        else { float *o = static_cast<float *>(out) + (size_t)b * 2 * total + off; o[i] = l; o[total + i] = r; }
    }
}

// planar (L, R) -> interleaved arena layout; R == nullptr copies mono
// nonfinite: set to 1 when a sample is NaN or infinite -- the kernel holds every value anyway; one OR over the workgroup, and a store
// (every writer writes the same word: no atomic) only from a workgroup that saw one.  The host turns "still 0" into ZL_SOUND_FINITE.
__global__ void zl_k_interleave(const float *L, const float *R, float *dst, int length, int pad, uint32_t *nonfinite)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < length;
    bool bad = false;
    if (i < length + pad) {
        const float l = in ? L[i] : 0.0f, r = (in && R) ? R[i] : 0.0f;
        bad = !zl_f32_bits_finite(__float_as_uint(l)) || !zl_f32_bits_finite(__float_as_uint(r));
        if (R) { dst[2 * i] = l; dst[2 * i + 1] = r; }
        else   { dst[i] = l; }
    }
    if (nonfinite) {
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (any && threadIdx.x == 0) __hip_atomic_store(nonfinite, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (called from zl_engine.cpp)
#define ZL_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int zl_launch_apply_ops(const ZlBatch &A, hipStream_t s)
{
    if (A.n_op_ranges <= 0 && A.n_clip_edits <= 0) return 0;
    hipLaunchKernelGGL(zl_k0_apply_ops, dim3((std::max(A.n_op_ranges, 0) + 63) / 64 + std::max(A.n_clip_edits, 0)), dim3(64), 0, s, A);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_plan(const ZlBatch &A, int force_slow, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k1_plan, dim3((A.V + 63) / 64), dim3(64), 0, s, A, force_slow);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_assemble(const ZlBatch &A, hipStream_t s)
{
    const int bpl = zl_k1c_blocks_per_lane(A);
    hipLaunchKernelGGL(zl_k1c_assemble, dim3((A.V + 63) / 64, (A.K + bpl - 1) / bpl), dim3(64), 0, s, A, bpl);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_order(const ZlBatch &A, int32_t *order, int nslots, int norun, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k1o_order, dim3(nslots), dim3(256), 0, s, A, order, norun);
    ZL_LAUNCH_CHECK();
    return 0;
}

// what zl_k2_launch (zl_launch.h) takes from the environment and the code object: read once per process
const ZlK2Switches &zl_k2_switches()
{
    static const ZlK2Switches sw = [] {
        ZlK2Switches w = zl_k2_env_switches();
        w.pair_lds = ZL_K2_PAIR_LDS;
        hipFuncAttributes fa;
        w.pair_static_lds = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(zl_k2_pair_render)) == hipSuccess ? (int)fa.sharedSizeBytes : ZL_K2_PAIR_LDS;
        w.st_ring = 4 * ZL_ST_D * ZL_ST_SLOT;
        return w;
    }();
    return sw;
}

// K2 as zl_k2_launch describes it: nothing is decided here.  The switch's key spells the kernel's template arguments.
static constexpr int zl_k2_key(int kernel, int bpw, bool st, int mode) { return ((kernel * 8 + bpw) * 2 + (st ? 1 : 0)) * 8 + mode; }

int zl_launch_render(const ZlBatch &A, const ZlK2Launch &L, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const dim3 grid(L.gx, L.gy, L.gz), block(L.threads);
    ZlBatch At = A;
    At.tail_from = L.tail_from; At.tail_split = L.tail_split; At.tail_nb = L.tail_nb;
    At.order = L.order ? A.order : nullptr;
    // ev_start / ev_stop (profiling): the kernel's own begin / end timestamps, taken by the dispatch packet itself -- no
    // event packets around the launch for the command processor to handle
#define ZL_GO(...) hipExtLaunchKernelGGL((__VA_ARGS__), grid, block, L.dyn_lds, s, ev_start, ev_stop, 0, At); break;
    switch (zl_k2_key(L.kernel, L.bpw, L.staged, (int)(A.mode & 7u))) {
#define ZL_CASE(M) \
    case zl_k2_key(ZL_K2_RENDER, 4, true, M):        ZL_GO(zl_k2_render<M, 4, true>) \
    case zl_k2_key(ZL_K2_RENDER, 2, true, M):        ZL_GO(zl_k2_render<M, 2, true>) \
    case zl_k2_key(ZL_K2_RENDER, 1, true, M):        ZL_GO(zl_k2_render<M, 1, true>) \
    case zl_k2_key(ZL_K2_RENDER, 4, false, M):       ZL_GO(zl_k2_render<M, 4, false>) \
    case zl_k2_key(ZL_K2_RENDER, 2, false, M):       ZL_GO(zl_k2_render<M, 2, false>) \
    case zl_k2_key(ZL_K2_PHASE_RENDER, 1, false, M): ZL_GO(zl_k2_phase_render<M>) \
    case zl_k2_key(ZL_K2_RENDER, 1, false, M):       ZL_GO(zl_k2_render<M, 1, false>)
        ZL_CASE(0) ZL_CASE(1) ZL_CASE(2) ZL_CASE(3) ZL_CASE(4) ZL_CASE(5) ZL_CASE(6) ZL_CASE(7)
#undef ZL_CASE
    case zl_k2_key(ZL_K2_PAIR_RENDER, 1, false, 0):       ZL_GO(zl_k2_pair_render)
    case zl_k2_key(ZL_K2_PAIR_PHASE_RENDER, 1, false, 0): ZL_GO(zl_k2_pair_phase_render)
    default: return (int)hipErrorInvalidValue;                     // no kernel of that description: an error, never another kernel
    }
#undef ZL_GO
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_rt_loop(const ZlBatch &A, void *mailbox_dev, void *dev_state, unsigned long long first_seq, unsigned long long idle_ticks, float *gain_out,
                      ZlReport *host_reports, float *host_gain, ZlOpRange *dev_ranges, int vw, int threads, hipStream_t s)
{
    ZlRtShared *sh = reinterpret_cast<ZlRtShared *>(mailbox_dev);
    ZlRtDev *dv = reinterpret_cast<ZlRtDev *>(dev_state);
    const bool wide = A.groups > 1;                                // one workgroup per vw voices
    switch (A.mode & 7u) {
#define ZL_CASE(M) case M: \
        if (wide) hipLaunchKernelGGL((zl_k_rt_loop<M, true>), dim3(A.V / vw), dim3(threads), 0, s, A, sh, dv, first_seq, idle_ticks, gain_out, host_reports, host_gain, dev_ranges, vw); \
        else      hipLaunchKernelGGL((zl_k_rt_loop<M, false>), dim3(A.B), dim3(threads), 0, s, A, sh, dv, first_seq, idle_ticks, gain_out, host_reports, host_gain, dev_ranges, 0); \
        break;
        ZL_CASE(0) ZL_CASE(1) ZL_CASE(2) ZL_CASE(3) ZL_CASE(4) ZL_CASE(5) ZL_CASE(6) ZL_CASE(7)
#undef ZL_CASE
    }
    ZL_LAUNCH_CHECK();
    return 0;
}

// How many workgroups of the resident kernel the device holds at once (every one of them must be resident: a block is complete
// when all have arrived).  0 on error.
int zl_rt_loop_capacity(uint32_t mode, int wide, int threads, int device)
{
    int per_cu = 0, cus = 0;
    hipError_t st = hipErrorUnknown;
    switch (mode & 7u) {
#define ZL_CASE(M) case M: \
        st = wide ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zl_k_rt_loop<M, true>, threads, 0) \
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, zl_k_rt_loop<M, false>, threads, 0); \
        break;
        ZL_CASE(0) ZL_CASE(1) ZL_CASE(2) ZL_CASE(3) ZL_CASE(4) ZL_CASE(5) ZL_CASE(6) ZL_CASE(7)
#undef ZL_CASE
    }
    if (st != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return per_cu * cus;
}

int zl_launch_finalize(const ZlBatch &A, const float *bus_in, hipStream_t s)
{
    // nothing to sum (K2 wrote the bus, or the caller hands one over) and 16-byte aligned rows: the wave-per-block scan
    const float *scan = bus_in ? bus_in : (A.groups == 1 ? A.bus : nullptr);
    if (scan) {
        const long long pairs = (long long)A.K * A.B;
        hipLaunchKernelGGL(zl_k3_scan, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, A, scan);
    } else {
        hipLaunchKernelGGL(zl_k3_finalize, dim3(A.K, A.B), dim3(zl_whole_waves(A.N)), 0, s, A, bus_in);
    }
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_reports(const ZlReport *reports, int V, float *gain_out, ZlReport *host_reports, float *host_gain,
                      const ZlBatchStats *stats, ZlBatchStats *host_stats, hipStream_t s, hipEvent_t ev_done)
{
    // ev_done: the call's completion event rides on this dispatch (its stop event) instead of a packet of its own
    hipExtLaunchKernelGGL(zl_k_reports, dim3((V + 255) / 256), dim3(256), 0, s, nullptr, ev_done, 0, reports, V, gain_out, host_reports, host_gain, stats, host_stats);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_levels_tick(ZlLevelsState *state, const ZlBlockLevels *levels, int B, int N, int with_hold_bus, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k_levels_tick, dim3((B + 63) / 64), dim3(64), 0, s, state, levels, B, N, with_hold_bus);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_reduce_scan(const float *pieces, int npieces, long long stride, long long units, int N, int off, float *out, ZlUnitLevels *lv, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k_reduce_scan, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, s, pieces, npieces, stride, units, N, off, out, lv);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_group_reduce(const ZlGroupReduceArgs &a, int members, hipStream_t s)
{
    const long long pairs = a.p1 - a.p0;
    if (pairs <= 0) return 0;
    const dim3 grid((unsigned)((pairs + 3) / 4)), block(256);
    switch (members) {
    case 1: hipLaunchKernelGGL(zl_k_group_reduce_scan<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(zl_k_group_reduce_scan<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(zl_k_group_reduce_scan<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(zl_k_group_reduce_scan<4>, grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL(zl_k_group_reduce_scan<5>, grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL(zl_k_group_reduce_scan<6>, grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL(zl_k_group_reduce_scan<7>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(zl_k_group_reduce_scan<8>, grid, block, 0, s, a); break;
    default: return (int)hipErrorInvalidValue;
    }
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_levels_import(const ZlUnitLevels *units, ZlBlockLevels *levels, int B, int K, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k_levels_import, dim3((unsigned)((B * K + 255) / 256)), dim3(256), 0, s, units, levels, B, K);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_passthrough(const void *params_dev, const float *in, float *out, int B, long long frames, hipStream_t s)
{
    const bool vec = (frames % 4) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15u) == 0;
    long long nb = (frames / (vec ? 4 : 1) + 255) / 256;
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    if (vec) hipLaunchKernelGGL(zl_k_passthrough<4>, dim3((unsigned)nb, B), dim3(256), 0, s, (const ZlPassParams *)params_dev, in, out, frames);
    else     hipLaunchKernelGGL(zl_k_passthrough<1>, dim3((unsigned)nb, B), dim3(256), 0, s, (const ZlPassParams *)params_dev, in, out, frames);
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_deliver(const float *bus, void *out, int pcm16, int B, long long in_stride, long long off, long long frames, long long total, hipStream_t s)
{
    // 16-byte accesses need rows, offset and the output rows to start on multiples of four frames (the base pointers are allocations)
    const bool vec = ((in_stride | off | total) & 3) == 0 && (reinterpret_cast<uintptr_t>(bus) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    long long nb = ((vec ? frames / 4 : frames) + 255) / 256;
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    if (pcm16) { if (vec) hipLaunchKernelGGL((zl_k_deliver<true, 4>), dim3((unsigned)nb, B), dim3(256), 0, s, bus, out, in_stride, off, frames, total);
                 else     hipLaunchKernelGGL((zl_k_deliver<true, 1>), dim3((unsigned)nb, B), dim3(256), 0, s, bus, out, in_stride, off, frames, total); }
    else       { if (vec) hipLaunchKernelGGL((zl_k_deliver<false, 4>), dim3((unsigned)nb, B), dim3(256), 0, s, bus, out, in_stride, off, frames, total);
                 else     hipLaunchKernelGGL((zl_k_deliver<false, 1>), dim3((unsigned)nb, B), dim3(256), 0, s, bus, out, in_stride, off, frames, total); }
    ZL_LAUNCH_CHECK();
    return 0;
}

int zl_launch_interleave(const float *L, const float *R, float *dst, int length, int pad, uint32_t *nonfinite, hipStream_t s)
{
    hipLaunchKernelGGL(zl_k_interleave, dim3((length + pad + 255) / 256), dim3(256), 0, s, L, R, dst, length, pad, nonfinite);
    ZL_LAUNCH_CHECK();
    return 0;
}
