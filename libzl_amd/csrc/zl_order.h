// zl_order.h -- K2's launch order of a window's blocks, sorted by loop phase (K1o, zl_kernels.hip).
//
// A looping voice re-reads its loop once per pass: block k and block k + M / N read the same source lines.  In time order
// two such reads on one XCD are a whole pass apart -- a pass of every voice of the z-slot streams through the XCD's 4 MiB L2
// in between -- so every read misses L2.  Sorted by the loop phase of one key voice, the blocks that read the same lines
// are neighbours in launch order: they run at the same time on the same XCD (zl_k2_body gives XCD x one contiguous
// eighth of the launch slots) and the repeats hit L2.  K2's blocks are independent, so any permutation renders the same bits.
//
// Everything here is __host__ __device__: the CPU tier tests the keys, the key voice and the host reference of the sort
// (tests/cpu_harness/order_host.cpp); the product runs them in K1o only.
#pragma once
#include "zl_types.h"

#define ZL_ORDER_MAXBKT 2048      // phase buckets per z-slot (K1o's LDS histogram: 8 KB); longer loops get buckets of several blocks

// voices of z-slot z of the K2 grid: one bus (NB == 1, no mix groups) or NB consecutive narrow buses
ZL_HD inline void zl_order_slot_voices(int z, int NB, int VPB, int V, int &vb, int &ve)
{
    vb = z * NB * VPB;
    ve = vb + NB * VPB < V ? vb + NB * VPB : V;
}

// a voice can key the order: it plays through the whole window and has a periodic part (a sample-space loop in sustain)
ZL_HD inline bool zl_order_is_key(const ZlRunList &rl, int K)
{
    return rl.per_n > 0 && rl.per_M > 0 && rl.dead_from >= K;
}

struct ZlOrderKey { int t0, M, N, width, nbkt; };

// the key voice's phase buckets; false: no order (the window is no longer than one pass -- the sort would be time order
// rotated -- or nothing loops)
ZL_HD inline bool zl_order_setup(const ZlRunList &rl, int K, int N, ZlOrderKey &key)
{
    if (rl.per_n <= 0 || rl.per_M <= 0 || N <= 0 || (long long)K * N <= (long long)rl.per_M) return false;
    const int blocks = (rl.per_M + N - 1) / N;                     // buckets of one block's frames ...
    const int per = (blocks + ZL_ORDER_MAXBKT - 1) / ZL_ORDER_MAXBKT;   // ... or of `per` blocks' when the pass is long
    key.t0 = rl.per_t0; key.M = rl.per_M; key.N = N; key.width = per * N;
    key.nbkt = (rl.per_M + key.width - 1) / key.width;
    return true;
}

// exact phase of block k: its first frame's offset into the key voice's pass, in frames (0 .. M - 1)
ZL_HD inline long long zl_order_phase(const ZlOrderKey &key, int k)
{
    long long p = ((long long)k * key.N - key.t0) % key.M;
    if (p < 0) p += key.M;
    return p;
}

// bucket of block k: that offset in buckets (0 .. nbkt - 1)
ZL_HD inline int zl_order_bucket(const ZlOrderKey &key, int k)
{
    return (int)(zl_order_phase(key, k) / key.width);
}

// ---- the order INSIDE a bucket: by exact phase, ties by block number.  Two neighbouring slots share a workgroup (ZL_K2_PAIR_LAPS, zl_launch.h),
// and what they share of the source is largest between neighbours by exact phase.  A segment of at most ZL_ORDER_SORT_MAX entries is sorted; a
// longer one stays as placed (nothing depends on the order but speed).  K1o sorts the packed word (phase - bucket * width) << 16 | k, which needs
// the bucket's width within 15 bits and k within 16: wider buckets (width = per * N above 32768: blocks of more than 32768 frames, or a pass of
// more than 2048 such blocks that 32768 frames do not hold) stay as placed too, on the device and here.
#define ZL_ORDER_SORT_MAX 64
ZL_HD inline bool zl_order_sorts(const ZlOrderKey &key, int K) { return key.width <= 32768 && K <= 65536; }
ZL_HD inline unsigned zl_order_pack(const ZlOrderKey &key, int k)
{
    const long long p = zl_order_phase(key, k);
    return ((unsigned)(p - (p / key.width) * key.width) << 16) | (unsigned)k;
}

// ---- the slot's summary of its voices' inline runs, kept behind the order table.  K1o reads every run list of its slot anyway; the
// pair kernel's staging (zl_k2_stage_load) fetches a voice's run list only where an inline run can cover the block.
//   order[nslots * K + z]           run_end of z-slot z: no voice of the slot has an inline run that reaches block run_end or later
//   order[nslots * K + nslots + v]  runs[v].dead_from, dense: a staging wave reads its voices' words with one coalesced load
// first block behind the voice's last inline run; 0: it has none
ZL_HD inline int zl_order_run_end(const ZlRunList &rl)
{
    int e = 0;
    for (int j = 0; j < ZL_MAXRUNS; ++j) if (j < rl.n && rl.r[j].k1 > e) e = rl.r[j].k1;
    return e;
}

// ... and of the voices [vb, ve) of a slot.  on = 0 (ZL_K2_STAGE_NORUN=0): INT_MAX, every block fetches the run lists
ZL_HD inline int zl_order_slot_run_end(const ZlRunList *runs, int vb, int ve, int on)
{
    if (!on) return 0x7fffffff;
    int e = 0;
    for (int v = vb; v < ve; ++v) { const int ev = zl_order_run_end(runs[v]); e = ev > e ? ev : e; }
    return e;
}

ZL_HD inline size_t zl_order_tail_run_end(int nslots, int K, int z) { return (size_t)nslots * (size_t)K + (size_t)z; }
ZL_HD inline size_t zl_order_tail_dead(int nslots, int K, int v) { return (size_t)nslots * (size_t)K + (size_t)nslots + (size_t)v; }
// ints of the order buffer of a window: the table and the tail
ZL_HD inline size_t zl_order_ints(int nslots, int K, int V) { return (size_t)nslots * (size_t)K + (size_t)nslots + (size_t)V; }

// the launch shapes K2 can take an order in: one block per workgroup (not the 64- / 128-frame batch forms), no mix groups, not staged
inline bool zl_order_shape(int groups, int staged, int nblocks, int nframes)
{
    return groups == 1 && !staged && nblocks > 1 && nframes != 64 && nframes != 128;
}

// does a window of K blocks get the order?  mode = ZL_K2_PHASE_ORDER: 0 off, 1 auto, 2 wherever the shape allows.  Auto: blocks of
// 256 frames or more, no bounce, and the window longer than the shortest playing loop (ZlHostControl::phase_order_loop_frames:
// INFINITY unless every playing voice is cheap to plan)
inline bool zl_order_window(int mode, bool shape, bool bounce, int nframes, int K, double loopFrames)
{
    if (mode == 2) return shape;
    return mode == 1 && shape && !bounce && nframes >= 256 && (double)K * nframes > loopFrames;
}

// host reference of K1o for one z-slot: a stable counting sort of blocks [0, K) by bucket, then each bucket's segment by exact phase as K1o
// does (above; every bijection renders the same bits).  key == nullptr: the identity.  hist holds nbkt ints.
inline void zl_order_sort_host(const ZlOrderKey *key, int K, int *hist, int *order)
{
    if (!key) { for (int k = 0; k < K; ++k) order[k] = k; return; }
    for (int b = 0; b < key->nbkt; ++b) hist[b] = 0;
    for (int k = 0; k < K; ++k) ++hist[zl_order_bucket(*key, k)];
    int run = 0;
    for (int b = 0; b < key->nbkt; ++b) { const int c = hist[b]; hist[b] = run; run += c; }
    for (int k = 0; k < K; ++k) order[hist[zl_order_bucket(*key, k)]++] = k;
    // inside a bucket: by exact phase, ties by block number (hist[b] is now the end of bucket b's segment); an insertion sort of the packed words
    if (!zl_order_sorts(*key, K)) return;
    for (int b = 0, s = 0; b < key->nbkt; s = hist[b], ++b) {
        const int e = hist[b];
        if (e - s < 2 || e - s > ZL_ORDER_SORT_MAX) continue;
        for (int i = s + 1; i < e; ++i) {
            const int k = order[i];
            const unsigned w = zl_order_pack(*key, k);
            int j = i;
            for (; j > s && zl_order_pack(*key, order[j - 1]) > w; --j) order[j] = order[j - 1];
            order[j] = k;
        }
    }
}
