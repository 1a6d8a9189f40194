// zl_launch.h -- which K2 kernel a plan window gets, with what grid, and how a call is cut into windows.
//
// One pure function from a window's launch inputs to its launch description (zl_k2_launch), and the two call-level rules in front of it
// (zl_k2_narrow_buses, zl_plan_windows).  zlhip_render_batch computes the description once per window and reads everything off it -- the
// order table's size, whether K1o and K3 run, the fused reports; zl_launch_render (zl_kernels.hip) copies it into the kernel arguments and
// launches from one switch.  HIP-free and host-only: the CPU tier holds the table of known answers and the invariants over a sweep of
// shapes (tests/cpu_harness/launch_host.cpp, tests/test_k2_launch_cpu.py) -- a GPU test cannot see which kernel ran.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "zl_order.h"
#include "zl_pair.h"

// (whole waves: a block of 100 frames runs on 128 lanes, one of 300 on two workgroups of 256)
inline int zl_whole_waves(int nframes) { return nframes < 256 ? ((nframes + 63) & ~63) : 256; }

// narrow buses in batches: several whole buses per K2 workgroup (voices of consecutive buses are contiguous); needs the
// bus width to be a multiple of K2's chunk of 8 voices, no mix groups, one frame tile per block
inline int zl_k2_narrow_buses(int nblocks, int groups, int VPB, int B, int nframes)
{
    if (nblocks > 1 && groups == 1 && VPB <= 64 && (VPB % 8) == 0 && nframes <= 256) return std::max(1, std::min(128 / VPB, B));
    return 1;
}

// ---- plan windows: (first block, blocks) of a call of nblocks blocks -------------------------------------------------------------
// Large windows keep K2 launches long (their ramp-up and drain are a fixed cost per launch), but planning window i+1 must fit behind
// rendering window i.  W: the windowBlocks override, else mul * windowFrames worth of blocks (mul: zlhip_render_batch's choice per call,
// ZL_WINDOW_MUL), under three caps.  firstWindowFrames: the ZL_FIRST_WINDOW_FRAMES override, or null.
#define ZL_K2_MAX_WINDOW 60000    // a K2 launch has one y slot per block (+ 1920 for a split tail): gridDim.y stays below 65536
inline void zl_plan_windows(int nblocks, int nframes, int windowBlocks, size_t windowFrames, int windowCap, size_t mul, bool twoSets,
                            bool behindPrev, const int *firstWindowFrames, std::vector<std::pair<int, int>> &wins)
{
    int W = windowBlocks > 0 ? windowBlocks : (int)std::max<size_t>(1, std::min<size_t>(mul * windowFrames / (size_t)nframes, (size_t)1 << 30));
    W = std::min(W, windowCap);
    W = std::min(W, (1 << 30) / nframes);                          // window time is a 32-bit frame index in K1 / K1c
    W = std::min(W, ZL_K2_MAX_WINDOW);
    wins.clear();
    // when the previous call is still in flight (behindPrev) its rendering hides the planning of this call's first window: no
    // need to start small (fewer, longer K2 launches)
    if (nblocks <= W || !twoSets || behindPrev) {
        for (int k0 = 0; k0 < nblocks; k0 += W) wins.push_back({k0, std::min(W, nblocks - k0)});
        return;
    }
    // nothing hides the planning of this call's first window: a quarter-size window first (its planning is short,
    // and its rendering is long enough to hide the planning of a full window), then full windows.  (Doubling from
    // 64 Ki frames cost three small, inefficient K2 launches: +280 us per such call against +110 us.)
    int size = std::min(W, std::max(1, (firstWindowFrames ? *firstWindowFrames : (int)std::min<size_t>(windowFrames / 4, (size_t)1 << 28)) / nframes));
    for (int k0 = 0; k0 < nblocks;) {
        const int n = std::min(size, nblocks - k0);
        wins.push_back({k0, n});
        k0 += n;
        size = W;
    }
}

// ---- one window's K2 launch ------------------------------------------------------------------------------------------------------
// what the launcher reads once per process from the environment and from the code object (zl_k2_switches, zl_kernels.hip)
struct ZlK2Switches {
    int tail = 1;                 // ZL_K2_TAIL: 0 = no split tail
    int tail_min = 2048;          // ZL_K2_TAIL_MIN_BLOCKS (at least 8; the test tier lowers it): a window long enough to have a tail worth splitting
    int pad = -1;                 // ZL_K2_LDS_PAD, ZL_K2_LDS_PAD_HERMITE, ZL_K2_PAIR_LDS_PAD: dynamic LDS of the launch in bytes, -1 = the default below
    int pad_hermite = -1;
    int pair_pad = -1;
    int pair_static_lds = 0;      // static LDS of zl_k2_pair_render (hipFuncGetAttributes)
    int pair_lds = 0;             // ZL_K2_PAIR_LDS: LDS per workgroup a pair launch pads to
    int st_ring = 0;              // the staged kernels' ring: 4 waves * ZL_ST_D * ZL_ST_SLOT bytes
};

// the five of them the environment sets (the code object's three are the launcher's to fill in)
inline ZlK2Switches zl_k2_env_switches()
{
    auto env = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
    ZlK2Switches w;
    w.tail = env("ZL_K2_TAIL", w.tail);
    if (getenv("ZL_K2_TAIL_MIN_BLOCKS")) w.tail_min = std::max(8, env("ZL_K2_TAIL_MIN_BLOCKS", 0));    // (the test tier lowers it)
    w.pad = env("ZL_K2_LDS_PAD", w.pad);
    w.pad_hermite = env("ZL_K2_LDS_PAD_HERMITE", w.pad_hermite);
    w.pair_pad = env("ZL_K2_PAIR_LDS_PAD", w.pair_pad);
    return w;
}

struct ZlK2In {
    uint32_t mode;
    int N, K, B, groups, NB;      // frames per block, blocks of the window, buses, mix groups per bus, buses per workgroup (zl_k2_narrow_buses)
    int staged, trace, ongrid;    // ZlBatch's flags of the same names
    bool fan, host_out;           // fused fan-out; bounce with direct delivery
    // the phase order (zl_order.h): ZL_K2_PHASE_ORDER, blocks of the whole call, a bounce sink, ZlHostControl::phase_order_loop_frames, and
    // whether the window's record set has an order table (the sizing pass in front of the windows says yes)
    int order_mode, call_blocks;
    bool bounce, order_table;
    double loop_frames;
    // two frames per lane (zl_pair.h): ZL_K2_PAIR, and the call's "every playing voice is cheap to plan"
    int pair_mode;
    bool cheap;
    // phase-neighbour slots per workgroup of zl_k2_pair_phase_render (zl_k2_pair_laps): ZL_K2_PAIR_LAPS where the window can have the scalar
    // records (zl_pair_scalar_window with the launch's own two answers taken as yes), else 1
    int pair_laps = 1;
};

enum ZlK2Kernel { ZL_K2_RENDER, ZL_K2_PHASE_RENDER, ZL_K2_PAIR_RENDER, ZL_K2_PAIR_PHASE_RENDER };

struct ZlK2Launch {
    int kernel;                   // ZlK2Kernel
    int bpw; bool staged;         // template arguments of zl_k2_render: blocks per workgroup, LDS-staged source windows
    unsigned gx, gy, gz, threads, dyn_lds;
    int tail_from, tail_split, tail_nb;   // ZlBatch's fields of the same names (tail_from 0: no split tail)
    bool order;                   // the launch reads A.order: K1o runs for the window, the table holds gz * K entries
    bool scans_levels;            // K2 writes the window's ZlBlockLevels itself: no K3
    int laps;                     // slots of a bus's order per workgroup (1; 2 in a zl_k2_pair_phase_render launch that asked for it: gy = ceil(K / laps))
};

// slots per workgroup of a pair launch: sw = ZL_K2_PAIR_LAPS (1 = one block per workgroup, 2 = default; the kernel is built for 1 and 2),
// scalar = the window has the scalar records once its launch is zl_k2_pair_phase_render (zl_pair_scalar_window) -- the two-slot walk
// exists in the scalar-record text only
inline int zl_k2_pair_laps(int sw, bool scalar) { return scalar && sw >= 2 ? 2 : 1; }

inline ZlK2Launch zl_k2_launch(const ZlK2In &in, const ZlK2Switches &sw)
{
    const int N = in.N, K = in.K, NB = in.NB;
    ZlK2Launch L{};
    L.laps = 1;
    // blocks of 64 / 128 frames: 4 / 2 blocks per workgroup (batches only; a single block keeps its small workgroup; other lengths
    // below 256 -- 16, 32, 48, 100 ... -- are real-time periods: one block per workgroup of whole waves)
    L.bpw = ((N == 64 || N == 128) && K > 1) ? 256 / N : 1;
    L.threads = L.bpw > 1 ? 256u : (unsigned)zl_whole_waves(N);
    L.gx = L.bpw > 1 ? 1u : ((unsigned)N + L.threads - 1) / L.threads;
    L.gy = (unsigned)((K + L.bpw - 1) / L.bpw);
    L.gz = (unsigned)(NB > 1 ? (in.B + NB - 1) / NB : in.B * in.groups);
    // K2 scans the block for AudioLevels itself when one workgroup holds the whole block of the final mix
    L.scans_levels = in.groups == 1 && L.gx == 1;
    L.tail_from = 0; L.tail_split = 1; L.tail_nb = NB;
    // two frames per lane (zl_k2_pair_body): the call asked for it (zl_pair_window) and the launch has the shape the kernels are built
    // for.  128 lanes per block; dynamic LDS pads a workgroup to ZL_K2_PAIR_LDS, which holds the launch at 8 workgroups per CU = 4 waves
    // per SIMD and leaves the planner its wave slot and its LDS, as the 5-workgroup cap below does for the 256-lane kernels.
    const bool pair = zl_pair_window(in.pair_mode, zl_pair_shape(in.mode, N, K, NB, in.groups, in.staged, in.trace, in.fan, in.host_out, in.ongrid), in.cheap);
    // the phase order exists for one block per workgroup, register gathers (zl_order_shape)
    L.order = in.order_table && zl_order_window(in.order_mode, zl_order_shape(in.groups, in.staged, in.call_blocks, N), in.bounce, N, K, in.loop_frames);
    if (pair) {
        L.kernel = L.order ? ZL_K2_PAIR_PHASE_RENDER : ZL_K2_PAIR_RENDER;
        L.threads = 128;
        // two phase-neighbour slots per workgroup: workgroup w of a bus holds slots 2 w and 2 w + 1 of its order (the last one alone when K is odd)
        if (L.kernel == ZL_K2_PAIR_PHASE_RENDER && in.pair_laps > 1) { L.laps = 2; L.gy = (unsigned)((K + 1) / 2); }
        L.dyn_lds = (unsigned)(sw.pair_pad >= 0 ? sw.pair_pad : std::max(0, sw.pair_lds - sw.pair_static_lds));
        return L;
    }
    L.kernel = L.order ? ZL_K2_PHASE_RENDER : ZL_K2_RENDER;
    // LDS-staged source windows: batches only, whole 256-thread workgroups; the ring is dynamic LDS
    L.staged = in.staged && K > 1 && L.threads == 256;
    // split tail (see zl_k2_body): one workgroup per block holding ALL the buses, a window long enough to have a tail worth splitting
    if (sw.tail && L.bpw == 1 && NB > 1 && NB == in.B && L.gz == 1 && L.gx == 1 && !L.staged && K >= sw.tail_min) {
        const int split = (NB % 4 == 0) ? 4 : (NB % 2 == 0) ? 2 : 1;
        if (split > 1) {
            const int T = std::min(K / 4, 640);                    // half a generation of workgroups (5 per CU x 256 CUs)
            L.tail_from = K - T; L.tail_split = split; L.tail_nb = NB / split;
            L.gy = (unsigned)(L.tail_from + T * split);
        }
    }
    // One-block-per-workgroup kernels fill every SIMD's register file (6 waves x 80 VGPRs; 5 x 96 with 4 taps) and
    // leave no room for a planning wave (88 VGPRs): a K1 launch that arrives after K2 has filled the machine then
    // crawls (measured 550 instead of 130 us).  Unused dynamic LDS caps K2 at 5 workgroups per CU (27 KB each of
    // 160 KB) -- one wave slot per SIMD stays free for the planner, and K2 itself is 0.5 % faster that way.
    // (ZL_K2_LDS_PAD=0 -- the sixth workgroup per CU -- was measured again after the planner became a single sweep: K2 itself gains
    // 1..3 %, but a planner launch that arrives just after K2 has filled the machine then waits for the whole K2 launch every now
    // and then (2.5 ms instead of 35 us), and across boxes the calls gain nothing: the cap stays.)
    const int pad = (in.mode & ZL_MODE_HERMITE) ? (sw.pad_hermite >= 0 ? sw.pad_hermite : 0) : (sw.pad >= 0 ? sw.pad : 10240);
    L.dyn_lds = (unsigned)(L.staged ? sw.st_ring : L.bpw > 1 ? 0 : pad);
    return L;
}
