// zl_pair.h -- which K2 launches take the two-frames-per-lane kernels (zl_k2_pair_render / zl_k2_pair_phase_render, zl_kernels.hip).
//
// The pair form halves the load instructions of ON-GRID chunks only (a voice playing a clip at its own pitch and rate: lane j loads
// frames 2 j and 2 j + 1 of the source with one 16-byte load); every other chunk costs what it costs in zl_k2_body.  The kernels are
// built for one shape -- faithful linear mode, 256-frame blocks, one whole bus per workgroup -- and every other launch keeps the kernel
// it has.  HIP-free: the CPU tier tests the truth table (tests/cpu_harness/pair_host.cpp).
#pragma once
#include <stdint.h>

// the launch shapes the pair kernels exist for: mode exactly 0, blocks of 256 frames, a batch (K > 1: the resident kernel and single
// real-time blocks never), one bus per workgroup (no narrow-bus packing, no mix groups), register gathers (not LDS-staged), no position
// trace, no fused fan-out, no bounce sink, and the on-grid form switched on
inline bool zl_pair_shape(uint32_t mode, int N, int K, int NB, int groups, int staged, int trace, bool fan, bool host_out, int ongrid)
{
    return mode == 0u && N == 256 && K > 1 && NB == 1 && groups == 1 && !staged && !trace && !fan && !host_out && ongrid != 0;
}

// does a launch of that shape take them?  sw = ZL_K2_PAIR: 0 never, 1 auto, 2 wherever the shape allows (tests, A/B runs).  Auto: every
// playing voice is cheap to plan (unit ratio on a sample-space loop -- the voices whose interior blocks are on-grid; the flag that also
// decides the one-window call and the phase order).  A window of pitched voices gains nothing from the form.
inline bool zl_pair_window(int sw, bool shape, bool cheap)
{
    if (sw == 2) return shape;
    return sw == 1 && shape && cheap;
}

// does a pair launch read the scalar records K1c leaves (zl_render.h, ZL_ONGRID_SCALAR)?  sw = ZL_K2_PAIR_SCALAR (0 / 1); phase_order: the
// launch is zl_k2_pair_phase_render -- only it knows the blocks no inline run reaches (run_end, zl_order.h), and only there every record
// is an explicit one; have_tab: the engine has the buffer (mode 0).  A fast workgroup walks its bus in whole chunks of 8 voices read with
// one scalar load each: buses whose width is not a multiple of 8 (then some bus's first voice is not one either) never qualify.
inline bool zl_pair_scalar_window(int sw, bool pair, bool phase_order, bool have_tab, int VPB)
{
    return sw != 0 && pair && phase_order && have_tab && VPB > 0 && (VPB % 8) == 0;
}

// ---- two slots per workgroup (ZL_K2_PAIR_LAPS; zl_launch.h, zl_k2_pair_body): may the workgroup that holds blocks kA and kB of a bus render them in
// one walk (zl_k2_pair_fast2)?  One text for the kernel and for the CPU tier's count (tests/cpu_harness/pair_laps_host.cpp).
#if defined(__HIPCC__)
#define ZL_PAIR_HD __host__ __device__
#else
#define ZL_PAIR_HD
#endif
// the blocks: both at or behind run_end (every record an explicit one), neither the call's last block (`last`, in the window's numbering)
ZL_PAIR_HD inline bool zl_pair_laps_blocks(int kA, int kB, int run_end, int last) { return kA >= run_end && kB >= run_end && kA != last && kB != last; }
// the kinds zl_k2_pair_fast_kind gives the two (0 = not fast, 1 = stereo, 2 = mono): both fast and of one layout -> the walk's layout, else 0
ZL_PAIR_HD inline int zl_pair_laps_kind(int kindA, int kindB) { return kindA != 0 && kindA == kindB ? kindA : 0; }
