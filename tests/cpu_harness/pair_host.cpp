// Host build of the gate of K2's two-frames-per-lane kernels (libzl_amd/csrc/zl_pair.h) for the CPU tier -- TEST HARNESS ONLY.
#include "zl_pair.h"

extern "C" {

int zlpg_shape(unsigned mode, int N, int K, int NB, int groups, int staged, int trace, int fan, int host_out, int ongrid)
{
    return zl_pair_shape(mode, N, K, NB, groups, staged, trace, fan != 0, host_out != 0, ongrid) ? 1 : 0;
}

// the whole gate, as zlhip_render_batch applies it to a window: the shape of the launch, the switch, the call's "cheap to plan" flag
int zlpg_window(int sw, int cheap, unsigned mode, int N, int K, int NB, int groups, int staged, int trace, int fan, int host_out, int ongrid)
{
    return zl_pair_window(sw, zl_pair_shape(mode, N, K, NB, groups, staged, trace, fan != 0, host_out != 0, ongrid), cheap != 0) ? 1 : 0;
}

}
