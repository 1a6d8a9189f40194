// Host build of K2's launch decision (libzl_amd/csrc/zl_launch.h) for the CPU tier -- TEST HARNESS ONLY.
#include "zl_launch.h"

extern "C" {

// n launches at once.  in: n rows of ZLLH_IN ints (the order of tests/test_k2_launch_cpu.py's IN); loop: n loop lengths in frames;
// sw: tail, tail_min, pad, pad_hermite, pair_pad, pair_static_lds, pair_lds, st_ring; out: n rows of ZLLH_OUT ints (the test's OUT).
enum { ZLLH_IN = 17, ZLLH_OUT = 13 };
void zllh_launch(int n, const int *in, const double *loop, const int *sw, int *out)
{
    ZlK2Switches s;
    s.tail = sw[0]; s.tail_min = sw[1]; s.pad = sw[2]; s.pad_hermite = sw[3]; s.pair_pad = sw[4]; s.pair_static_lds = sw[5]; s.pair_lds = sw[6]; s.st_ring = sw[7];
    for (int i = 0; i < n; ++i, in += ZLLH_IN, out += ZLLH_OUT) {
        ZlK2In a;
        a.mode = (uint32_t)in[0]; a.N = in[1]; a.K = in[2]; a.B = in[3]; a.groups = in[4]; a.NB = in[5];
        a.staged = in[6]; a.trace = in[7]; a.ongrid = in[8]; a.fan = in[9] != 0; a.host_out = in[10] != 0;
        a.order_mode = in[11]; a.call_blocks = in[12]; a.bounce = in[13] != 0; a.order_table = in[14] != 0; a.loop_frames = loop[i];
        a.pair_mode = in[15]; a.cheap = in[16] != 0;
        const ZlK2Launch L = zl_k2_launch(a, s);
        const int o[ZLLH_OUT] = { L.kernel, L.bpw, L.staged ? 1 : 0, (int)L.gx, (int)L.gy, (int)L.gz, (int)L.threads, (int)L.dyn_lds,
                                  L.tail_from, L.tail_split, L.tail_nb, L.order ? 1 : 0, L.scans_levels ? 1 : 0 };
        for (int j = 0; j < ZLLH_OUT; ++j) out[j] = o[j];
    }
}

// tail, tail_min, pad, pad_hermite, pair_pad as the environment sets them now
void zllh_env_switches(int *out)
{
    const ZlK2Switches s = zl_k2_env_switches();
    out[0] = s.tail; out[1] = s.tail_min; out[2] = s.pad; out[3] = s.pad_hermite; out[4] = s.pair_pad;
}

int zllh_narrow_buses(int nblocks, int groups, int VPB, int B, int nframes) { return zl_k2_narrow_buses(nblocks, groups, VPB, B, nframes); }

int zllh_whole_waves(int nframes) { return zl_whole_waves(nframes); }

// the call's windows as (first block, blocks) pairs into out (room for cap pairs); returns how many there are.  first_window_frames < 0: no override
int zllh_windows(int nblocks, int nframes, int windowBlocks, long long windowFrames, int windowCap, int mul, int twoSets, int behindPrev,
                 int first_window_frames, int *out, int cap)
{
    std::vector<std::pair<int, int>> wins;
    zl_plan_windows(nblocks, nframes, windowBlocks, (size_t)windowFrames, windowCap, (size_t)mul, twoSets != 0, behindPrev != 0,
                    first_window_frames >= 0 ? &first_window_frames : nullptr, wins);
    for (size_t i = 0; i < wins.size() && (int)i < cap; ++i) { out[2 * i] = wins[i].first; out[2 * i + 1] = wins[i].second; }
    return (int)wins.size();
}

}
