// Host build of the per-slot run summary behind K2's order table (libzl_amd/csrc/zl_order.h) for the CPU tier -- TEST HARNESS ONLY.
// zlsum_build replays what K1o (zl_kernels.hip) writes behind the table: run_end per z-slot, dead_from per voice.
// With -DZL_ORDER_SUMMARY_MAIN the file is a program of its own that runs hand-made cases (the sanitizer build).
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zl_order.h"

// buf holds zl_order_ints(nslots, K, V) ints: the order table (left alone) and the tail.  n, dead_from: per voice; k0k1: [V][ZL_MAXRUNS][2]
static int summary_build(int V, int VPB, int NB, int nslots, int K, int on, const int *n, const int *dead_from, const int *k0k1, int *buf)
{
    std::vector<ZlRunList> runs((size_t)V);
    for (int v = 0; v < V; ++v) {
        ZlRunList &rl = runs[(size_t)v];
        std::memset(&rl, 0, sizeof(ZlRunList));
        rl.n = n[v]; rl.dead_from = dead_from[v];
        for (int j = 0; j < ZL_MAXRUNS; ++j) {
            rl.r[j].k0 = k0k1[((size_t)v * ZL_MAXRUNS + (size_t)j) * 2];
            rl.r[j].k1 = k0k1[((size_t)v * ZL_MAXRUNS + (size_t)j) * 2 + 1];
        }
    }
    for (int z = 0; z < nslots; ++z) {
        int vb, ve;
        zl_order_slot_voices(z, NB, VPB, V, vb, ve);
        buf[zl_order_tail_run_end(nslots, K, z)] = zl_order_slot_run_end(runs.data(), vb, ve, on);
        for (int v = vb; v < ve; ++v) buf[zl_order_tail_dead(nslots, K, v)] = runs[(size_t)v].dead_from;
    }
    return (int)zl_order_ints(nslots, K, V);
}

extern "C" {

int zlsum_build(int V, int VPB, int NB, int nslots, int K, int on, const int *n, const int *dead_from, const int *k0k1, int *buf)
{
    return summary_build(V, VPB, NB, nslots, K, on, n, dead_from, k0k1, buf);
}

int zlsum_ints(int nslots, int K, int V) { return (int)zl_order_ints(nslots, K, V); }
int zlsum_run_end_index(int nslots, int K, int z) { return (int)zl_order_tail_run_end(nslots, K, z); }
int zlsum_dead_index(int nslots, int K, int v) { return (int)zl_order_tail_dead(nslots, K, v); }

}

#ifdef ZL_ORDER_SUMMARY_MAIN
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int K = 96, VPB = 4, V = 10, nslots = 3;                // the last slot is partial: voices 8 and 9
    std::vector<int> n((size_t)V, 0), dead((size_t)V, K), kk((size_t)V * ZL_MAXRUNS * 2, 0);
    auto run = [&](int v, int j, int k0, int k1) { kk[((size_t)v * ZL_MAXRUNS + (size_t)j) * 2] = k0; kk[((size_t)v * ZL_MAXRUNS + (size_t)j) * 2 + 1] = k1; };
    const int ints = (int)zl_order_ints(nslots, K, V);
    EXPECT(ints == nslots * K + nslots + V);
    std::vector<int> buf((size_t)ints, -7);
    // every voice n == 0
    EXPECT(summary_build(V, VPB, 1, nslots, K, 1, n.data(), dead.data(), kk.data(), buf.data()) == ints);
    for (int z = 0; z < nslots; ++z) EXPECT(buf[(size_t)(nslots * K + z)] == 0);
    for (int v = 0; v < V; ++v) EXPECT(buf[(size_t)(nslots * K + nslots + v)] == K);
    for (int i = 0; i < nslots * K; ++i) EXPECT(buf[(size_t)i] == -7);
    // one voice with two runs (stale entries behind n do not count), an idle voice, a voice that ends mid-window, runs in the partial slot
    n[1] = 2; run(1, 0, 0, 30); run(1, 1, 31, 61); run(1, 2, 70, 95);
    dead[2] = 0; dead[6] = 41;
    n[9] = ZL_MAXRUNS; for (int j = 0; j < ZL_MAXRUNS; ++j) run(9, j, 10 * j, 10 * j + 9);
    summary_build(V, VPB, 1, nslots, K, 1, n.data(), dead.data(), kk.data(), buf.data());
    EXPECT(buf[(size_t)(nslots * K + 0)] == 61 && buf[(size_t)(nslots * K + 1)] == 0 && buf[(size_t)(nslots * K + 2)] == 10 * (ZL_MAXRUNS - 1) + 9);
    EXPECT(buf[(size_t)(nslots * K + nslots + 2)] == 0 && buf[(size_t)(nslots * K + nslots + 6)] == 41 && buf[(size_t)(nslots * K + nslots + 9)] == K);
    // the switch off
    summary_build(V, VPB, 1, nslots, K, 0, n.data(), dead.data(), kk.data(), buf.data());
    for (int z = 0; z < nslots; ++z) EXPECT(buf[(size_t)(nslots * K + z)] == INT_MAX);
    // narrow buses: two buses per slot, the last slot holds one bus of two voices
    summary_build(V, VPB, 2, 2, K, 1, n.data(), dead.data(), kk.data(), buf.data());
    EXPECT(buf[(size_t)(2 * K + 0)] == 61 && buf[(size_t)(2 * K + 1)] == 10 * (ZL_MAXRUNS - 1) + 9);
    std::printf(failures ? "order summary: %d failures\n" : "order summary: ok\n", failures);
    return failures ? 1 : 0;
}
#endif
