// Host build of what decides K2's two-slot workgroups (ZL_K2_PAIR_LAPS) for the CPU tier -- TEST HARNESS ONLY: the launch decision with the new
// input (libzl_amd/csrc/zl_launch.h: zl_k2_launch, zl_k2_pair_laps), and, from the records of a SimSynth's last call (pair_scalar_host.cpp: zlps_scan)
// and the host order of each bus (zl_order.h), the workgroups of zl_k2_pair_phase_render that take the two-slot walk.
// -DZL_PAIR_LAPS_MAIN: a program of its own (for the sanitizers) that runs the launch sweep and the pairing over made-up records.
#include "pair_scalar_host.cpp"
#include "zl_launch.h"

// zl_k2_pair_body's choice for the workgroups of one bus, through the predicates the kernel calls (zl_pair.h: zl_pair_laps_blocks,
// zl_pair_laps_kind): order[K] the bus's slots, fast[K] the layout zl_k2_pair_fast_kind gives each block from its chunk bits alone (0 = not every chunk
// fast or two layouts; 1 / 2 = stereo / mono), run_end the bus's word.  walk[w] of workgroup w (ceil(K / 2) of them): 2 = the two-slot walk, 1 = its
// blocks one after the other (or one block alone).  Returns the number of walks.
static int pair_up(int K, const int *order, const int *fast, int run_end, int *walk)
{
    int n = 0;
    for (int w = 0; 2 * w < K; ++w) {
        const int s0 = 2 * w, nb = s0 + 2 <= K ? 2 : K - s0;
        const bool both = nb == 2 && zl_pair_laps_blocks(order[s0], order[s0 + 1], run_end, K - 1) && zl_pair_laps_kind(fast[order[s0]], fast[order[s0 + 1]]) != 0;
        walk[w] = both ? 2 : 1;
        n += both ? 1 : 0;
    }
    return n;
}

// the layout of (block k, bus b) from K1c's chunk bits alone, as zl_k2_pair_fast_kind reads them
static int fast_kind(const uint16_t *bits, int G, int k, int v0, int v1)
{
    bool all = true, anyMono = false, allMono = true;
    for (int g = v0 >> 6; g <= (v1 - 1) >> 6; ++g) {
        const uint32_t w = bits[(size_t)k * G + g], need = zl_pair_group_need(v0, v1, g);
        all = all && (w & need) == need;
        anyMono = anyMono || ((w >> 8) & need) != 0u;
        allMono = allMono && ((w >> 8) & need) == need;
    }
    return !all ? 0 : allMono ? 2 : anyMono ? 0 : 1;
}

extern "C" {

// one launch: the 17 ints and the loop length of tests/test_k2_launch_cpu.py's IN, sw as there, pair_laps = the new input (0: leave the
// member's default).  out: the 13 ints of that file's OUT and the launch's laps.
void zlpl_launch(const int *in, double loop, const int *sw, int pair_laps, int *out)
{
    ZlK2Switches s;
    s.tail = sw[0]; s.tail_min = sw[1]; s.pad = sw[2]; s.pad_hermite = sw[3]; s.pair_pad = sw[4]; s.pair_static_lds = sw[5]; s.pair_lds = sw[6]; s.st_ring = sw[7];
    ZlK2In a;
    a.mode = (uint32_t)in[0]; a.N = in[1]; a.K = in[2]; a.B = in[3]; a.groups = in[4]; a.NB = in[5];
    a.staged = in[6]; a.trace = in[7]; a.ongrid = in[8]; a.fan = in[9] != 0; a.host_out = in[10] != 0;
    a.order_mode = in[11]; a.call_blocks = in[12]; a.bounce = in[13] != 0; a.order_table = in[14] != 0; a.loop_frames = loop;
    a.pair_mode = in[15]; a.cheap = in[16] != 0;
    if (pair_laps) a.pair_laps = pair_laps;
    const ZlK2Launch L = zl_k2_launch(a, s);
    const int o[14] = { L.kernel, L.bpw, L.staged ? 1 : 0, (int)L.gx, (int)L.gy, (int)L.gz, (int)L.threads, (int)L.dyn_lds,
                        L.tail_from, L.tail_split, L.tail_nb, L.order ? 1 : 0, L.scans_levels ? 1 : 0, L.laps };
    for (int j = 0; j < 14; ++j) out[j] = o[j];
}

// ZL_K2_PAIR_LAPS and the scalar window's answer -> the launch's input
int zlpl_laps(int sw, int scalar) { return zl_k2_pair_laps(sw, scalar != 0); }

// the host order of every bus of the last call a SimSynth rendered (one z-slot per bus: NB = 1), as K1o forms it: order[B][K]
void zlpl_order(ZlSim *S, int32_t *order)
{
    const int K = S->lastK, N = S->lastN, B = S->B, VPB = S->VPB;
    std::vector<int> hist(ZL_ORDER_MAXBKT);
    for (int b = 0; b < B; ++b) {
        int vb, ve, kv = -1;
        zl_order_slot_voices(b, 1, VPB, S->V, vb, ve);
        for (int v = vb; v < ve && kv < 0; ++v) if (zl_order_is_key(S->runs[(size_t)v], K)) kv = v;
        ZlOrderKey key;
        const bool keyed = kv >= 0 && zl_order_setup(S->runs[(size_t)kv], K, N, key);
        zl_order_sort_host(keyed ? &key : nullptr, K, hist.data(), order + (size_t)b * K);
    }
}

// bits[K][G] and run_end[B] of zlps_scan and order[B][K] of zlpl_order -> walk[B][ceil(K / 2)]; returns the number of two-slot walks of the call
int zlpl_walks(int K, int B, int VPB, int V, const uint16_t *bits, const int32_t *run_end, const int32_t *order, int32_t *walk)
{
    const int W = (K + 1) / 2, G = (V + 63) / 64;
    std::vector<int> fb((size_t)K);
    int n = 0;
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < K; ++k) fb[(size_t)k] = fast_kind(bits, G, k, b * VPB, (b + 1) * VPB);
        n += pair_up(K, order + (size_t)b * K, fb.data(), run_end[b], walk + (size_t)b * W);
    }
    return n;
}

// the in-bucket order of zl_order_sort_host for a made-up key voice: t0, M = the loop in frames; order[K], phase[K] (of block k), bucket[K] (of block k),
// returns nbkt, or 0 where the window gets no order (the identity is written)
int zlpl_sort(int t0, int M, int N, int K, int32_t *order, long long *phase, int32_t *bucket)
{
    ZlRunList rl{};
    rl.per_n = 1; rl.per_M = M; rl.per_t0 = t0;
    ZlOrderKey key;
    std::vector<int> hist(ZL_ORDER_MAXBKT);
    if (!zl_order_setup(rl, K, N, key)) { zl_order_sort_host(nullptr, K, hist.data(), order); return 0; }
    zl_order_sort_host(&key, K, hist.data(), order);
    for (int k = 0; k < K; ++k) { phase[k] = zl_order_phase(key, k); bucket[k] = zl_order_bucket(key, k); }
    return key.nbkt;
}

}  // extern "C"

#ifdef ZL_PAIR_LAPS_MAIN
static int lfail(const char *what) { std::printf("pair laps: FAILED %s\n", what); return 1; }

int main()
{
    const int sw[8] = {1, 2048, -1, -1, -1, 17024, 18432, 0};
    long rows = 0, two = 0;
    for (int K : {1, 2, 3, 47, 48, 375, 8191, 8192}) for (int N : {128, 256, 512}) for (int NB : {1, 2}) for (int mode : {0, 1}) for (int pm : {0, 2})
        for (int om : {0, 2}) for (int tab : {0, 1}) {
            const int in[17] = {mode, N, K, 8, 1, NB, 0, 0, 3, 0, 0, om, K, 0, tab, pm, 1};
            int a[14], b[14], c[14];
            zlpl_launch(in, 96000.0, sw, 0, a);
            zlpl_launch(in, 96000.0, sw, 1, b);
            zlpl_launch(in, 96000.0, sw, 2, c);
            for (int j = 0; j < 14; ++j) if (a[j] != b[j]) return lfail("the default is not 1");
            const bool want = a[0] == ZL_K2_PAIR_PHASE_RENDER;
            if (a[13] != 1 || c[13] != (want ? 2 : 1) || c[4] != (want ? (K + 1) / 2 : a[4])) return lfail("gy or laps");
            for (int j = 0; j < 13; ++j) if (j != 4 && a[j] != c[j]) return lfail("something else than gy moved");
            ++rows; two += want ? 1 : 0;
        }
    if (two == 0 || two == rows) return lfail("the sweep has no (or only) two-slot launches");
    if (zl_k2_pair_laps(2, true) != 2 || zl_k2_pair_laps(2, false) != 1 || zl_k2_pair_laps(1, true) != 1 || zl_k2_pair_laps(0, true) != 1 || zl_k2_pair_laps(4, true) != 2) return lfail("the switch");
    // pairing over made-up records: K = 7, slots (3 0 | 6 2 | 5 1 | 4): layouts 1 1 | 1 0 | 2 2 | 1
    const int order[7] = {3, 0, 6, 2, 5, 1, 4}, kind[7] = {1, 2, 0, 1, 1, 2, 1};
    int walk[4];
    if (pair_up(7, order, kind, 0, walk) != 2 || walk[0] != 2 || walk[1] != 1 || walk[2] != 2 || walk[3] != 1) return lfail("the pairing");
    if (pair_up(7, order, kind, 1, walk) != 1 || walk[0] != 1) return lfail("block 0 in front of run_end");
    const int all1[7] = {1, 1, 1, 1, 1, 1, 1}, ord6[6] = {0, 1, 2, 3, 4, 5};
    if (pair_up(6, ord6, all1, 0, walk) != 2 || walk[2] != 1) return lfail("the call's last block");
    const int mixed[2] = {1, 2}, ord2[2] = {0, 1};
    if (pair_up(2, ord2, mixed, 0, walk) != 0 || pair_up(1, ord2, mixed, 0, walk) != 0) return lfail("two layouts, or one block");
    // the in-bucket order at the headline's key voice and at short loops
    for (int M : {95936, 100, 257, 300}) for (int K : {1, 2, 3, 47, 48, 375, 8192}) {
        std::vector<int32_t> ord((size_t)K), bk((size_t)K); std::vector<long long> ph((size_t)K);
        const int nbkt = zlpl_sort(5, M, 256, K, ord.data(), ph.data(), bk.data());
        std::vector<char> seen((size_t)K, 0);
        for (int i = 0; i < K; ++i) { if (ord[i] < 0 || ord[i] >= K || seen[ord[i]]) return lfail("the order is no bijection"); seen[ord[i]] = 1; }
        if (nbkt) for (int i = 1; i < K; ++i) if (bk[ord[i]] < bk[ord[i - 1]]) return lfail("buckets decrease");
    }
    std::printf("pair laps: ok (%ld launches, %ld with two slots)\n", rows, two);
    return 0;
}
#endif
