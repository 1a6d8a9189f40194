// The warp's harness walk (tests/cpu_harness/warp_host.cpp) over random calls with buffers of exactly the size needed, as a program of
// its own so that it can be built with -fsanitize=address,undefined (tests/test_warp_cpu.py): a read or write outside a clip's floats,
// an extent, the offsets or the staging arrays is the sanitizer's to find, a float written twice or not at all the program's.
//   warp_check <seed> <calls>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "../cpu_harness/warp_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 20;
    std::mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const double rates[4] = { 300.0, 1000.0, 2000.0, 8000.0 };
    long applied = 0, segments = 0;
    for (int call = 0; call < calls; ++call) {
        const int n = pick(1, 6);
        std::vector<std::vector<zlhip_warp_anchor>> anchors((size_t)n);
        std::vector<std::vector<float>> src((size_t)n), dst((size_t)n);
        std::vector<std::vector<int32_t>> writes((size_t)n), offs((size_t)n);
        std::vector<int32_t> counts((size_t)n), length((size_t)n), channels((size_t)n);
        std::vector<int64_t> nsrc((size_t)n);
        std::vector<double> rate((size_t)n);
        std::vector<zlhip_warp> out((size_t)n);
        std::vector<uint32_t> verdicts((size_t)n, 0u);
        for (int i = 0; i < n; ++i) {
            rate[(size_t)i] = rates[pick(0, 3)];
            channels[(size_t)i] = pick(1, 2);
            const int32_t O = zl_wp_overlap(rate[(size_t)i]);
            // regions drawn until they are acceptable: a copy, or a stretch with tau in [0.25, 4]
            std::vector<zlhip_warp_anchor> &an = anchors[(size_t)i];
            an.push_back({0, 0});
            const int regions = pick(1, 5);
            for (int r = 0; r < regions; ++r) {
                for (int attempt = 0; ; ++attempt) {
                    const int base = (int)(rate[(size_t)i] * 0.12);
                    int A = pick(base / 2, base * 3), D = pick(0, 3) == 0 ? A : pick(A / 4 + 1, A * 4);
                    if (attempt > 200) D = A;
                    ZlWpRegion R;
                    if (A < 1 || zl_wp_region(rate[(size_t)i], O, 0, 0, A, D, ZL_WP_RATIO, &R) != 0) continue;
                    an.push_back({an.back().src_frame + A, an.back().dst_frame + D});
                    break;
                }
            }
            counts[(size_t)i] = (int32_t)an.size();
            length[(size_t)i] = an.back().src_frame;
            zlhip_warp s;
            if (zlwp_resolve(rate[(size_t)i], length[(size_t)i], an.data(), counts[(size_t)i], &s) != 0) { printf("a drawn request does not resolve\n"); return 1; }
            src[(size_t)i].resize((size_t)length[(size_t)i] * (size_t)channels[(size_t)i]);
            for (float &v : src[(size_t)i]) v = (float)pick(-1000, 1000) / 1000.0f;
            nsrc[(size_t)i] = (int64_t)src[(size_t)i].size();
            const size_t floats = (size_t)zlwp_extent_floats(s.length, channels[(size_t)i]);
            dst[(size_t)i].assign(s.applied ? floats : 0, -5.0f);
            writes[(size_t)i].assign(s.applied ? floats : 0, 0);
            offs[(size_t)i].assign((size_t)s.segments, -1);
        }
        std::vector<const zlhip_warp_anchor *> pA; std::vector<const float *> pSrc; std::vector<float *> pDst; std::vector<int32_t *> pW, pO;
        for (int i = 0; i < n; ++i) {
            pA.push_back(anchors[(size_t)i].data()); pSrc.push_back(src[(size_t)i].data()); pDst.push_back(dst[(size_t)i].data());
            pW.push_back(writes[(size_t)i].data()); pO.push_back(offs[(size_t)i].data());
        }
        int64_t walk[4];
        const int32_t rc = zlwp_call(n, counts.data(), pA.data(), pSrc.data(), nsrc.data(), length.data(), channels.data(), rate.data(), pDst.data(), pW.data(),
                                     out.data(), pO.data(), verdicts.data(), walk);
        if (rc < 0 || walk[3] != 0) { printf("call %d: status %d, %lld reads refused\n", call, rc, (long long)walk[3]); return 1; }
        for (int i = 0; i < n; ++i) {
            if (!out[(size_t)i].applied) continue;
            ++applied; segments += out[(size_t)i].segments;
            for (size_t k = 0; k < writes[(size_t)i].size(); ++k)
                if (writes[(size_t)i][k] != 1) { printf("call %d clip %d: float %zu written %d times\n", call, i, k, writes[(size_t)i][k]); return 1; }
            for (int32_t o : offs[(size_t)i]) if (o < 0) { printf("call %d clip %d: an offset not written\n", call, i); return 1; }
            if (verdicts[(size_t)i] != 0u) { printf("call %d clip %d: a finite clip lost its flag\n", call, i); return 1; }
        }
    }
    printf("warp check ok: %ld clips, %ld segments\n", applied, segments);
    return 0;
}
