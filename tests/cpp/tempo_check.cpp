// The tempo estimate's harness walk (tests/cpu_harness/tempo_host.cpp over libzl_amd/csrc/zl_tempo.h) in a stand-alone program, for a
// build with AddressSanitizer and UBSan (tests/test_tempo_cpu.py builds and runs it): every buffer has exactly the size the call
// needs, so a staged word, a lag or a record outside its array, a shift out of range or an overflowing signed product ends the program.
// The calls mix hops of 1, 2 and 3, segment and lag-tile edges, several segments, silence, loud energies and ranges too short for a tempo.
//   tempo_check <seed> <calls>        exit 0 and "tempo check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/tempo_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t sizes[] = {1, 2, 3, 4, 7, 130, 257, 655, 657, 659, 4095, 4096, 4097, 8193, 9000};
    const int32_t hopsizes[] = {64, 256, 4096};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 5);
        std::vector<int32_t> hops((size_t)nreq), hop((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        std::vector<float> lo((size_t)nreq), hi((size_t)nreq);
        std::vector<uint64_t> E;
        int64_t nh = 0, need = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            hops[(size_t)i] = sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
            hop[(size_t)i] = hopsizes[rng() % 3];
            rate[(size_t)i] = (rng() & 1) ? 48000.0 : 44100.0;
            lo[(size_t)i] = (rng() & 1) ? 75.0f : 60.0f; hi[(size_t)i] = (rng() & 1) ? 150.0f : 400.0f;
            int32_t h = hop[(size_t)i];
            if (zl_tp_resolve(rate[(size_t)i], &h, &lo[(size_t)i], &hi[(size_t)i]) != 0) { lo[(size_t)i] = 75.0f; hi[(size_t)i] = 150.0f; }
            const int kind = (int)(rng() % 4);                     // silence, quiet, loud, a pulse train
            for (int32_t k = 0; k < hops[(size_t)i]; ++k) {
                uint64_t e = 0;
                if (kind == 1) e = rng() % 100000;
                if (kind == 2) e = rng() % ((uint64_t)1 << 44);
                if (kind == 3) e = k % 37 == 0 ? ((uint64_t)1 << 40) + rng() % 1000 : rng() % 4096;
                E.push_back(e);
            }
            ZlTpRequest T; double a, b;
            zl_tp_lags(rate[(size_t)i], hop[(size_t)i], lo[(size_t)i], hi[(size_t)i], &a, &b);
            zl_tp_geometry(&T, hops[(size_t)i], a, b);
            need += T.nlags; nh += hops[(size_t)i];
        }
        std::vector<uint16_t> W((size_t)nh);
        std::vector<uint64_t> A((size_t)need);
        std::vector<int32_t> geom((size_t)nreq * 8);
        std::vector<ZlTpResult> out((size_t)nreq);
        int64_t walk[3];
        const int64_t used = zltp_call(nreq, hops.data(), rate.data(), hop.data(), lo.data(), hi.data(), E.data(), W.data(), A.data(), need, geom.data(), out.data(), nullptr, walk);
        assert(used == need);
        int64_t expect = 0;
        for (int32_t i = 0; i < nreq; ++i)
            for (int32_t l = 0; l < geom[(size_t)i * 8 + 4]; ++l) expect += hops[(size_t)i] - (geom[(size_t)i * 8 + 3] + l);
        assert(walk[0] == expect && walk[1] == 0 && walk[2] == 0);
        for (int32_t i = 0; i < nreq; ++i) {
            const ZlTpResult &r = out[(size_t)i];
            assert(r.hops == hops[(size_t)i] && r.shift >= 0 && r.shift <= 6);
            assert(r.lag_fine == 0 || (r.lag_fine >= r.lag_coarse && r.lag_coarse >= geom[(size_t)i * 8] && r.lag_coarse <= geom[(size_t)i * 8 + 1] && r.bpm > 0.0f));
        }
        total += walk[0];
    }
    printf("tempo check ok (%lld products)\n", (long long)total);
    return 0;
}
