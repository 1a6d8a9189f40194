// The loudness measurement's harness walk (tests/cpu_harness/loudness_host.cpp over libzl_amd/csrc/zl_loudness.h) in a stand-alone
// program, for a build with AddressSanitizer and UBSan (tests/test_loudness_cpu.py builds and runs it): every buffer has exactly the
// size the call needs -- a sound holds length * channels floats and not one more, the records hold the call's items and not one more --
// so an element read outside a request, a record outside its array or an overflowing signed product ends the program.  The calls mix
// mono and stereo, two rates, odd first frames, sub-blocks from 16 to the default, the short rule, one-frame requests and remainders.
//   loudness_check <seed> <calls>        exit 0 and "loudness check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/loudness_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t subs[] = {16, 17, 64, 100, 441, 0};
    const int32_t firsts[] = {0, 1, 3, 5};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 9);
        std::vector<zlhip_loudness_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        int64_t items = 0, expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t ch = 1 + (int32_t)(rng() & 1), first = firsts[rng() % 4];
            int32_t sub = subs[rng() % 6];
            rate[(size_t)i] = (rng() & 1) ? 48000.0 : 44100.0;
            const int32_t rsub = sub ? sub : zl_ld_default_sub(rate[(size_t)i]);
            const int kind = (int)(rng() % 4);                     // one frame, the short rule, whole sub-blocks, a remainder
            const int32_t n = kind == 0 ? 1 : (kind == 1 ? 1 + (int32_t)(rng() % (uint64_t)(4 * rsub - 1)) : (4 + (int32_t)(rng() % 6)) * rsub + (kind == 3 ? 1 + (int32_t)(rng() % (uint64_t)(rsub - 1)) : 0));
            zlhip_loudness_request &q = reqs[(size_t)i];
            q.id = 0; q.first_frame = first; q.num_frames = n; q.sub_frames = sub;
            length[(size_t)i] = first + n + (int32_t)(rng() % 3);
            channels[(size_t)i] = ch;
            std::vector<float> &s = sounds[(size_t)i];
            s.resize((size_t)length[(size_t)i] * (size_t)ch);
            const int content = (int)(rng() % 3);                  // silence, noise, a tone
            for (size_t k = 0; k < s.size(); ++k) {
                float v = 0.0f;
                if (content == 1) v = (float)((double)(rng() % 2001) - 1000.0) / 2000.0f;
                if (content == 2) v = 0.4f * (float)sin(6.283185307179586 * (double)(k / (size_t)ch) / 48.0);
                s[k] = v;
            }
            data[(size_t)i] = s.data();
            const int64_t S = n / rsub;
            items += zl_ld_items(n, rsub);
            expect += (S >= 4 ? S * rsub : (int64_t)n) * ch;
        }
        std::vector<ZlLdSub> recs((size_t)items);
        std::vector<int32_t> base((size_t)nreq);
        std::vector<ZlLdResult> out((size_t)nreq);
        int64_t walk[6];
        const int64_t used = zlld_call(nreq, reqs.data(), data.data(), length.data(), channels.data(), rate.data(), recs.data(), items, base.data(), out.data(), walk);
        assert(used == items);
        assert(walk[0] == expect && walk[1] == 0 && walk[2] == 0 && walk[3] == 0 && walk[5] == (items + ZL_LD_GROUP - 1) / ZL_LD_GROUP);
        for (int32_t i = 0; i < nreq; ++i) {
            const ZlLdResult &r = out[(size_t)i];
            assert(r.sub_blocks >= 1 && r.blocks >= 1 && r.above_relative <= r.above_absolute && r.above_absolute <= r.blocks);
            assert(r.peak[0] >= 0.0f && r.peak[0] <= 1.0f && (channels[(size_t)i] == 2 || r.peak[1] == 0.0f));
            assert(r.above_absolute == 0 ? (r.lufs < 0.0 && isinf(r.lufs)) : (r.lufs > -70.0 && r.lufs < 10.0));
        }
        total += walk[0];
    }
    printf("loudness check ok (%lld samples)\n", (long long)total);
    return 0;
}
