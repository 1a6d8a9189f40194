// The limiter's and the peak measurement's harness walk (tests/cpu_harness/limit_host.cpp over libzl_amd/csrc/zl_limit.h) in a
// stand-alone program, for a build with AddressSanitizer and UBSan (tests/test_limit_cpu.py builds and runs it): every buffer has exactly
// the size the call needs -- a sound holds the floats of its arena extent and not one more, an extent the same, the records the chunks
// of the call -- so a group beyond the extent, a record beyond the clip's chunks or a weight outside its window ends the program.  The
// calls mix mono and stereo, every look-ahead and hold, clips with no, one and many hot frames, gains, rates of every oversampling
// factor, with and without the true-peak flag; the output is checked against the ceiling and, out of reach of every hot frame, against
// the source.
//   limit_check <seed> <calls>        exit 0 and "limit check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/limit_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t looks[] = {0, 1, 2, 17, 240, 512}, holds[] = {0, 0, 1, 33, 512};
    const double rates[] = {44100.0, 48000.0, 96000.0, 192000.0};
    int64_t tiles = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 5);
        std::vector<zlhip_limit_request> reqs((size_t)nreq);
        std::vector<zlhip_peak_request> preqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq), dsts((size_t)nreq);
        std::vector<std::vector<int32_t>> counts((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<float *> dst((size_t)nreq);
        std::vector<int32_t *> writes((size_t)nreq);
        std::vector<int64_t> floats((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        std::vector<uint32_t> verdicts((size_t)nreq, 0u);
        int32_t nrec = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t ch = 1 + (int32_t)(rng() & 1);
            const int32_t len = 1 + (int32_t)(rng() % (rng() % 3 == 0 ? 4200 : 700));
            zlhip_limit_request &q = reqs[(size_t)i];
            memset(&q, 0, sizeof q);
            q.flags = (int32_t)(rng() & 1); q.lookahead_frames = looks[rng() % 6]; q.hold_frames = holds[rng() % 5];
            q.ceiling = rng() % 2 ? 0.0f : 0.5f; q.gain = rng() % 3 ? 0.0f : 1.5f;
            length[(size_t)i] = len; channels[(size_t)i] = ch; rate[(size_t)i] = rates[rng() % 4];
            std::vector<float> &v = sounds[(size_t)i];
            v.assign((size_t)zllm_extent_floats(len, ch), 7.0f);   // (what lies behind the data must not reach the output)
            const int content = (int)(rng() % 4);                  // quiet, one hot sample, a few, loud everywhere
            for (int64_t k = 0; k < (int64_t)len * ch; ++k) v[(size_t)k] = (float)((double)(rng() % 20001) - 10000.0) / 10000.0f * (content == 3 ? 1.0f : 0.3f);
            if (content == 1 || content == 2) for (int h = 0; h < (content == 1 ? 1 : 5); ++h) v[(size_t)(rng() % ((uint64_t)len * ch))] = rng() % 2 ? 0.99f : -1.4f;
            data[(size_t)i] = v.data(); floats[(size_t)i] = (int64_t)v.size();
            dsts[(size_t)i].assign(v.size(), -9.0f); counts[(size_t)i].assign(v.size(), 0);
            dst[(size_t)i] = dsts[(size_t)i].data(); writes[(size_t)i] = counts[(size_t)i].data();
            zlhip_peak_request &p = preqs[(size_t)i];
            p.id = 0; p.first_frame = (int32_t)(rng() % (uint64_t)len); p.num_frames = 1 + (int32_t)(rng() % (uint64_t)(len - p.first_frame)); p.flags = (int32_t)(rng() & 1);
            nrec += zl_lm_chunks(p.num_frames);
        }
        std::vector<zlhip_limit> out((size_t)nreq);
        int64_t walk[8];
        const int32_t applied = zllm_call(nreq, reqs.data(), data.data(), floats.data(), length.data(), channels.data(), rate.data(), dst.data(), writes.data(), out.data(),
                                          verdicts.data(), walk);
        assert(applied >= 0);
        assert(walk[3] == 0 && walk[5] == 0 && walk[7] == 0);
        tiles += walk[2];
        for (int32_t i = 0; i < nreq; ++i) {
            const zlhip_limit &r = out[(size_t)i];
            assert(verdicts[(size_t)i] == 0u);
            if (!r.applied) { for (int32_t n : counts[(size_t)i]) assert(n == 0); continue; }
            for (int32_t n : counts[(size_t)i]) assert(n == 1);
            const int32_t ch = channels[(size_t)i], n = length[(size_t)i], L = r.lookahead_frames, H = r.hold_frames;
            const std::vector<float> &x = sounds[(size_t)i], &y = dsts[(size_t)i];
            // frames in reach of a hot sample peak (with the flag more frames may be hot: the bit-identity is asked without it only)
            std::vector<char> reach((size_t)n, 0);
            for (int32_t f = 0; f < n; ++f) {
                bool hot = false;
                for (int32_t k = 0; k < ch; ++k) hot = hot || fabsf(x[(size_t)f * ch + k] * r.gain) > r.ceiling;
                if (hot) for (int32_t j = f - L < 0 ? 0 : f - L; j <= f + L + H && j < n; ++j) reach[(size_t)j] = 1;
            }
            for (int64_t k = 0; k < (int64_t)y.size(); ++k) {
                const int64_t f = k / ch;
                if (f >= n) { assert(y[(size_t)k] == 0.0f); continue; }
                assert(fabsf(y[(size_t)k]) <= r.ceiling);
                const float v = x[(size_t)k] * r.gain;
                if (!reach[(size_t)f] && r.oversampling == 1) assert(y[(size_t)k] == v);
                assert(fabsf(y[(size_t)k]) <= fabsf(v));
            }
        }
        std::vector<ZlLmRecord> rec((size_t)nrec);
        std::vector<int32_t> recw((size_t)nrec, 0);
        std::vector<zlhip_peak> pout((size_t)nreq);
        const int32_t wrote = zllm_peak_call(nreq, preqs.data(), data.data(), floats.data(), length.data(), channels.data(), rate.data(), pout.data(), rec.data(), recw.data(), walk);
        assert(wrote == nrec && walk[3] == 0);
        for (int32_t n : recw) assert(n == 1);
        for (int32_t i = 0; i < nreq; ++i) {
            const zlhip_peak_request &p = preqs[(size_t)i];
            float m[2] = {0.0f, 0.0f};
            for (int32_t f = p.first_frame; f < p.first_frame + p.num_frames; ++f)
                for (int32_t k = 0; k < channels[(size_t)i]; ++k) m[k] = fmaxf(m[k], fabsf(sounds[(size_t)i][(size_t)f * channels[(size_t)i] + k]));
            assert(pout[(size_t)i].sample_peak[0] == m[0] && pout[(size_t)i].sample_peak[1] == m[1]);
            assert(pout[(size_t)i].true_peak[0] >= m[0] && pout[(size_t)i].true_peak[1] >= m[1]);
        }
    }
    printf("limit check ok (%lld tiles)\n", (long long)tiles);
    return 0;
}
