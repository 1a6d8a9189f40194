// The loop crossfade's harness walk (tests/cpu_harness/xfade_host.cpp over libzl_amd/csrc/zl_xfade.h) in a stand-alone program, for a
// build with AddressSanitizer and UBSan (tests/test_xfade_cpu.py builds and runs it): every buffer has exactly the size the call needs --
// a sound holds length * channels floats and not one more, an extent its floats, a weight table 2 X floats -- so a group's float that a
// mask should have kept out, a float of B below the clip's first, a weight outside its table, a write outside the extent or an
// overflowing signed product ends the program.  The calls mix mono and stereo, fades from 1 frame to several chunks, loops that end at
// the last frame, fades that begin at frame 0, adjoining regions, requests with nothing to fade, silence, full scale and noise.
//   xfade_check <seed> <calls>        exit 0 and "xfade check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/xfade_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t fades[] = {1, 2, 3, 5, 8, 64, 257, 960, 1024, 1025, 2500};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 6);
        std::vector<zlhip_xfade_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq), dsts((size_t)nreq), tables((size_t)nreq);
        std::vector<std::vector<int32_t>> counts((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<float *> dst((size_t)nreq), weights((size_t)nreq);
        std::vector<int32_t *> writes((size_t)nreq);
        std::vector<int64_t> floats((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq);
        std::vector<double> rate((size_t)nreq, 48000.0);
        std::vector<uint32_t> verdicts((size_t)nreq, 0u);
        int32_t expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t ch = 1 + (int32_t)(rng() & 1), X = fades[rng() % 11];
            const int kind = (int)(rng() % 5);                     // inside, B from frame 0, A to the last frame, adjoining, nothing to fade
            int32_t s = X + 1 + (int32_t)(rng() % 9), e = s + X + 1 + (int32_t)(rng() % 700), len = e + 1 + (int32_t)(rng() % 9);
            if (kind == 1) { e -= s - X; len -= s - X; s = X; }
            if (kind == 2) len = e;
            if (kind == 3) { s = X; e = 2 * X; len = e + (int32_t)(rng() % 3); }
            zlhip_xfade_request &q = reqs[(size_t)i];
            q.id = 0; q.start_frame = kind == 4 ? 0 : s; q.stop_frame = e; q.fade_frames = kind == 4 ? 0 : X; q.curve = (int32_t)(rng() % 3);
            length[(size_t)i] = len; channels[(size_t)i] = ch;
            std::vector<float> &v = sounds[(size_t)i];
            v.resize((size_t)len * (size_t)ch);
            const int content = (int)(rng() % 3);                  // silence, full scale, noise
            for (size_t k = 0; k < v.size(); ++k)
                v[k] = content == 0 ? 0.0f : content == 1 ? ((rng() & 1) ? 9.0f : -9.0f) : (float)((double)(rng() % 20001) - 10000.0) / 10000.0f;
            data[(size_t)i] = v.data(); floats[(size_t)i] = (int64_t)v.size();
            const int64_t ext = zlxf_extent_floats(len, ch);
            dsts[(size_t)i].assign((size_t)ext, -1.0f); counts[(size_t)i].assign((size_t)ext, 0);
            tables[(size_t)i].assign(kind == 4 ? 1 : (size_t)X * 2, -1.0f);
            dst[(size_t)i] = dsts[(size_t)i].data(); writes[(size_t)i] = counts[(size_t)i].data(); weights[(size_t)i] = kind == 4 ? nullptr : tables[(size_t)i].data();
            expect += kind == 4 ? 0 : 1;
        }
        std::vector<zlhip_xfade> out((size_t)nreq);
        int64_t walk[4];
        const int32_t applied = zlxf_call(nreq, reqs.data(), data.data(), floats.data(), length.data(), channels.data(), rate.data(), dst.data(), writes.data(), out.data(),
                                          weights.data(), verdicts.data(), walk);
        assert(applied == expect);
        assert(walk[3] == 0);
        for (int32_t i = 0; i < nreq; ++i) {
            const zlhip_xfade &r = out[(size_t)i];
            if (!r.applied) { assert(reqs[(size_t)i].start_frame == 0 && r.fade_frames == 0 && r.saa == 0 && counts[(size_t)i][0] == 0); continue; }
            assert(r.fade_frames == reqs[(size_t)i].fade_frames && r.rho >= 0.0 && r.rho <= 1.0 && r.correlation >= -1.0000001 && r.correlation <= 1.0000001);
            assert(r.saa >= 0 && r.sbb >= 0 && verdicts[(size_t)i] == 0u);
            for (int32_t n : counts[(size_t)i]) assert(n == 1);
            const int32_t ch = channels[(size_t)i], len = length[(size_t)i], e = r.stop_frame, s = r.start_frame, X = r.fade_frames;
            const std::vector<float> &x = sounds[(size_t)i], &y = dsts[(size_t)i];
            for (int64_t k = 0; k < (int64_t)y.size(); ++k) {
                const int64_t f = k / ch;
                if (f >= len) assert(y[(size_t)k] == 0.0f);
                else if (f < e - X || f >= e) assert(y[(size_t)k] == x[(size_t)k]);
            }
            for (int c2 = 0; c2 < ch; ++c2) assert(y[(size_t)(e - 1) * ch + c2] == x[(size_t)(s - 1) * ch + c2]);       // the last frame of the loop is the frame in front of its start
            assert(tables[(size_t)i][(size_t)X * 2 - 2] == 0.0f && tables[(size_t)i][(size_t)X * 2 - 1] == 1.0f);
            total += walk[0];
        }
    }
    printf("xfade check ok (%lld groups)\n", (long long)total);
    return 0;
}
