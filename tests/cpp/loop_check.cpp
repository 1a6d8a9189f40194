// The loop finder's harness walk (tests/cpu_harness/loop_host.cpp over libzl_amd/csrc/zl_loop.h) in a stand-alone program, for a build
// with AddressSanitizer and UBSan (tests/test_loop_cpu.py builds and runs it): every buffer has exactly the size the call needs -- a
// sound holds length * channels floats and not one more, so a group's float that the mask should have kept out, a strip sample, a
// staged element, a cost, an item or a record outside its array, a shift out of range or an overflowing signed product ends the program.
// The calls mix mono and stereo, odd nominal points, candidate counts around the tile's 64, every window class, ranges clipped at the
// data's edges, overlapping ranges, empty ranges, a kept point, silence, quiet noise, full scale and tones, in both forms.
//   loop_check <seed> <calls>        exit 0 and "loop check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/loop_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t radii[] = {-1, 1, 31, 32, 33, 64, 70};
    const int32_t windows[] = {16, 32, 256, 1024};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 4);
        std::vector<zlhip_loop_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        int64_t words = 0, nitems = 0, expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t W = windows[rng() % 4], H = W / 2, ch = 1 + (int32_t)(rng() & 1);
            const int32_t rs = radii[rng() % 7], re = radii[rng() % 7];
            rate[(size_t)i] = (rng() & 1) ? 48000.0 : 44100.0;
            const int kind = (int)(rng() % 5);                     // inside, clipped at the front, clipped at the back, overlapping, too short for a window
            int32_t len = 2 * W + 400 + (int32_t)(rng() % 7), s0, e0;
            if (kind == 0) { s0 = H + 75 + (int32_t)(rng() % 5); e0 = len - H - 75 - (int32_t)(rng() % 5); }
            else if (kind == 1) { s0 = (int32_t)(rng() % 3); e0 = len - H - 71; }
            else if (kind == 2) { s0 = H + 71; e0 = len - (int32_t)(rng() % 3); }
            else if (kind == 3) { s0 = len / 2 - 5; e0 = len / 2 + 6; }
            else { len = W - 1 - (int32_t)(rng() % 3); s0 = 0; e0 = len; }
            zlhip_loop_request &q = reqs[(size_t)i];
            q.id = 0; q.start_frame = s0; q.stop_frame = e0; q.start_search = rs; q.stop_search = re; q.window = W;
            q.min_length = (rng() & 1) ? 0 : 1 + (int32_t)(rng() % 40);
            length[(size_t)i] = len; channels[(size_t)i] = ch;
            std::vector<float> &s = sounds[(size_t)i];
            s.resize((size_t)len * (size_t)ch);
            const int content = (int)(rng() % 4);                  // silence, quiet noise, full scale, a tone
            const double period = 9.0 + (double)(rng() % 90);
            for (size_t k = 0; k < s.size(); ++k) {
                float v = 0.0f;
                if (content == 1) v = (float)((double)(rng() % 2001) - 1000.0) / 4096000.0f * 40.0f;
                if (content == 2) v = (rng() & 1) ? 9.0f : -9.0f;
                if (content == 3) v = 0.4f * (float)sin(6.283185307179586 * (double)(k / (size_t)ch) / period);
                s[k] = v;
            }
            data[(size_t)i] = s.data();
            ZlLpRequest R;
            assert(geometry(q, rate[(size_t)i], ch, len, s.data(), &R) == 0);
            if (kind == 4) assert(R.ns == 0 && R.ne == 0);
            if (kind == 0) assert(R.ns == (rs < 0 ? 1 : 2 * rs + 1) && R.ne == (re < 0 ? 1 : 2 * re + 1));
            words += (int64_t)R.ns * R.ne; nitems += zl_lp_items(R);
            expect += (int64_t)R.ns * R.ne * W;
        }
        std::vector<uint32_t> costs((size_t)words);
        std::vector<ZlLpItem> items((size_t)nitems);
        std::vector<int32_t> geom((size_t)nreq * 8);
        std::vector<int64_t> cbase((size_t)nreq);
        std::vector<ZlLpResult> out((size_t)nreq);
        int64_t walk[4];
        const int64_t used = zllp_call(nreq, reqs.data(), data.data(), length.data(), channels.data(), rate.data(), costs.data(), words, items.data(), nitems, geom.data(),
                                       cbase.data(), out.data(), nullptr, walk, (c & 1) ? kFormDot : kFormDiff);
        assert(used == words);
        assert(walk[0] == expect && walk[1] == 0 && walk[2] == 0 && walk[3] == 0);
        for (int32_t i = 0; i < nreq; ++i) {
            const ZlLpResult &r = out[(size_t)i];
            const int32_t *g = &geom[(size_t)i * 8];
            assert(r.shift >= 0 && r.shift <= 6);
            if (!r.found) { assert(r.pairs == 0 && r.starts == 0 && r.cost == 0); continue; }
            assert(r.starts == g[1] && r.ends == g[3] && r.pairs >= 1 && r.pairs <= (uint64_t)g[1] * (uint64_t)g[3]);
            assert(r.start_frame >= g[0] && r.start_frame < g[0] + g[1] && r.stop_frame >= g[2] && r.stop_frame < g[2] + g[3]);
            assert(r.stop_frame - r.start_frame >= g[5] && r.seam_db >= -120.0 && r.seam_db <= 10.0);
            assert(costs[(size_t)(cbase[(size_t)i] + (int64_t)(r.start_frame - g[0]) * g[3] + (r.stop_frame - g[2]))] == r.cost);
        }
        // the seconds of what was found
        for (int32_t i = 0; i < nreq; ++i) {
            if (!out[(size_t)i].found) continue;
            float a, l;
            assert(zllp_seconds(rate[(size_t)i], out[(size_t)i].start_frame, out[(size_t)i].stop_frame, &a, &l) == 0);
            assert(zllp_frame_of(a, rate[(size_t)i]) == out[(size_t)i].start_frame && zllp_stop_of(a, l, rate[(size_t)i]) == out[(size_t)i].stop_frame);
        }
        total += walk[0];
    }
    printf("loop check ok (%lld terms)\n", (long long)total);
    return 0;
}
