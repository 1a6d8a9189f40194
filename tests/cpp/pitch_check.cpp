// The pitch detection's harness walk (tests/cpu_harness/pitch_host.cpp over libzl_amd/csrc/zl_pitch.h) in a stand-alone program, for a
// build with AddressSanitizer and UBSan (tests/test_pitch_cpu.py builds and runs it): every buffer has exactly the size the call
// needs -- a sound holds length * channels floats and not one more, so a group's float that the mask should have kept out, a staged
// sample, a lag or a record outside its array, a shift out of range or an overflowing signed product ends the program.
// The calls mix mono and stereo, odd first frames, lag-tile edges, no, one, two, max_frames and stretched frames, silence, quiet noise,
// full scale and tones.
//   pitch_check <seed> <calls>        exit 0 and "pitch check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/pitch_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t tmaxes[] = {40, 254, 255, 256, 300, 511};
    const int32_t firsts[] = {0, 1, 3, 5};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 5);
        std::vector<zlhip_pitch_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        int64_t words = 0, nf = 0, expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t tmax = tmaxes[rng() % 6], ch = 1 + (int32_t)(rng() & 1), first = firsts[rng() % 4], mf = 1 + (int32_t)(rng() % 4);
            rate[(size_t)i] = (rng() & 1) ? 48000.0 : 44100.0;
            int32_t window = (tmax + 1 + 63) / 64 * 64;
            if (window < 256) window = 256;
            if (rng() & 1) window += 64;
            const int32_t L = window + tmax + 1;
            // the frames wanted: none, 1, 2, mf, or more than mf (the stretched hop)
            const int kind = (int)(rng() % 5);
            const int32_t want = kind == 0 ? 0 : (kind == 1 ? 1 : (kind == 2 ? 2 : (kind == 3 ? mf : mf + 2)));
            const int32_t n = want == 0 ? L - 1 - (int32_t)(rng() % 7) : L + (want - 1) * window + (int32_t)(rng() % window);
            zlhip_pitch_request &q = reqs[(size_t)i];
            q.id = 0; q.first_frame = first; q.num_frames = n; q.window = window; q.max_frames = mf;
            q.f_min = (float)(rate[(size_t)i] / ((double)tmax + 0.5)); q.f_max = (float)(rate[(size_t)i] / 8.5);
            q.threshold = (rng() & 1) ? 154 : 1024; q.gate = 8;
            length[(size_t)i] = first + n + (int32_t)(rng() % 3);
            channels[(size_t)i] = ch;
            std::vector<float> &s = sounds[(size_t)i];
            s.resize((size_t)length[(size_t)i] * (size_t)ch);
            const int content = (int)(rng() % 4);                  // silence, quiet noise, full scale, a tone
            const double period = 9.0 + (double)(rng() % (uint64_t)tmax);
            for (size_t k = 0; k < s.size(); ++k) {
                float v = 0.0f;
                if (content == 1) v = (float)((double)(rng() % 2001) - 1000.0) / 4096000.0f * 40.0f;
                if (content == 2) v = (rng() & 1) ? 9.0f : -9.0f;
                if (content == 3) v = 0.4f * (float)sin(6.283185307179586 * (double)(k / (size_t)ch) / period);
                s[k] = v;
            }
            data[(size_t)i] = s.data();
            ZlPtRequest R;
            assert(geometry(q, rate[(size_t)i], ch, s.data(), &R) == 0);
            assert(R.tmax == tmax && R.frames == (want > mf ? mf : want));
            words += (int64_t)R.frames * (tmax + 1); nf += R.frames;
            expect += (int64_t)R.frames * (tmax + 1) * window;
            if (R.frames > 0) assert(zl_pt_frame_start(R, R.frames - 1) + L <= (int64_t)first + n);
        }
        std::vector<uint64_t> D((size_t)words);
        std::vector<ZlPtFrame> frames((size_t)nf);
        std::vector<int32_t> geom((size_t)nreq * 8);
        std::vector<int64_t> dbase((size_t)nreq);
        std::vector<ZlPtResult> out((size_t)nreq);
        int64_t walk[4];
        const int64_t used = zlpt_call(nreq, reqs.data(), data.data(), length.data(), channels.data(), rate.data(), D.data(), words, frames.data(), nf, geom.data(),
                                       dbase.data(), out.data(), nullptr, nullptr, walk);
        assert(used == words);
        assert(walk[0] == expect && walk[1] == 0 && walk[2] == 0 && walk[3] == 0);
        for (int32_t i = 0; i < nreq; ++i) {
            const ZlPtResult &r = out[(size_t)i];
            assert(r.frames == geom[(size_t)i * 8 + 3] && r.shift >= 0 && r.shift <= 4);
            assert(r.lag == 0 || (r.lag >= geom[(size_t)i * 8] && r.lag <= geom[(size_t)i * 8 + 1] && r.hz > 0.0f && r.consistent >= 1 && r.consistent <= r.voiced));
        }
        total += walk[0];
    }
    printf("pitch check ok (%lld terms)\n", (long long)total);
    return 0;
}
