// The clip edit's harness walk (tests/cpu_harness/edit_host.cpp over libzl_amd/csrc/zl_edit.h) in a stand-alone program, for a build
// with AddressSanitizer and UBSan (tests/test_edit_cpu.py builds and runs it): every buffer has exactly the size the call needs -- a
// sound holds length * channels floats and not one more, an extent the floats of the length the request ends with (worked out here by a
// plain loop over the frames), a weight table the frames it fades -- so a group's float that a mask should have kept out, a source float
// in front of the kept region or behind it, a weight outside its table or a write outside the extent ends the program.  The calls mix
// mono and stereo, forward and reversed, regions from frame 0 and up to the last frame, trims with silence of every length around the
// loud part, silent clips, fades from none to far too long.
//   edit_check <seed> <calls>        exit 0 and "edit check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/edit_host.cpp"

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    std::mt19937_64 rng(seed);
    const int32_t fades[] = {0, 0, 1, 2, 3, 64, 1025, 1000000};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 6);
        std::vector<zlhip_edit_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq), dsts((size_t)nreq), tin((size_t)nreq), tout((size_t)nreq);
        std::vector<std::vector<int32_t>> counts((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<float *> dst((size_t)nreq), w_in((size_t)nreq), w_out((size_t)nreq);
        std::vector<int32_t *> writes((size_t)nreq);
        std::vector<int64_t> floats((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq), first((size_t)nreq), count((size_t)nreq);
        std::vector<uint32_t> verdicts((size_t)nreq, 0u);
        int32_t expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t ch = 1 + (int32_t)(rng() & 1);
            const int32_t len = 1 + (int32_t)(rng() % (rng() % 4 == 0 ? 7000 : 600));
            zlhip_edit_request &q = reqs[(size_t)i];
            memset(&q, 0, sizeof q);
            q.first_frame = rng() % 3 == 0 ? 0 : (int32_t)(rng() % (uint64_t)len);
            q.num_frames = rng() % 3 == 0 ? 0 : 1 + (int32_t)(rng() % (uint64_t)(len - q.first_frame));
            q.flags = (int32_t)(rng() % 4);
            q.pre_roll_frames = (int32_t)(rng() % 3 == 0 ? rng() % 50 : 0); q.hold_frames = (int32_t)(rng() % 3 == 0 ? rng() % 50 : 0);
            q.fade_in_frames = fades[rng() % 8]; q.fade_out_frames = fades[rng() % 8]; q.curve = (int32_t)(rng() % 3);
            q.threshold = rng() % 2 ? 0.0f : 0.25f;
            length[(size_t)i] = len; channels[(size_t)i] = ch;
            std::vector<float> &v = sounds[(size_t)i];
            v.assign((size_t)len * (size_t)ch, 0.0f);
            const int content = (int)(rng() % 4);                  // silence, noise everywhere, noise in the middle, one loud sample
            const int64_t lo = content == 2 ? (int64_t)(rng() % (uint64_t)len) : 0, hi = content == 2 ? lo + (int64_t)(rng() % (uint64_t)(len - lo)) : len;
            if (content == 1 || content == 2) for (int64_t k = lo * ch; k < hi * ch; ++k) v[(size_t)k] = (float)((double)(rng() % 20001) - 10000.0) / 10000.0f;
            if (content == 3) v[(size_t)(rng() % v.size())] = -0.5f;
            data[(size_t)i] = v.data(); floats[(size_t)i] = (int64_t)v.size();
            // the length the request ends with, by a plain loop
            const int32_t a = q.first_frame, b = q.num_frames ? a + q.num_frames : len;
            const float thr = q.threshold == 0.0f ? 0.0009765625f : q.threshold;
            int32_t a2 = a, b2 = b;
            bool silent = false;
            if (q.flags & 1) {
                int32_t F = -1, Z = -1;
                for (int32_t f = a; f < b; ++f)
                    for (int32_t k = 0; k < ch; ++k) if (!(fabsf(v[(size_t)f * ch + k]) < thr)) { if (F < 0) F = f; Z = f; }
                silent = F < 0;
                if (!silent) { a2 = F - q.pre_roll_frames > a ? F - q.pre_roll_frames : a; b2 = Z + 1 + q.hold_frames < b ? Z + 1 + q.hold_frames : b; }
            }
            const int32_t n = b2 - a2, Xi = q.fade_in_frames < n / 2 ? q.fade_in_frames : n / 2, Xo = q.fade_out_frames < n / 2 ? q.fade_out_frames : n / 2;
            const bool applied = !silent && !(a2 == 0 && n == len && !(q.flags & 2) && Xi == 0 && Xo == 0);
            first[(size_t)i] = a2; count[(size_t)i] = applied ? n : 0;
            const int64_t ext = applied ? zled_extent_floats(n, ch) : 0;
            dsts[(size_t)i].assign((size_t)ext, -1.0f); counts[(size_t)i].assign((size_t)ext, 0);
            tin[(size_t)i].assign(applied ? (size_t)Xi : 0, -1.0f); tout[(size_t)i].assign(applied ? (size_t)Xo : 0, -1.0f);
            dst[(size_t)i] = dsts[(size_t)i].data(); writes[(size_t)i] = counts[(size_t)i].data();
            w_in[(size_t)i] = tin[(size_t)i].data(); w_out[(size_t)i] = tout[(size_t)i].data();
            expect += applied ? 1 : 0;
        }
        std::vector<zlhip_edit> out((size_t)nreq);
        int64_t walk[6];
        const int32_t applied = zled_call(nreq, reqs.data(), data.data(), floats.data(), length.data(), channels.data(), dst.data(), writes.data(), out.data(),
                                          w_in.data(), w_out.data(), verdicts.data(), walk);
        assert(applied == expect);
        assert(walk[3] == 0);
        for (int32_t i = 0; i < nreq; ++i) {
            const zlhip_edit &r = out[(size_t)i];
            assert((r.applied ? r.length : 0) == count[(size_t)i] && verdicts[(size_t)i] == 0u);
            if (!r.applied) continue;
            assert(r.first_frame == first[(size_t)i] && r.num_frames == r.length);
            for (int32_t n : counts[(size_t)i]) assert(n == 1);
            const int32_t ch = channels[(size_t)i], n = r.length, a2 = r.first_frame;
            const std::vector<float> &x = sounds[(size_t)i], &y = dsts[(size_t)i];
            for (int64_t k = 0; k < (int64_t)y.size(); ++k) {
                const int64_t f = k / ch;
                if (f >= n) { assert(y[(size_t)k] == 0.0f); continue; }
                const float src = x[(size_t)((r.reversed ? a2 + n - 1 - f : a2 + f) * ch + k % ch)];
                if (f >= r.fade_in_frames && f < n - r.fade_out_frames) assert(y[(size_t)k] == src);
                else assert(fabsf(y[(size_t)k]) <= fabsf(src));
            }
            if (r.fade_in_frames) assert(tin[(size_t)i][0] == 0.0f);
            if (r.fade_out_frames) assert(tout[(size_t)i][0] == 0.0f);
            total += walk[0];
        }
    }
    printf("edit check ok (%lld groups)\n", (long long)total);
    return 0;
}
