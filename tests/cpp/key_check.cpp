// The key detection's host functions and harness walk (tests/cpu_harness/key_host.cpp over libzl_amd/csrc/zl_key.h) in a stand-alone
// program, for a build with AddressSanitizer and UBSan (tests/test_key_cpu.py builds and runs it): resolve, design, frames, finish
// and the relative-key shift on their edges, then the walk over random calls in which every buffer has exactly the size the call
// needs -- a sound holds length * channels floats and not one more, so a group's float that the mask should have kept out, a staged
// sample outside its chunk, a table index out of range or an overflowing signed product ends the program.
// The calls mix mono and stereo, odd first frames, one to twenty bins (partial bin groups), no, one, two, max_frames and spread
// frames, silence, quiet noise, full scale and tones.
//   key_check <seed> <calls>        exit 0 and "key check ok", or an abort
#undef NDEBUG
#include <assert.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../cpu_harness/key_host.cpp"

static void host_functions()
{
    // resolve: the defaults, the limits
    zlhip_key_request q = {0, 0, 1, 0, 0, 0.0f, 0, 0, 0, 0};
    assert(zl_ky_resolve(48000.0, &q.hop, &q.max_frames, &q.a4_hz, &q.note_lo, &q.note_hi, &q.q, &q.gate) == 0);
    assert(q.hop == 8192 && q.max_frames == 256 && q.a4_hz == 440.0f && q.note_lo == 36 && q.note_hi == 95 && q.q == 34 && q.gate == ZL_PT_GATE_DEFAULT);
    auto bad = [](double rate, zlhip_key_request r) { return zl_ky_resolve(rate, &r.hop, &r.max_frames, &r.a4_hz, &r.note_lo, &r.note_hi, &r.q, &r.gate) != 0; };
    zlhip_key_request r = q;
    r.note_hi = 36 + 96; assert(bad(48000.0, r));                  // 97 bins
    r = q; r.note_lo = 20; r.note_hi = 115; assert(!bad(48000.0, r));            // 96 bins
    r = q; r.a4_hz = NAN; assert(bad(48000.0, r));
    r = q; r.a4_hz = INFINITY; assert(bad(48000.0, r));
    r = q; r.max_frames = ZL_KY_MAX_FRAMES + 1; assert(bad(48000.0, r));
    r = q; assert(bad(NAN, r) && bad(0.0, r));
    r = q; r.note_hi = 81; assert(bad(1760.0, r) && !bad(1761.0, r));            // the top bin at rate / 2 (A5 = 880 Hz), and just under it
    // design: every bin's limits at the defaults and with every N clamped
    for (double rate : {8000.0, 48000.0, 192000.0}) {
        std::vector<ZlKyBin> bins(60);
        std::vector<int16_t> T(ZL_KY_TABLE);
        zl_ky_design(rate, 440.0f, 36, 95, rate > 100000.0 ? 256 : 34, bins.data(), T.data());
        for (size_t b = 0; b < bins.size(); ++b) {
            assert(bins[b].n % 2 == 0 && bins[b].n >= ZL_KY_SPAN_MIN && bins[b].n <= ZL_KY_SPAN_MAX && bins[b].step < 0x80000000u);
            assert((uint64_t)bins[b].wstep * (uint64_t)bins[b].n <= ((uint64_t)1 << 32) && (b == 0 || bins[b].n <= bins[b - 1].n));
        }
        assert(T[0] == 32767 && T[1024] == 0 && T[2048] == -32767 && T[3072] == 0);
    }
    // frames
    int32_t K, hop;
    zl_ky_frames(999, 1000, 100, 8, &K, &hop); assert(K == 0);
    zl_ky_frames(1000, 1000, 100, 8, &K, &hop); assert(K == 1 && hop == 100);
    zl_ky_frames(1099, 1000, 100, 8, &K, &hop); assert(K == 1);
    zl_ky_frames(1100, 1000, 100, 8, &K, &hop); assert(K == 2 && hop == 100);
    zl_ky_frames(5000, 1000, 100, 8, &K, &hop); assert(K == 8 && hop == 4000 / 7 && 7 * hop + 1000 <= 5000);
    zl_ky_frames(5000, 1000, 100, 1, &K, &hop); assert(K == 1 && hop == 100);
    // finish: a chroma that IS a profile gives its key with r = 1; a flat or an empty one gives none
    for (int i = 0; i < 24; ++i) {
        uint64_t c[12];
        const double *prof = i < 12 ? kZlKyMajor : kZlKyMinor;
        for (int p = 0; p < 12; ++p) c[p] = (uint64_t)(prof[(p - i % 12 + 12) % 12] * 1e12);
        ZlKyResult o;
        zlky_finish(c, 4, 4, &o);
        assert(o.tonic == i % 12 && o.mode == i / 12 && o.confidence > 0.999999 && o.second_confidence < o.confidence && o.sounding == 4);
    }
    uint64_t flat[12];
    for (int p = 0; p < 12; ++p) flat[p] = (uint64_t)1 << 61;
    ZlKyResult o;
    zlky_finish(flat, 4, 4, &o);
    assert(o.tonic == -1 && o.mode == 0 && o.confidence == 0.0 && o.frames == 4 && o.sounding == 0 && o.chroma[3] == 0);
    flat[5] += (uint64_t)1 << 60;
    zlky_finish(flat, 4, 0, &o); assert(o.tonic == -1);
    zlky_finish(flat, 0, 0, &o); assert(o.tonic == -1 && o.frames == 0);
    zlky_finish(flat, 4, 4, &o); assert(o.tonic >= 0);
    // the shift
    for (int a = 0; a < 24; ++a) for (int b = 0; b < 24; ++b) {
        const int32_t s = zl_ky_match_shift(a % 12, a / 12, b % 12, b / 12);
        assert(s >= -6 && s <= 5);
        const int from = a / 12 == b / 12 ? a % 12 : (a % 12 + (a / 12 == 0 ? 9 : 3)) % 12;
        assert(((from + s) % 12 + 12) % 12 == b % 12);
    }
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int calls = argc > 2 ? atoi(argv[2]) : 4;
    host_functions();
    std::mt19937_64 rng(seed);
    const int32_t firsts[] = {0, 1, 3, 5};
    int64_t total = 0;
    for (int c = 0; c < calls; ++c) {
        const int32_t nreq = 1 + (int32_t)(rng() % 4);
        std::vector<zlhip_key_request> reqs((size_t)nreq);
        std::vector<std::vector<float>> sounds((size_t)nreq);
        std::vector<const float *> data((size_t)nreq);
        std::vector<int32_t> length((size_t)nreq), channels((size_t)nreq), wantK((size_t)nreq);
        std::vector<double> rate((size_t)nreq);
        int64_t pairs = 0, nf = 0, nb = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t ch = 1 + (int32_t)(rng() & 1), first = firsts[rng() % 4], mf = 1 + (int32_t)(rng() % 4);
            rate[(size_t)i] = (rng() & 1) ? 8000.0 : 11025.0;
            zlhip_key_request &q = reqs[(size_t)i];
            q.id = 0; q.first_frame = first; q.num_frames = 1; q.hop = 64 + (int32_t)(rng() % 900); q.max_frames = mf; q.a4_hz = 0.0f;
            q.note_lo = 48 + (int32_t)(rng() % 24); q.note_hi = q.note_lo + (int32_t)(rng() % 20); q.q = 8 + (int32_t)(rng() % 26); q.gate = 8;
            zlhip_key_request t = q;
            assert(zl_ky_resolve(rate[(size_t)i], &t.hop, &t.max_frames, &t.a4_hz, &t.note_lo, &t.note_hi, &t.q, &t.gate) == 0);
            std::vector<ZlKyBin> bins((size_t)(q.note_hi - q.note_lo + 1));
            zl_ky_design(rate[(size_t)i], t.a4_hz, t.note_lo, t.note_hi, t.q, bins.data(), nullptr);
            const int32_t L = bins[0].n;
            const int kind = (int)(rng() % 5);                     // the frames wanted: none, 1, 2, mf, or more than mf (the spread hop)
            const int32_t want = kind == 0 ? 0 : (kind == 1 ? 1 : (kind == 2 ? 2 : (kind == 3 ? mf : mf + 2)));
            q.num_frames = want == 0 ? L - 1 - (int32_t)(rng() % 7) : L + (want - 1) * q.hop + (int32_t)(rng() % q.hop);
            wantK[(size_t)i] = want > mf ? mf : want;
            length[(size_t)i] = first + q.num_frames + (int32_t)(rng() % 3);
            channels[(size_t)i] = ch;
            std::vector<float> &s = sounds[(size_t)i];
            s.resize((size_t)length[(size_t)i] * (size_t)ch);
            const int content = (int)(rng() % 4);                  // silence, quiet noise, full scale, a tone
            const double period = 9.0 + (double)(rng() % 60);
            for (size_t k = 0; k < s.size(); ++k) {
                float v = 0.0f;
                if (content == 1) v = (float)((double)(rng() % 2001) - 1000.0) / 4096000.0f * 40.0f;
                if (content == 2) v = (rng() & 1) ? 9.0f : -9.0f;
                if (content == 3) v = 0.4f * (float)sin(6.283185307179586 * (double)(k / (size_t)ch) / period);
                s[k] = v;
            }
            data[(size_t)i] = s.data();
            pairs += (int64_t)wantK[(size_t)i] * (int64_t)bins.size(); nf += wantK[(size_t)i]; nb += (int64_t)bins.size();
        }
        std::vector<ZlKyAcc> acc((size_t)pairs);
        std::vector<uint64_t> totals((size_t)nb);
        std::vector<ZlKyBin> bins((size_t)nb);
        std::vector<int32_t> silent((size_t)nf), geom((size_t)nreq * 8);
        std::vector<int64_t> base((size_t)nreq);
        std::vector<ZlKyResult> out((size_t)nreq);
        int64_t walk[4];
        const int64_t used = zlky_call(nreq, reqs.data(), data.data(), length.data(), channels.data(), rate.data(), acc.data(), pairs, totals.data(), bins.data(), nb,
                                       silent.data(), nf, geom.data(), base.data(), out.data(), walk);
        assert(used == pairs);
        int64_t expect = 0;
        for (int32_t i = 0; i < nreq; ++i) {
            const int32_t *g = &geom[(size_t)i * 8];
            assert(g[1] == wantK[(size_t)i] && out[(size_t)i].frames == g[1]);
            if (g[1] > 0) assert((int64_t)reqs[(size_t)i].first_frame + (int64_t)(g[1] - 1) * g[2] + g[0] <= (int64_t)reqs[(size_t)i].first_frame + reqs[(size_t)i].num_frames);
            for (int32_t k = 0; k < g[1]; ++k)
                if (!silent[(size_t)(g[5] + k)]) for (int32_t b = 0; b < g[3]; ++b) expect += bins[(size_t)(g[6] + b)].n;
            const ZlKyResult &r = out[(size_t)i];
            assert(r.tonic >= -1 && r.tonic <= 11 && r.sounding <= r.frames && (r.tonic < 0 || (r.confidence >= r.second_confidence && r.confidence <= 1.0000001)));
        }
        assert(walk[0] == expect && walk[1] == 0 && walk[2] == 0 && walk[3] == 0);
        total += walk[0];
    }
    printf("key check ok (%lld terms)\n", (long long)total);
    return 0;
}
