// stretch_host.cpp -- TEST HARNESS (not part of the product library).
//
// Host build of the clip re-render (libzl_amd/csrc/zl_stretch.h): the same scalar text the HIP kernels of zl_stretch.hip run --
// geometry, quantisation, weighted reference, score, argmax order, cross-fade, resampler, gain -- driven by plain loops.  The CPU tier
// compares it with the numpy restatement (tests/stretch_ref.py) bit for bit; scripts/rerender_bench.py times it on host threads
// next to the device.  libzl_amd never loads this library.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "zl_stretch.h"

namespace {

struct HostIn {
    const float *src; int64_t len; int ch;     // interleaved
    float operator()(int64_t n, int c) const { return n < len ? src[n * ch + c] : 0.0f; }
};

void seek(const ZlStretchGeom &g, const HostIn &in, int32_t *off)
{
    if (g.nseg < 1) return;
    const int ch = in.ch, O = g.O, W = g.W, L = g.S - g.O;
    std::vector<int32_t> q((size_t)ch * (W + O)), ref((size_t)ch * O);
    off[0] = 0;
    int64_t prev = 0;
    for (int32_t k = 1; k < g.nseg; ++k) {
        const int64_t base = zl_st_base(g, k);
        for (int c = 0; c < ch; ++c) {
            for (int i = 0; i < O; ++i) ref[(size_t)c * O + i] = zl_st_ref(zl_st_q(in(prev + L + i, c)), i, O);
            for (int j = 0; j < W + O; ++j) q[(size_t)c * (W + O) + j] = zl_st_q(in(base + j, c));
        }
        double bs = -INFINITY; int32_t bo = INT_MAX;
        for (int o = 0; o < W; ++o) {
            int64_t corr = 0, norm = 0;
            for (int c = 0; c < ch; ++c) {
                const int32_t *x = &q[(size_t)c * (W + O) + o], *r = &ref[(size_t)c * O];
                for (int i = 0; i < O; ++i) { corr += (int64_t)r[i] * x[i]; norm += (int64_t)x[i] * x[i]; }
            }
            const double s = zl_st_score(corr, norm);
            if (zl_st_better(s, o, bs, bo)) { bs = s; bo = o; }
        }
        off[k] = bo;
        prev = base + bo;
    }
}

// interleaved source -> interleaved output [N][ch]; offsets [nseg]
void render(const ZlStretchGeom &g, const float *src, int ch, float *out, int32_t *off)
{
    const HostIn in{src, g.len, ch};
    if (g.stretch) seek(g, in, off);
    for (int64_t j = 0; j < g.N; ++j)
        for (int c = 0; c < ch; ++c) out[j * ch + c] = zl_st_y(g, off, j, c, in);
}

std::vector<float> interleave(const float *L, const float *R, int64_t len)
{
    std::vector<float> v((size_t)len * (R ? 2 : 1));
    for (int64_t i = 0; i < len; ++i) {
        if (R) { v[2 * (size_t)i] = L[i]; v[2 * (size_t)i + 1] = R[i]; } else v[(size_t)i] = L[i];
    }
    return v;
}

}  // namespace

extern "C" {

// geometry of a render: returns 0, or -1 for parameters the engine rejects.  out: N, N1, nseg, O, S, W, stretch, resample, gain
int zlst_geometry(double sr, int64_t len, float gain_db, float pitch, float speed, int64_t *out)
{
    ZlStretchGeom g;
    if (zl_st_geometry(sr, len, gain_db, pitch, speed, &g) != 0) return -1;
    const int64_t v[9] = { g.N, g.N1, g.nseg, g.O, g.S, g.W, g.stretch, g.resample, g.gain };
    std::memcpy(out, v, sizeof v);
    return 0;
}

// one clip, planar in and out (R / outR NULL for mono); outL / outR hold N frames, offsets nseg values (zlst_geometry).
// Identity parameters copy the source, as the engine plays the original.
int zlst_render(const float *L, const float *R, int64_t len, double sr, float gain_db, float pitch, float speed,
                float *outL, float *outR, int32_t *offsets)
{
    ZlStretchGeom g;
    if (zl_st_geometry(sr, len, gain_db, pitch, speed, &g) != 0) return -1;
    const int ch = R ? 2 : 1;
    if (zl_st_identity(gain_db, pitch, speed)) {
        std::memcpy(outL, L, (size_t)len * sizeof(float));
        if (R) std::memcpy(outR, R, (size_t)len * sizeof(float));
        return 0;
    }
    const std::vector<float> src = interleave(L, R, len);
    std::vector<float> out((size_t)g.N * ch);
    std::vector<int32_t> off((size_t)g.nseg + 1);
    render(g, src.data(), ch, out.data(), off.data());
    for (int64_t j = 0; j < g.N; ++j) {
        outL[j] = out[(size_t)j * ch];
        if (R) outR[j] = out[(size_t)j * ch + 1];
    }
    if (offsets && g.nseg > 0) std::memcpy(offsets, off.data(), (size_t)g.nseg * sizeof(int32_t));
    return 0;
}

// a batch of clips of one shape (interleaved sources [count][len*ch], outputs [count][N*ch]) on `threads` host threads, the clips
// dealt out round robin: the host side of scripts/rerender_bench.py
int zlst_render_batch(const float *src, int32_t count, int ch, int64_t len, double sr, float gain_db, float pitch, float speed,
                      float *out, int threads)
{
    ZlStretchGeom g;
    if (zl_st_geometry(sr, len, gain_db, pitch, speed, &g) != 0 || threads < 1) return -1;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        pool.emplace_back([&, t]() {
            std::vector<int32_t> off((size_t)g.nseg + 1);
            for (int32_t i = t; i < count; i += threads)
                render(g, src + (size_t)i * len * ch, ch, out + (size_t)i * g.N * ch, off.data());
        });
    }
    for (auto &th : pool) th.join();
    return 0;
}

}  // extern "C"
