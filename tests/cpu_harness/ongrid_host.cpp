// Host build of K2's on-grid form (libzl_amd/csrc/zl_render.h: zl_voice_ongrid, zl_mix_frame_ongrid, zl_all_finite) for the CPU
// tier -- TEST HARNESS ONLY.  The two-tap side is zl_mix_frame<0> with alpha = 0, as zl_k2_simple_mix calls it.
#include <cstdint>
#include <cstring>

#include "zl_render.h"

extern "C" {

// n frames of one voice each: the plain linear form with alpha 0 (full_*) and the one-tap form (short_*).  stereo = 0: a mono
// source, as zl_k2_chunk_simple_mono feeds it (x0r = x1r = 0, r = l) against the one-tap form with x0r = x0l.
void zlog_mix(int n, int stereo, const float *x0l, const float *x0r, const float *x1l, const float *x1r,
              const float *lgain, const float *rgain, const float *env, const float *vol, const float *lpan, const float *rpan,
              float *full_l, float *full_r, float *short_l, float *short_r)
{
    for (int i = 0; i < n; ++i) {
        ZlTaps t;
        t.x0l = x0l[i]; t.x1l = x1l[i];
        t.x0r = stereo ? x0r[i] : 0.0f; t.x1r = stereo ? x1r[i] : 0.0f;
        t.xml = t.xmr = t.x2l = t.x2r = 0.0f;
        zl_mix_frame<0>(t, 0.0f, true, true, stereo != 0, lgain[i], rgain[i], env[i], vol[i], lpan[i], rpan[i], full_l[i], full_r[i]);
        zl_mix_frame_ongrid(x0l[i], stereo ? x0r[i] : x0l[i], lpan[i], rpan[i], short_l[i], short_r[i]);
    }
}

// K2's bus sum and report peak of F frames of V voices ([V][F] rows): the ordered sum from +0.0f in voice order, and per voice
// the maximum over the frames of (ng > 0 ? ng : 0), ng = l + r (zl_k2_simple_mix)
void zlog_sum_peak(int V, int F, const float *l, const float *r, float *acc_l, float *acc_r, float *peak)
{
    for (int f = 0; f < F; ++f) { acc_l[f] = 0.0f; acc_r[f] = 0.0f; }
    for (int v = 0; v < V; ++v) {
        float pk = 0.0f;
        for (int f = 0; f < F; ++f) {
            const float lo = l[(size_t)v * F + f], ro = r[(size_t)v * F + f];
            acc_l[f] += lo; acc_r[f] += ro;
            const float ng = lo + ro;
            const float p = ng > 0.0f ? ng : 0.0f;
            pk = p > pk ? p : pk;
        }
        peak[v] = pk;
    }
}

int zlog_predicate(unsigned mode, int enabled, int simple, int unit, int interior, double P0, double step, int sound_flags)
{
    return zl_voice_ongrid(mode, enabled, simple != 0, unit != 0, interior != 0, P0, step, sound_flags) ? 1 : 0;
}

int zlog_all_finite(const float *x, long long n) { return zl_all_finite(x, (size_t)n) ? 1 : 0; }

int zlog_sound_finite_flag(void) { return ZL_SOUND_FINITE; }

}
