// Host build of the packed on-grid mix as restated in libzl_amd/csrc/zl_render.h (zl_mix_frame_ongrid_pk: the operation sequence of
// zl_mix_acc_ongrid_pk in zl_kernels.hip) beside the two forms that define it -- TEST HARNESS ONLY.
#include <cstdint>

#include "zl_render.h"

extern "C" {

// n frames: the packed sequence (pk_*), the one-tap definition (og_*), and the plain linear expression zl_mix_frame<0> with alpha = 0 whose
// second tap is the first and whose gains are 1 (two_*): its dropped term is then a zero of the tap's own sign, and l = x0l, r = x0r to the bit
void zlpk_mix(int n, const float *x0l, const float *x0r, const float *lpan, const float *rpan,
              float *pk_l, float *pk_r, float *og_l, float *og_r, float *two_l, float *two_r)
{
    for (int i = 0; i < n; ++i) {
        zl_mix_frame_ongrid_pk(x0l[i], x0r[i], lpan[i], rpan[i], pk_l[i], pk_r[i]);
        zl_mix_frame_ongrid(x0l[i], x0r[i], lpan[i], rpan[i], og_l[i], og_r[i]);
        ZlTaps t;
        t.x0l = t.x1l = x0l[i]; t.x0r = t.x1r = x0r[i];
        t.xml = t.xmr = t.x2l = t.x2r = 0.0f;
        zl_mix_frame<0>(t, 0.0f, true, true, true, 1.0f, 1.0f, 1.0f, 1.0f, lpan[i], rpan[i], two_l[i], two_r[i]);
    }
}

// the bus sum of F frames of V voices ([V][F] rows of samples, one pan pair per voice), in voice order from +0.0f: packed and defined
void zlpk_sum(int V, int F, const float *x0l, const float *x0r, const float *lpan, const float *rpan,
              float *pk_l, float *pk_r, float *og_l, float *og_r)
{
    for (int f = 0; f < F; ++f) { pk_l[f] = pk_r[f] = og_l[f] = og_r[f] = 0.0f; }
    for (int v = 0; v < V; ++v)
        for (int f = 0; f < F; ++f) {
            float l, r;
            zl_mix_frame_ongrid_pk(x0l[(size_t)v * F + f], x0r[(size_t)v * F + f], lpan[v], rpan[v], l, r);
            pk_l[f] += l; pk_r[f] += r;
            zl_mix_frame_ongrid(x0l[(size_t)v * F + f], x0r[(size_t)v * F + f], lpan[v], rpan[v], l, r);
            og_l[f] += l; og_r[f] += r;
        }
}

}
