// Host build of the pair kernels' on-grid form for blocks with one loop restart (libzl_amd/csrc/zl_render.h: zl_voice_ongrid2,
// zl_ongrid2_lane) for the CPU tier -- TEST HARNESS ONLY.  The lane selection is the function the kernel calls; what a lane does with it
// (zl_k2_chunk_ongrid_pair_wrap, zl_kernels.hip) is restated here and held against the definition, zl_eval_control + zl_mix_frame<0>.
// The planner comes with plan_host.cpp, included whole: this library IS a planner harness with three more functions, and the test makes its
// ZlSim with this library's zlsim_create, so zlwrap_scan reads an object of its own build.
// -DZL_PAIR_WRAP_MAIN: a program of its own (for the sanitizers) that runs the truth table and the selection over buffers of the exact size.
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "plan_host.cpp"

static bool same_or_both_zero(float a, float b)
{
    return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b) || (a == 0.0f && b == 0.0f) || (a != a && b != b);
}

extern "C" {

int zlwrap_predicate(unsigned mode, int ongrid, int sound_flags, int cls, int n_active, int plan_flags, int gains_finite, int nseg, int n1, int N,
                     double step, double step1, double P0, double P1, int sample_duration)
{
    return zl_voice_ongrid2(mode, ongrid, sound_flags, cls, n_active, plan_flags, gains_finite != 0, nseg, n1, N, step, step1, P0, P1, sample_duration) ? 1 : 0;
}

// One voice-block of N frames, every lane of the pair kernels: src = the voice's source, length frames (+ the 8 frames of padding the arena
// keeps behind a source), interleaved stereo or mono.  n1 = INT_MAX: a single-segment on-grid voice of the same chunk (P1 is not read).
// Returns the number of frames that differ from the definition in more than the sign of a zero; lohi = the lowest and the highest source
// frame any lane read, the halves it does not use included.
int zlwrap_block(int stereo, int length, const float *src, int P0, int P1, int n1, int N, float lgain, float rgain, float env, float vol,
                 float lpan, float rpan, int *lohi)
{
    ZlBlockPlan pl;
    zl_plan_clear(pl);
    pl.flags = ZL_PLAN_ACTIVE; pl.n_active = N; pl.nseg = n1 == INT_MAX ? 1 : 2; pl.env = env; pl.P0 = (double)P0; pl.step = 1.0;
    if (n1 != INT_MAX) { pl.n1 = n1; pl.P1 = (double)P1; pl.step1 = 1.0; pl.E1 = env; }
    ZlVoiceConst vc{};
    vc.sample_duration = length - 1; vc.channels = stereo ? 2 : 1; vc.lgain = lgain; vc.rgain = rgain; vc.lpan = lpan; vc.rpan = rpan;
    vc.clip_volume = vol; vc.env = env;
    const int ipos = P0, alt = n1 == INT_MAX ? 0 : P1 - n1;         // (zl_k2_stage_unit)
    const int ch = stereo ? 2 : 1;
    int bad = 0, lo = INT_MAX, hi = INT_MIN;
    for (int f0 = 0; f0 < N; f0 += 2) {
        const ZlWrapLane w = zl_ongrid2_lane(ipos, alt, n1, f0);
        // the two loads: frames x and x + 1, and frame y
        lo = w.x < lo ? w.x : lo; lo = w.y < lo ? w.y : lo;
        hi = w.x + 1 > hi ? w.x + 1 : hi; hi = w.y > hi ? w.y : hi;
        const float *x = src + (size_t)w.x * ch, *y = src + (size_t)w.y * ch;
        float fr[2][2];
        fr[0][0] = x[0]; fr[0][1] = stereo ? x[1] : x[0];
        if (w.straddle) { fr[1][0] = y[0]; fr[1][1] = stereo ? y[1] : y[0]; }
        else            { fr[1][0] = x[ch]; fr[1][1] = stereo ? x[ch + 1] : x[ch]; }
        for (int h = 0; h < 2; ++h) {
            float l, r, dl, dr; int pos; double P; float e;
            zl_mix_frame_ongrid(fr[h][0], fr[h][1], lpan, rpan, l, r);
            zl_eval_control(pl, f0 + h, P, e);
            zl_render_frame<0>(vc, src, P, e, dl, dr, pos);
            if (!same_or_both_zero(l, dl) || !same_or_both_zero(r, dr)) ++bad;
        }
    }
    lohi[0] = lo; lohi[1] = hi;
    return bad;
}

// The classes of every (block, voice) of the LAST call a SimSynth rendered, as zl_k2_stage_class forms them (restated: the kernel's text is device
// code): out[K][V][6] = { 0 not on-grid / 1 on-grid, one segment / 2 on-grid with one loop restart,  n1,  P0,  P1,  mono,  source offset in floats }.
// A source counts as finite when every sample of it is (the engine's scan, zl_all_finite).
int zlwrap_scan(ZlSim *S, int ongrid, int32_t *out)
{
    const int K = S->lastK, N = S->lastN, V = S->V;
    ZlBatch A; std::memset(&A, 0, sizeof A);
    A.V = V; A.K = K; A.N = N; A.runs = S->runs.data(); A.plan_hdr = S->planHdr.data(); A.plan_seg0 = S->planSeg0.data(); A.plan_seg1 = S->planSeg1.data();
    for (int k = 0; k < K; ++k)
        for (int v = 0; v < V; ++v) {
            const ZlVoiceConst &vc = S->vconst[(size_t)v];
            const ZlBlockPlan pl = zl_plan_lookup(A, k, v, vc.env);
            int32_t *o = out + ((size_t)k * V + v) * 6;
            o[0] = 0; o[1] = pl.n1; o[2] = (int32_t)pl.P0; o[3] = (int32_t)pl.P1; o[4] = vc.channels == 1; o[5] = (int32_t)vc.src_offset;
            const int cls = (pl.flags & ZL_PLAN_ACTIVE) ? (1 | ((pl.flags & ZL_PLAN_SLOW) ? 2 : 0)) : 0;
            const float gprod = vc.lgain * vc.rgain * vc.clip_volume * pl.env;
            if (!(cls == 1 && pl.nseg <= 2 && !(pl.flags & ZL_PLAN_ENV) && pl.n_active == N && (vc.channels == 1 || vc.channels == 2)
                  && (gprod - gprod) == 0.0f && (uint32_t)vc.sample_duration < 0x1ffffff0u)) continue;
            const int flags = zl_all_finite(S->arena.data() + vc.src_offset, ((size_t)vc.sample_duration + 1) * (size_t)vc.channels) ? ZL_SOUND_FINITE : 0;
            const double Pmax = fma((double)(N - 1), pl.step, pl.P0);
            const bool interior = pl.nseg == 1 && pl.P0 >= 0.0 && Pmax < (double)vc.sample_duration;
            const bool unit = pl.nseg == 1 && pl.step == 1.0 && pl.P0 < 1073741824.0;
            if (zl_voice_ongrid(S->mode, ongrid, true, unit, interior, pl.P0, pl.step, flags)) o[0] = 1;
            if (zl_voice_ongrid2(S->mode, ongrid, flags, cls, pl.n_active, pl.flags, true, pl.nseg, pl.n1, N, pl.step, pl.step1, pl.P0, pl.P1, vc.sample_duration)) o[0] = 2;
        }
    return K;
}

int zlwrap_sound_finite_flag(void) { return ZL_SOUND_FINITE; }

}  // extern "C"

#ifdef ZL_PAIR_WRAP_MAIN
// every n1, stereo and mono, the loop's start at frame 0 of a buffer of exactly the source's size: a read outside it is the sanitizer's to find
static int fail(const char *what) { std::printf("pair wrap: FAILED %s\n", what); return 1; }

int main()
{
    const int N = 256, FIN = ZL_SOUND_FINITE;
    auto pred = [&](int ongrid, int flags, int cls, int n_active, int pf, int gf, int nseg, int n1, double step, double step1, double P0, double P1, int dur) {
        return zlwrap_predicate(0u, ongrid, flags, cls, n_active, pf, gf, nseg, n1, N, step, step1, P0, P1, dur);
    };
    if (!pred(3, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 900.0, 0.0, 1000)) return fail("the eligible block");
    if (pred(1, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 900.0, 0.0, 1000) || pred(2, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 900.0, 0.0, 1000)) return fail("the switch");
    if (pred(3, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 901.0, 0.0, 1000) || pred(3, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 900.0, 845.0, 1000)) return fail("a tap outside the source");
    if (pred(3, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 1e300, 0.0, 1000) || pred(3, FIN, 1, N, 0, 1, 2, 100, 1.0, 1.0, 900.0, -1e300, 1000)) return fail("positions no int holds");
    for (int stereo = 0; stereo < 2; ++stereo)
        for (int n1 = 1; n1 < N; ++n1)
            for (int start = 0; start < 3; ++start) {
                const int ch = stereo ? 2 : 1, loop = 700 + n1, length = start + loop + 1;       // (the loop ends one frame short of the source's last)
                float *src = (float *)std::malloc(((size_t)length + 8) * ch * sizeof(float));
                for (int i = 0; i < (length + 8) * ch; ++i) src[i] = i < length * ch ? (float)((i * 37 + n1) % 201 - 100) / 64.0f : 0.0f;
                int lohi[2];
                const int P0 = start + loop - n1, P1 = start;
                // (a loop that ends AT the source's last frame is not interior: that frame is silent, SamplerSynthVoice.cpp:204)
                if (!pred(3, FIN, 1, N, 0, 1, 2, n1, 1.0, 1.0, (double)P0, (double)P1, length - 1) || pred(3, FIN, 1, N, 0, 1, 2, n1, 1.0, 1.0, (double)P0, (double)P1, length - 2))
                    { std::free(src); return fail("interior or not"); }
                if (zlwrap_block(stereo, length, src, P0, P1, n1, N, 0.7f, 0.6f, 0.9f, 0.8f, 0.25f, 0.75f, lohi) != 0) { std::free(src); return fail("a frame"); }
                if (lohi[0] < 0 || lohi[1] >= length) { std::free(src); return fail("an address"); }
                if (zlwrap_block(stereo, length, src, start, 0, INT_MAX, N, 0.7f, 0.6f, 0.9f, 0.8f, 0.25f, 0.75f, lohi) != 0) { std::free(src); return fail("a single-segment frame"); }
                std::free(src);
            }
    std::printf("pair wrap: ok\n");
    return 0;
}
#endif
