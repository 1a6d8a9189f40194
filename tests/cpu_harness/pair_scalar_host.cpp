// Host build of the pair kernels' scalar records (libzl_amd/csrc/zl_render.h: zl_voice_block_class, zl_pair_fast_bits, zl_pair_group_need,
// zl_ongrid_addr0; zl_pair.h: zl_pair_scalar_window) for the CPU tier -- TEST HARNESS ONLY.  The class is the function K1c and the pair
// kernels' staging call; zlps_class_ref restates the text staging had before the two shared it, and the test holds one against the other over
// the boundary values of every input.  The records of a scene are made the way zl_k1c_assemble makes them -- ZlAssembler::block hands over
// the record it stores, the class is taken from it, a chunk's bit from the classes of its eight voices -- and the workgroups that skip
// staging are counted with the gate zl_k2_pair_body applies.  The planner comes with plan_host.cpp, included whole (as pair_wrap_host.cpp
// does): the test makes its ZlSim with this library's zlsim_create.
// -DZL_PAIR_SCALAR_MAIN: a program of its own (for the sanitizers) that runs the truth table and the bit helpers.
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "plan_host.cpp"
#include "zl_order.h"
#include "zl_pair.h"

// zl_k2_stage_class<MODE> as it stood before zl_voice_block_class (zl_kernels.hip of the parent commit), restated
static int class_ref(uint32_t mode, int ongrid, int trace, int N, const ZlVoiceConst &vc, const ZlBlockPlan &pl)
{
    int cls = (pl.flags & ZL_PLAN_ACTIVE) ? (1 | ((pl.flags & ZL_PLAN_SLOW) ? 2 : 0)) : 0;
    const float gprod = vc.lgain * vc.rgain * vc.clip_volume * pl.env;
    if (cls == 1 && pl.nseg <= 2 && !(pl.flags & ZL_PLAN_ENV) && pl.n_active == N && (vc.channels == 1 || vc.channels == 2) && !trace
        && (gprod - gprod) == 0.0f && (uint32_t)vc.sample_duration < 0x1ffffff0u)
    {
        const bool HM = (mode & ZL_MODE_HERMITE) != 0;
        const double Pmax = fma((double)(N - 1), pl.step, pl.P0);
        const bool interior = pl.nseg == 1 && pl.P0 >= (HM ? 1.0 : 0.0) && Pmax < (double)(vc.sample_duration - (HM ? 1 : 0));
        cls |= 4 | (pl.nseg == 2 ? 8 : 0) | (vc.channels == 1 ? 16 : 0) | ((pl.nseg == 1 && pl.step == 1.0 && pl.P0 < 1073741824.0) ? 32 : 0)
             | (interior ? 64 : 0);
        cls |= zl_voice_ongrid(mode, ongrid, true, (cls & 32) != 0, interior, pl.P0, pl.step, vc.pad[0]) ? 128 : 0;
        cls |= zl_voice_ongrid2(mode, ongrid, vc.pad[0], cls & 3, pl.n_active, pl.flags, true, pl.nseg, pl.n1, N, pl.step, pl.step1, pl.P0, pl.P1,
                                vc.sample_duration) ? 256 : 0;
    }
    return cls;
}

static void make_records(int plan_flags, int n_active, int nseg, float env, double P0, double step, int n1, double P1, double step1,
                         int channels, int duration, float lgain, float rgain, float vol, int sound_flags, ZlVoiceConst &vc, ZlBlockPlan &pl)
{
    zl_plan_clear(pl);
    pl.flags = plan_flags; pl.n_active = n_active; pl.nseg = nseg; pl.env = env; pl.P0 = P0; pl.step = step; pl.n1 = n1; pl.P1 = P1; pl.step1 = step1;
    vc = ZlVoiceConst{};
    vc.channels = channels; vc.sample_duration = duration; vc.lgain = lgain; vc.rgain = rgain; vc.clip_volume = vol; vc.pad[0] = sound_flags;
}

extern "C" {

// which = 0: zl_voice_block_class, 1: the restated text
int zlps_class(int which, unsigned mode, int ongrid, int trace, int N, int plan_flags, int n_active, int nseg, float env, double P0, double step,
               int n1, double P1, double step1, int channels, int duration, float lgain, float rgain, float vol, int sound_flags)
{
    ZlVoiceConst vc; ZlBlockPlan pl;
    make_records(plan_flags, n_active, nseg, env, P0, step, n1, P1, step1, channels, duration, lgain, rgain, vol, sound_flags, vc, pl);
    return which ? class_ref(mode, ongrid, trace, N, vc, pl) : zl_voice_block_class(mode, ongrid, trace, N, vc, pl);
}
int zlps_voice_fast(int cls) { return zl_voice_block_fast(cls) ? 1 : 0; }
unsigned zlps_fast_bits(unsigned long long fast, unsigned long long mono) { return zl_pair_fast_bits(fast, mono); }
unsigned zlps_group_need(int v0, int v1, int g) { return zl_pair_group_need(v0, v1, g); }
int zlps_gate(int sw, int pair, int phase_order, int have_tab, int VPB) { return zl_pair_scalar_window(sw, pair != 0, phase_order != 0, have_tab != 0, VPB) ? 1 : 0; }
unsigned long long zlps_addr0(unsigned long long arena, unsigned long long src_offset, double P0, int mono) { return zl_ongrid_addr0(arena, src_offset, P0, mono != 0); }
unsigned long long zlps_tab_words(int K, int V) { return (unsigned long long)zl_pair_tab_words(K, V); }

// The records of the LAST call a SimSynth rendered, as zl_k1c_assemble leaves them, and what zl_k2_pair_body makes of them.
//   bits[K][G]     the 16 bits of every (block, group of 64 voices)
//   run_end[B]     K1o's word per bus (zl_order_slot_run_end)
//   kind[K][B]     0 = the workgroup stages; 1 / 2 = it is a fast workgroup, stereo / mono (switch on, k >= run_end, not the call's last block, every chunk
//                  of the bus fast and of one layout)
//   cls[K][V]      the class staging forms for the voice-block (zl_plan_lookup + zl_voice_block_class), whatever path the workgroup takes
// A source counts as finite when every sample of it is (the engine's scan).  Returns the number of voice-blocks at or behind their bus's run_end
// whose bit, taken from K1c's record, is not the one staging's class gives: it must be 0 (one predicate, two readers).
int zlps_scan(ZlSim *S, int ongrid, uint16_t *bits, int32_t *run_end, int32_t *kind, int32_t *cls_out)
{
    const int K = S->lastK, N = S->lastN, V = S->V, B = S->B, VPB = S->VPB, G = (V + 63) / 64;
    std::vector<ZlVoiceConst> vconst = S->vconst;
    for (int v = 0; v < V; ++v) {
        const ZlVoiceConst &vc = vconst[(size_t)v];
        const bool fin = vc.channels > 0 && zl_all_finite(S->arena.data() + vc.src_offset, ((size_t)vc.sample_duration + 1) * (size_t)vc.channels);
        vconst[(size_t)v].pad[0] = fin ? ZL_SOUND_FINITE : 0;
    }
    // (K1c writes the records again: into copies, so that what the call left stays as it is)
    std::vector<ZlPlanHdr> hdr = S->planHdr; std::vector<ZlPlanSeg0> seg0 = S->planSeg0; std::vector<ZlPlanSeg1> seg1 = S->planSeg1;
    ZlBatch A; std::memset(&A, 0, sizeof A);
    A.V = V; A.B = B; A.VPB = VPB; A.K = K; A.N = N; A.Ktot = K; A.mode = S->mode; A.ongrid = ongrid;
    A.vconst = vconst.data(); A.runs = S->runs.data(); A.tsegs = S->tsegs.data(); A.plan_hdr = hdr.data(); A.plan_seg0 = seg0.data(); A.plan_seg1 = seg1.data();
    A.arena = S->arena.data();
    std::vector<int> vfast((size_t)K * V, 0), vmono((size_t)K * V, 0);
    const int bpl = V >= 512 ? 8 : 2;
    for (int v = 0; v < V; ++v)
        for (int kbeg = 0; kbeg < K; kbeg += bpl) {
            ZlAssembler as;
            const int kend = kbeg + bpl < K ? kbeg + bpl : K;
            as.begin(A, v, kbeg, kend);
            for (int k = kbeg; k < kend; ++k) {
                int idx0 = 0, base0 = 0, n_active = 0;
                ZlBlockPlan pl;
                as.block(A, k, idx0, base0, n_active, &pl);
                const int cls = zl_voice_block_class(0u, ongrid, 0, N, vconst[(size_t)v], pl);
                vfast[(size_t)k * V + v] = zl_voice_block_fast(cls) ? 1 : 0;
                vmono[(size_t)k * V + v] = (zl_voice_block_fast(cls) && (cls & 16)) ? 1 : 0;
            }
        }
    for (int k = 0; k < K; ++k)
        for (int g = 0; g < G; ++g) {
            unsigned long long mf = 0, mm = 0;
            for (int i = 0; i < 64 && 64 * g + i < V; ++i) {
                if (vfast[(size_t)k * V + 64 * g + i]) mf |= 1ull << i;
                if (vmono[(size_t)k * V + 64 * g + i]) mm |= 1ull << i;
            }
            bits[(size_t)k * G + g] = (uint16_t)zl_pair_fast_bits(mf, mm);
        }
    // staging's view, from the records the call left
    A.vconst = vconst.data(); A.plan_hdr = S->planHdr.data(); A.plan_seg0 = S->planSeg0.data(); A.plan_seg1 = S->planSeg1.data();
    int mismatches = 0;
    const bool gate = zl_pair_scalar_window(1, true, true, true, VPB) && (ongrid & ZL_ONGRID_ON);
    for (int b = 0; b < B; ++b) {
        const int v0 = b * VPB, v1 = v0 + VPB;
        run_end[b] = zl_order_slot_run_end(S->runs.data(), v0, v1, 1);
        for (int k = 0; k < K; ++k) {
            for (int v = v0; v < v1; ++v) {
                const ZlVoiceConst &vc = vconst[(size_t)v];
                const ZlBlockPlan pl = zl_plan_lookup(A, k, v, vc.env);
                const int cls = zl_voice_block_class(S->mode, ongrid, 0, N, vc, pl);
                cls_out[(size_t)k * V + v] = cls;
                if (k >= run_end[b] && (zl_voice_block_fast(cls) ? 1 : 0) != vfast[(size_t)k * V + v]) ++mismatches;
            }
            int kd = 0;
            if (gate && k >= run_end[b] && k != K - 1) {
                bool all = true, anyMono = false, allMono = true;
                for (int g = v0 >> 6; g <= (v1 - 1) >> 6; ++g) {
                    const uint32_t w = bits[(size_t)k * G + g], need = zl_pair_group_need(v0, v1, g);
                    all = all && (w & need) == need;
                    anyMono = anyMono || ((w >> 8) & need) != 0u;
                    allMono = allMono && ((w >> 8) & need) == need;
                }
                kd = !all ? 0 : allMono ? 2 : anyMono ? 0 : 1;
            }
            kind[(size_t)k * B + b] = kd;
        }
    }
    return mismatches;
}

}  // extern "C"

#ifdef ZL_PAIR_SCALAR_MAIN
static int fail(const char *what) { std::printf("pair scalar: FAILED %s\n", what); return 1; }

int main()
{
    const int N = 256, FIN = ZL_SOUND_FINITE;
    // the class against the restated text over the boundary values of every input, and the fast voice-block where it must be
    const double P0s[] = {0.0, 17.0, 17.5, 743.0, 744.0, 745.0, 1073741824.0, 1e300, -1.0};
    const double steps[] = {1.0, 1.0 + 2.220446049250313e-16, 1.0 - 1.1102230246251565e-16, 0.5, 2.0};
    const int durs[] = {998, 999, 1000, 0x1ffffff0 - 1, 0x1ffffff0, INT_MAX};
    const float envs[] = {0.8f, 0.0f, __builtin_inff(), __builtin_nanf("")};
    long n = 0, fast = 0;
    for (double P0 : P0s) for (double step : steps) for (int dur : durs) for (float env : envs)
        for (int nseg = 1; nseg <= 3; ++nseg) for (int ch = 1; ch <= 3; ++ch) for (int pf : {0, 1, 1 | 2, 1 | 4}) for (int na : {N, N - 1})
            for (int flags : {FIN, 0}) for (int ongrid : {0, 1, 3, 7}) for (unsigned mode : {0u, 1u, 4u}) {
                const int a = zlps_class(0, mode, ongrid, 0, N, pf, na, nseg, env, P0, step, nseg == 2 ? 100 : INT_MAX, 40.0, 1.0, ch, dur, 0.7f, 0.6f, 0.9f, flags);
                const int b = zlps_class(1, mode, ongrid, 0, N, pf, na, nseg, env, P0, step, nseg == 2 ? 100 : INT_MAX, 40.0, 1.0, ch, dur, 0.7f, 0.6f, 0.9f, flags);
                if (a != b) return fail("the class differs from the restated text");
                ++n; fast += zl_voice_block_fast(a) ? 1 : 0;
            }
    if (fast == 0 || fast == n) return fail("the sweep has no fast (or only fast) voice-blocks");
    // 743 + 255 = 998 < 999: interior; 744 + 255 = 999: not
    if (!zl_voice_block_fast(zlps_class(0, 0u, 1, 0, N, 1, N, 1, 0.8f, 743.0, 1.0, INT_MAX, 0.0, 0.0, 2, 999, 0.7f, 0.6f, 0.9f, FIN))) return fail("the fast voice-block");
    if (zl_voice_block_fast(zlps_class(0, 0u, 1, 0, N, 1, N, 1, 0.8f, 744.0, 1.0, INT_MAX, 0.0, 0.0, 2, 999, 0.7f, 0.6f, 0.9f, FIN))) return fail("a tap outside the source");
    if (zl_pair_fast_bits(~0ull, 0ull) != 0xffu || zl_pair_fast_bits(~0ull, ~0ull) != 0xffffu) return fail("all chunks fast");
    if (zl_pair_fast_bits(~0ull ^ (1ull << 19), 0ull) != (0xffu ^ 4u)) return fail("one voice of chunk 2 not fast");
    if (zl_pair_fast_bits(~0ull, 1ull << 9) != (0xffu ^ 2u)) return fail("a mono voice among stereo ones");
    if (zl_pair_group_need(0, 128, 0) != 0xffu || zl_pair_group_need(0, 128, 1) != 0xffu || zl_pair_group_need(0, 128, 2) != 0u) return fail("a bus of 128");
    if (zl_pair_group_need(72, 144, 1) != 0xfeu || zl_pair_group_need(72, 144, 2) != 0x03u || zl_pair_group_need(72, 144, 0) != 0u) return fail("bus 1 of two buses of 72");
    if (zl_pair_scalar_window(1, true, true, true, 12) || !zl_pair_scalar_window(1, true, true, true, 72) || zl_pair_scalar_window(0, true, true, true, 72)
        || zl_pair_scalar_window(1, false, true, true, 72) || zl_pair_scalar_window(1, true, false, true, 72) || zl_pair_scalar_window(1, true, true, false, 72)) return fail("the host gate");
    std::printf("pair scalar: ok (%ld classes, %ld fast)\n", n, fast);
    return 0;
}
#endif
