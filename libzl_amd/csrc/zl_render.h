// zl_render.h -- per-frame arithmetic of SamplerSynthVoice::process (reference
// lib/SamplerSynthVoice.cpp:198-216): fractional-index gather, linear (or Hermite) interpolation,
// gain / envelope / clip volume, M/S pan.  One call = one (voice, frame).  The operation order is
// the reference's expression order; the translation unit must be built with -ffp-contract=off so
// no multiply-add is fused (the oracle defines the same rounding sequence).
//
// __host__ __device__ so tests/cpu_harness can execute the identical code on the CPU.
#pragma once
#include "zl_types.h"
#include <math.h>
#include <stddef.h>
#include <string.h>

// Position and envelope of frame f of a planned FAST block (at most two inline segments; blocks with per-frame control: zl_plan.h,
// zl_slow_control).
ZL_HD inline void zl_eval_control(const ZlBlockPlan &pl, int f, double &P, float &env)
{
    const bool seg1 = f >= pl.n1;
    const int n0 = seg1 ? pl.n1 : 0;
    P = fma((double)(f - n0), seg1 ? pl.step1 : pl.step, seg1 ? pl.P1 : pl.P0);                     // exact (see zl_plan.h)
    env = (float)fma((double)(f - n0), (double)(seg1 ? pl.estep1 : pl.estep0), (double)(seg1 ? pl.E1 : pl.env));   // exact fp32 ramp
}

// 4-point Catmull-Rom (build-defined extension, absent in the reference) in TAP-WEIGHT form: the four cubic
// weights of the fractional position a,
//   w0 = ((-a/2 + 1) a - 1/2) a    w1 = (3/2 a - 5/2) a^2 + 1    w2 = ((-3/2 a + 2) a + 1/2) a    w3 = (a/2 - 1/2) a^2,
// are computed once per frame and shared by both channels; y = w0 y0 + w1 y1 + w2 y2 + w3 y3.  Fused multiply-adds in
// exactly this order (11 operations for the weights + 4 per channel; every fmaf is ONE rounding -- the oracle and the numpy
// restatement do the same).  The Horner form of round 1 cost 12 per channel: the kernel is bound by VALU issue in this mode.
struct ZlHermiteW { float w0, w1, w2, w3; };
ZL_HD inline ZlHermiteW zl_hermite_weights(float a)
{
    ZlHermiteW w;
    const float t = a * a;
    w.w0 = fmaf(fmaf(-0.5f, a, 1.0f), a, -0.5f) * a;
    w.w1 = fmaf(fmaf(1.5f, a, -2.5f), t, 1.0f);
    w.w2 = fmaf(fmaf(-1.5f, a, 2.0f), a, 0.5f) * a;
    w.w3 = fmaf(0.5f, a, -0.5f) * t;
    return w;
}
ZL_HD inline float zl_hermite4(float y0, float y1, float y2, float y3, const ZlHermiteW &w)
{
    return fmaf(w.w3, y3, fmaf(w.w2, y2, fmaf(w.w1, y1, w.w0 * y0)));
}

// The gathered samples of one frame: taps pos, pos+1 (and pos-1, pos+2 for Hermite) of both channels.
struct ZlTaps {
    float x0l, x0r, x1l, x1r;       // pos, pos+1
    float xml, xmr, x2l, x2r;       // pos-1, pos+2 (Hermite only)
};

// :198-199 -- integer position and fractional part
ZL_HD inline void zl_split_position(double P, int &pos, float &alpha)
{
    pos = (int)P;
    alpha = (float)(P - (double)pos);
}

// :204-211 on gathered taps.  inb = guard of :204 (Q5); wide = all four Hermite taps are inside the
// source; stereo = the source has a second channel.  Returns the panned (l', r') of :210-211.
template <uint32_t MODE>
ZL_HD inline void zl_mix_frame(const ZlTaps &t, float alpha, bool inb, bool wide, bool stereo,
                               float lgain, float rgain, float env, float vol, float lpan, float rpan,
                               float &lout, float &rout)
{
    const float invAlpha = 1.0f - alpha;                         // :200
    float l, r;
    if (MODE & ZL_MODE_HERMITE) {
        // build-defined extension: Catmull-Rom, linear at the source edges; whole-sample gain with the gain product formed first,
        // sample * ((gain * envelope) * volume) -- for a voice in sustain the product is one number per block
        const ZlHermiteW w = zl_hermite_weights(alpha);
        const float sl = wide ? zl_hermite4(t.xml, t.x0l, t.x1l, t.x2l, w) : (t.x0l * invAlpha + t.x1l * alpha);
        const float sr = wide ? zl_hermite4(t.xmr, t.x0r, t.x1r, t.x2r, w) : (t.x0r * invAlpha + t.x1r * alpha);
        l = sl * ((lgain * env) * vol);
        r = sr * ((rgain * env) * vol);
    } else if (MODE & ZL_MODE_FIX_GAIN) {
        l = (t.x0l * invAlpha + t.x1l * alpha) * lgain * env * vol;
        r = (t.x0r * invAlpha + t.x1r * alpha) * rgain * env * vol;
    } else {
        // :204-205 -- quirk Q1: the gain chain multiplies only the second tap
        l = t.x0l * invAlpha + t.x1l * alpha * lgain * env * vol;
        r = t.x0r * invAlpha + t.x1r * alpha * rgain * env * vol;
    }
    if (!inb) l = 0.0f;
    if (!(stereo && inb)) r = l;                                 // :205 mono source / out of range: r = l
    const float mSignal = 0.5f * (l + r);                        // :208 (0.5 * float in double, exact)
    const float sSignal = l - r;                                 // :209
    lout = lpan * mSignal + sSignal;                             // :210
    rout = rpan * mSignal - sSignal;                             // :211
}

// ---- on-grid unit-step voices: one tap ---------------------------------------------------------------------------------------------
// A voice that plays at its own rate from an integer position has alpha = 0 in every frame, and the plain linear expression above is
//   l = x0l * 1.0f + (((x1l * 0.0f) * lgain) * env) * vol = x0l + (a signed zero)          whenever x1l and the gains are finite.
// The zero's sign reaches no output: l + r and l - r depend on it only when l and r are both zero; then lout and rout are zeros, the
// bus accumulator starts at +0 and never becomes -0 (+0 + -0 = +0, x + -x = +0), and the report peak is ng > 0 ? ng : 0.  So the
// second tap, its gain chain and 1 - alpha can go -- where the source is KNOWN to be finite (inf * 0 = NaN): ZL_SOUND_FINITE.
//
// Does K2 take the short form for this voice-block?  simple / unit / interior: the staging classes of zl_k2_body (whole block in
// sustain with finite gains; one segment of step exactly 1; every tap inside the source).
ZL_HD inline bool zl_voice_ongrid(uint32_t mode, int enabled, bool simple, bool unit, bool interior, double P0, double step, int sound_flags)
{
    return enabled != 0 && simple && unit && interior && step == 1.0 && P0 == (double)(int)P0 && (sound_flags & ZL_SOUND_FINITE) != 0
        && (mode & (ZL_MODE_HERMITE | ZL_MODE_FIX_GAIN)) == 0;
}

// The same for a block that holds ONE loop restart (two segments): both segments of a clip at its own pitch and rate are unit-step runs
// from integer positions, so alpha = 0 in every frame of both and each frame is zl_mix_frame_ongrid on the first tap of its own segment --
// frame f reads position P0 + f below n1 and P1 + (f - n1) from n1 on.  `ongrid` is ZlBatch::ongrid: bit 0 the on-grid form, bit 1 this
// one (ZL_K2_PAIR_WRAP).  cls / n_active / plan_flags / gains_finite: the voice plays the whole block (cls == 1: no per-frame control) in
// sustain with a finite gain product.  Every tap of both segments lies inside the source: the first segment's last frame is n1 - 1, the
// second's is N - 1.
#define ZL_ONGRID_ON   1
#define ZL_ONGRID_WRAP 2
ZL_HD inline bool zl_voice_ongrid2(uint32_t mode, int ongrid, int sound_flags, int cls, int n_active, int plan_flags, bool gains_finite,
                                   int nseg, int n1, int N, double step, double step1, double P0, double P1, int sample_duration)
{
    return (ongrid & ZL_ONGRID_ON) != 0 && (ongrid & ZL_ONGRID_WRAP) != 0 && (mode & (ZL_MODE_HERMITE | ZL_MODE_FIX_GAIN)) == 0
        && (sound_flags & ZL_SOUND_FINITE) != 0
        && cls == 1 && n_active == N && (plan_flags & ZL_PLAN_ENV) == 0 && gains_finite
        && nseg == 2 && n1 > 0 && n1 < N
        && step == 1.0 && step1 == 1.0
        && P0 >= 0.0 && P0 < 1073741824.0 && P0 == (double)(int)P0 && P1 >= 0.0 && P1 < 1073741824.0 && P1 == (double)(int)P1
        && P0 + (double)(n1 - 1) < (double)sample_duration && P1 + (double)(N - 1 - n1) < (double)sample_duration;
}

// What a lane of the two-frames-per-lane kernels reads of such a voice (zl_kernels.hip, zl_k2_chunk_ongrid_pair_wrap).  The lane renders
// frames f0 (even) and f0 + 1.  ipos = P0 and alt = P1 - n1 as integers (alt may be negative: it is only added to frames >= n1), both in
// source frames; a single-segment on-grid voice of the same chunk has n1 = INT_MAX.  x = the source frame of a two-frame load (frames x
// and x + 1), y = the source frame of a one-frame load; frame f0 is x's first frame, frame f0 + 1 is y where `straddle` (f0 + 1 == n1: one
// frame from each segment) and x's second frame otherwise.  Where the lane does not straddle y = x, a frame it reads anyway: no lane
// reads in front of P1, and a straddling lane's unused frame x + 1 = P0 + n1 <= sample_duration is the source's own.
struct ZlWrapLane { int x, y; bool straddle; };
ZL_HD inline ZlWrapLane zl_ongrid2_lane(int ipos, int alt, int n1, int f0)
{
    ZlWrapLane w;
    w.x = (f0 >= n1 ? alt : ipos) + f0;
    w.straddle = f0 + 1 == n1;
    w.y = w.straddle ? alt + f0 + 1 : w.x;
    return w;
}

// The class bits of one voice-block as K2's pair kernels stage it (zl_kernels.hip, zl_k2_stage_class) and as K1c reads it when it leaves
// the scalar records below: 1 = plays this block, 2 = per-frame control, 4 = "simple" (whole block, sustain, finite gains, no debug
// trace), 8 = it has a second position segment, 16 = mono source, 32 = unit step, 64 = "interior" (every tap of the block inside the
// source), 128 = on-grid (zl_voice_ongrid), 256 = on-grid with one loop restart (zl_voice_ongrid2).  One text for both readers and for
// the CPU tier (tests/cpu_harness/pair_scalar_host.cpp).  zl_k2_body's kernels keep their own text (zl_kernels.hip, above zl_k2_stage_load).
ZL_HD inline int zl_voice_block_class(uint32_t mode, int ongrid, int trace, int N, const ZlVoiceConst &vc, const ZlBlockPlan &pl)
{
    int cls = (pl.flags & ZL_PLAN_ACTIVE) ? (1 | ((pl.flags & ZL_PLAN_SLOW) ? 2 : 0)) : 0;
    const float gprod = vc.lgain * vc.rgain * vc.clip_volume * pl.env;     // finite iff every factor is (or one is 0 * inf = NaN)
    // (sources of 4 GiB and more take the general path: the simple paths address a source with 32-bit byte offsets)
    if (cls == 1 && pl.nseg <= 2 && !(pl.flags & ZL_PLAN_ENV) && pl.n_active == N && (vc.channels == 1 || vc.channels == 2) && !trace
        && (gprod - gprod) == 0.0f && (uint32_t)vc.sample_duration < 0x1ffffff0u)
    {
        // first and last position of the block (P0 and P0 + (N-1) step, step > 0) leave room for every tap: pos + 1 <= duration
        // (pos >= 1 and pos + 2 <= duration with 4 taps)
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

// ---- the pair kernels' scalar records (ZL_K2_PAIR_SCALAR; zl_kernels.hip: K1c writes them, zl_k2_pair_body reads them with scalar loads) --------
// What an on-grid chunk reads of a voice-block is wave-uniform: the byte address of the block's frame 0 and the pan pair.  K1c holds the
// block's plan when it stores it and leaves, per window and record set, in ONE buffer of 8-byte words (zl_batch_pair_tab, zl_types.h):
//   addr0[k V + v]        words [0, K V): the address, as zl_unit_record forms it -- meaningful only where the voice-block is on-grid
//   pan[v]                words [K V, K V + V): (lpan, rpan) of ZlVoiceConst, dense
//   fast[k G + g]         behind them, 16 bits per (block, group of 64 voices; G = ceil(V / 64)): bit c = chunk c of the group (voices 8 c .. 8 c + 7)
//                         is FAST -- every voice on-grid, interior, one segment, all of one source layout, which is the chunk class test
//                         (cc & 132) == 132 of the staged path; bit 8 + c = the chunk is all mono.  A block that an inline run covers
//                         or K1 simulated has no record assembled by K1c: its bit is 0.
#define ZL_ONGRID_SCALAR 4        // ZlBatch::ongrid bit 2 (only with bit 0): this window's K1c writes the records and its pair launch reads them
ZL_HD inline size_t zl_pair_tab_pan(int K, int V) { return (size_t)K * (size_t)V; }
ZL_HD inline size_t zl_pair_tab_fast(int K, int V) { return (size_t)K * (size_t)V + (size_t)V; }
ZL_HD inline size_t zl_pair_tab_words(int K, int V) { return zl_pair_tab_fast(K, V) + ((size_t)K * (size_t)((V + 63) / 64) * 2 + 7) / 8; }
// a voice-block of this class is one a fast chunk may hold; its layout bit
ZL_HD inline bool zl_voice_block_fast(int cls) { return (cls & (4 | 64 | 128)) == (4 | 64 | 128); }
// frame 0 of an on-grid voice-block: arena + 4 src_offset + 8 ipos (4 ipos mono) in 64-bit unsigned arithmetic, which wraps modulo 2^64 for
// a source in a grown arena segment exactly as zl_unit_record's does
ZL_HD inline uint64_t zl_ongrid_addr0(uint64_t arena, uint64_t src_offset, double P0, bool mono)
{
    return arena + (src_offset << 2) + ((uint64_t)(uint32_t)(int)P0 << (mono ? 2 : 3));
}
// the 16 bits of one (block, group): cls[i] = class of voice 64 g + i (0 for a voice the group does not have)
ZL_HD inline uint32_t zl_pair_fast_bits(unsigned long long fast, unsigned long long mono)
{
    uint32_t w = 0;
    for (int c = 0; c < 8; ++c) {
        const unsigned f = (unsigned)(fast >> (8 * c)) & 255u, m = (unsigned)(mono >> (8 * c)) & 255u;
        if (f == 255u && (m == 0u || m == 255u)) w |= 1u << c;
        if (m == 255u) w |= 256u << c;
    }
    return w;
}
// the chunks of voices [v0, v1) (both multiples of 8) inside group g as a mask of the group's 8 bits; 0: none
ZL_HD inline uint32_t zl_pair_group_need(int v0, int v1, int g)
{
    const int lo = v0 > 64 * g ? v0 : 64 * g, hi = v1 < 64 * g + 64 ? v1 : 64 * g + 64;
    if (hi <= lo) return 0u;
    return ((1u << ((hi - lo) >> 3)) - 1u) << ((lo - 64 * g) >> 3);
}

// :208-211 on the one tap (x0l, x0r) of an on-grid frame; a mono source passes x0r = x0l (r = l, :205)
ZL_HD inline void zl_mix_frame_ongrid(float x0l, float x0r, float lpan, float rpan, float &lout, float &rout)
{
    const float mSignal = 0.5f * (x0l + x0r);                    // :208
    const float sSignal = x0l - x0r;                             // :209
    lout = lpan * mSignal + sSignal;                             // :210
    rout = rpan * mSignal - sSignal;                             // :211
}

// The same frame as K2's packed on-grid mix evaluates it (zl_kernels.hip, zl_mix_acc_ongrid_pk: five v_pk_*_f32 over the pairs
// (sum, difference) and (left, right)), restated operation for operation so that the CPU tier can hold it against the definition
// above: a - b is a + (-b) (the neg_hi source modifier: a negation is exact, so this is the same IEEE operation on every input),
// and where the 0.5 multiply is a packed one the difference rides through it in the other half of the pair, times 1.0f (x * 1.0f = x
// for every finite or infinite x; a NaN stays a NaN) -- the kernel as built multiplies the sum's half alone, which is the same frame.
// Nothing is fused.
ZL_HD inline void zl_mix_frame_ongrid_pk(float x0l, float x0r, float lpan, float rpan, float &lout, float &rout)
{
    const float sum = x0l + x0r, dif = x0l + (-x0r);             // v_pk_add_f32, neg_hi
    const float m = sum * 0.5f, s = dif * 1.0f;                  // v_pk_mul_f32 by (0.5, 1.0), or v_mul_f32 on the sum alone
    const float lm = lpan * m, rm = rpan * m;                    // v_pk_mul_f32, the mid signal in both halves
    lout = lm + s;                                               // v_pk_add_f32, neg_hi
    rout = rm + (-s);
}

// is every sample of a host buffer finite?  (the exponent field of a NaN or an infinity is all ones)
ZL_HD inline bool zl_f32_bits_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
inline bool zl_all_finite(const float *x, size_t n)
{
    uint32_t worst = 0;
    for (size_t i = 0; i < n; ++i) { uint32_t b; memcpy(&b, x + i, sizeof b); worst |= zl_f32_bits_finite(b) ? 0u : 1u; }
    return worst == 0;
}

// JackPassthrough fan-out of one bus frame (JackPassthrough.cpp:55-109): output pair c (0 dry, 1 wetFx1, 2 wetFx2) of
// input (sl, sr).  lm, rm = zl_pass_pan().  The memset / memcpy fast paths of the reference are value-identical to
// these selects (they differ from the multiply only in the sign of zero and for non-finite input, which is why they
// are kept).
ZL_HD inline void zl_pass_pan(const ZlPassParams &p, float &lm, float &rm)
{
    const float a = 1 - p.pan, b = 1 + p.pan;
    lm = (1.0f < a) ? 1.0f : a;                                  // std::min(1 - panAmount, 1.0f), :100
    rm = (1.0f < b) ? 1.0f : b;                                  // :101
}
ZL_HD inline void zl_pass_pair(const ZlPassParams &p, float amount, float lm, float rm, float sl, float sr, float &ol, float &orr)
{
    if (p.muted)                            { ol = 0.0f; orr = 0.0f; }                      // :55-61
    else if (p.pan == 0 && amount == 0)     { ol = 0.0f; orr = 0.0f; }                      // :66-69 memset
    else if (p.pan == 0 && amount == 1)     { ol = sl;   orr = sr; }                        // :70-73 memcpy
    else                                    { ol = amount * sl * lm; orr = amount * sr * rm; }   // :100-109
}

// Host-side convenience used by tests/cpu_harness: gather + mix for one (voice, frame).
// src points at the voice's source in the arena (interleaved stereo or mono).
template <uint32_t MODE>
ZL_HD inline void zl_render_frame(const ZlVoiceConst &vc, const float *src, double P, float env,
                                  float &lout, float &rout, int &pos_out)
{
    int pos; float alpha;
    zl_split_position(P, pos, alpha);
    const bool inb = vc.sample_duration > pos && pos >= 0;       // :204 guard; pos < 0 cannot occur for P >= 0
    const bool stereo = vc.channels > 1;
    const bool wide = (MODE & ZL_MODE_HERMITE) && inb && (pos - 1 >= 0) && (pos + 2 <= vc.sample_duration);
    const int p = inb ? pos : 0;
    ZlTaps t;
    t.xml = t.xmr = t.x2l = t.x2r = 0.0f;
    if (stereo) {
        t.x0l = src[2 * p]; t.x0r = src[2 * p + 1]; t.x1l = src[2 * p + 2]; t.x1r = src[2 * p + 3];
        if (wide) { t.xml = src[2 * p - 2]; t.xmr = src[2 * p - 1]; t.x2l = src[2 * p + 4]; t.x2r = src[2 * p + 5]; }
    } else {
        t.x0l = src[p]; t.x1l = src[p + 1]; t.x0r = 0.0f; t.x1r = 0.0f;
        if (wide) { t.xml = src[p - 1]; t.x2l = src[p + 2]; }
    }
    zl_mix_frame<MODE>(t, alpha, inb, wide, stereo, vc.lgain, vc.rgain, env, vc.clip_volume, vc.lpan, vc.rpan, lout, rout);
    pos_out = pos;
}

// One sample of a 16-bit WAV as the reference's recorder writes it (AudioLevels.cpp:53-58: a juce::WavAudioFormat writer, 16 bit,
// fed floats through AudioFormatWriter::ThreadedWriter): float -> 32-bit fixed point (clamped at +-1, times 0x7fffffff in double,
// round to nearest even) -> its upper 16 bits.  JUCE is not in the tree: restated from its public source (convertFloatsToInts +
// the Int32 -> Int16 little-endian write), version unpinned like the ADSR.  NaN, which JUCE leaves
// undefined, is written as 0.  The reader side (zl_libzl.cpp, libzl_wav_read) is the inverse convention.
ZL_HD inline int16_t zl_pcm16(float x)
{
    const double d = (double)x;
    int32_t q;
    if (d <= -1.0) q = INT32_MIN;
    else if (d >= 1.0) q = INT32_MAX;
    else if (d != d) q = 0;
    else q = (int32_t)rint(2147483647.0 * d);                   // |.| < 2^31: fits
    return (int16_t)(q >> 16);
}
