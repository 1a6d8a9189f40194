// zl_loudness.h -- a clip's loudness, measured on the device (zlhip_sound_loudness / _batch): the integrated
// loudness of ITU-R BS.1770-4 / EBU R 128 (K-weighting, 400 ms blocks with 75 % overlap, a -70 LUFS absolute and a -10 LU relative
// gate) and the sample peak, so that a bank of clips from different sources can be levelled (ClipAudioSource_setGain takes a dB value
// the caller must already know).  The reference has no loudness measurement, so this is a build-defined extension and claims no
// parity.  Shared by the HIP kernel (zl_loudness.hip), the engine and a host build for the CPU tier
// (tests/cpu_harness/loudness_host.cpp): everything is defined HERE, once.
//
// A request is (sound, first_frame, num_frames, sub_frames) over the sound's current playback data.
//
//   Weighting.  Two biquads per channel, a high shelf and the RLB high-pass, designed for the sound's rate on the host in double
//               (zl_ld_design): the bilinear form whose 48 kHz values are BS.1770's tables.  c[0..4] = the shelf's b0 b1 b2 a1 a2,
//               c[5..9] = the high-pass's 1 -2 1 a1 a2.
//   Arithmetic. Transposed direct form II in double, one IEEE operation per operator (build without contraction):
//               o = b0 v + s1; s1 = (b1 v - a1 o) + s2; s2 = b2 v - a2 o.  A sample is (double)v; a non-finite sample is 0; subnormals
//               are kept on both sides.
//   Sub-blocks. sub = sub_frames; given as 0: floor(rate 0.1 + 0.5).  S = num_frames / sub whole sub-blocks.  Sub-block k is filtered
//               from ZERO STATE at the start of sub-block k - 1 (one sub-block of warm-up; sub-block 0 from zero state at first_frame,
//               which is the standard itself), and only its own outputs are squared and summed, serially in sample order, per channel:
//               sum[c] += z z.  A work item is (request, k); the items are independent and an item runs in one order everywhere.
//   Short.      S < 4: the items are ceil(num_frames / sub) sub-blocks, the last one partial, and there is ONE block over the whole
//               region, z_0 = (u[0] + u[1] + ...) / num_frames.
//   Peak.       per item and channel max |v| over the finite samples of the item's own frames, compared as bits.  With S >= 4 the last
//               item also scans the dropped remainder (fewer than sub frames) for the peak, not for the sum.
//   Record.     per item ZlLdSub { double sum[2]; float peak[2]; } (zlhip_loudness_sub); a mono clip leaves sum[1] = 0, peak[1] = 0.
//   Finish.     host, double, sequential in index order (zl_ld_finish): the blocks, the two gates, lufs.
//
// The walk.  A lane owns an item and reads the frames [w, pe) of it in the 16-byte groups of the arena's own layout (stereo
// [L0 R0 L1 R1], mono [x0 x1 x2 x3]): one group per step, the elements of the first and the last group outside [w, pe) masked by
// their float index (zl_ov_valid), so no address outside the request is needed beyond the 16-byte group at each edge.  The lanes of a
// wavefront have different numbers of steps (rate, sub_frames, item 0's missing warm-up, a partial last item, the remainder): the
// loop runs to the group's maximum (zl_ld_group_steps) on every lane, and a lane past its own end (zl_ld_item_steps) idles.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_overview.h"
#include "zl_types.h"

#define ZL_LD_SUB_MIN            16
#define ZL_LD_SUB_MAX            131072
#define ZL_LD_MAX_ITEMS          65536       // per request
#define ZL_LD_MAX_CALL_ITEMS     1048576     // per call
#define ZL_LD_GROUP              64          // items of a workgroup: one lane each, one wavefront
#define ZL_LD_GATE_ABS           1.1724653045822981e-07      // 10^((-70 + 0.691) / 10)
#define ZL_LD_OFFSET             0.691

// the ten coefficients for `rate` (host, double); 0 = valid, -1 = not
inline int zl_ld_design(double rate, double *c)
{
    if (!(rate > 0.0 && rate < 1e9)) return -1;
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / rate), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / rate);
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
    return 0;
}

// sub_frames given as 0
inline int32_t zl_ld_default_sub(double rate) { return (int32_t)floor(rate * 0.1 + 0.5); }

// items of a region: S whole sub-blocks, or with S < 4 every sub-block, the last one partial
ZL_HD inline int64_t zl_ld_whole(int64_t num_frames, int32_t sub) { return num_frames / sub; }
ZL_HD inline int64_t zl_ld_items(int64_t num_frames, int32_t sub)
{
    const int64_t S = zl_ld_whole(num_frames, sub);
    return S >= 4 ? S : (num_frames + sub - 1) / sub;
}

// the default of sub_frames and the limits that need no sound; the only place they are written.  0 = valid, -1 = not
inline int zl_ld_resolve(double rate, int32_t first_frame, int32_t num_frames, int32_t *sub)
{
    if (!(rate > 0.0 && rate < 1e9) || first_frame < 0 || num_frames < 1) return -1;
    int32_t s = *sub;
    if (s == 0) {
        const double d = floor(rate * 0.1 + 0.5);
        if (!(d >= (double)ZL_LD_SUB_MIN && d <= (double)ZL_LD_SUB_MAX)) return -1;
        s = (int32_t)d;
    }
    if (s < ZL_LD_SUB_MIN || s > ZL_LD_SUB_MAX) return -1;
    if (zl_ld_items(num_frames, s) > ZL_LD_MAX_ITEMS) return -1;
    *sub = s;
    return 0;
}

// One request of a call as the kernel sees it (built by the host)
struct ZlLdRequest {
    uint64_t src;                // device address of the extent the sound plays (16-byte aligned)
    double   c[10];              // zl_ld_design of the sound's rate
    int32_t  first, frames, sub, channels;
    int32_t  items;              // zl_ld_items
    int32_t  item_base;          // the request's first item of the call, and its first record
};

// a sub-block's record (zlhip_loudness_sub's layout)
struct ZlLdSub { double sum[2]; float peak[2]; };

// the result (zlhip_loudness's layout)
struct ZlLdResult { double lufs, mean_square, relative_gate; float peak[2]; int32_t sub_blocks, blocks, above_absolute, above_relative; };

// Item k of a request: it walks the frames [w, pe), sums the outputs of [s0, s1) and takes the peak of [s0, pe), all absolute frames
// of the sound.  The 16-byte groups [g0, g0 + steps) hold them; head and count are zl_ov_valid's.
struct ZlLdItem { int64_t g0; int32_t steps, head, count, own, end; };      // own = s0 - w, end = s1 - w, relative to w

ZL_HD inline void zl_ld_item_frames(const ZlLdRequest &R, int32_t k, int64_t *w, int64_t *s0, int64_t *s1, int64_t *pe)
{
    const int64_t stop = (int64_t)R.first + R.frames;
    *s0 = (int64_t)R.first + (int64_t)k * R.sub;
    *s1 = *s0 + R.sub < stop ? *s0 + R.sub : stop;
    *w = k > 0 ? *s0 - R.sub : *s0;
    *pe = k == R.items - 1 ? stop : *s1;
}

ZL_HD inline ZlLdItem zl_ld_item(const ZlLdRequest &R, int32_t k)
{
    int64_t w, s0, s1, pe, f0, f1, g0, g1;
    zl_ld_item_frames(R, k, &w, &s0, &s1, &pe);
    zl_ov_groups(w, pe, R.channels, &f0, &f1, &g0, &g1);
    ZlLdItem I;
    I.g0 = g0; I.steps = (int32_t)(g1 - g0); I.head = (int32_t)(f0 - 4 * g0); I.count = (int32_t)(f1 - f0);
    I.own = (int32_t)(s0 - w); I.end = (int32_t)(s1 - w);
    return I;
}

// the request of item `at` of the call: the last one whose item_base is <= at (every request has at least one item)
ZL_HD inline int32_t zl_ld_find(const ZlLdRequest *reqs, int32_t nreq, int32_t at)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if (reqs[mid].item_base <= at) lo = mid; else hi = mid - 1;
    }
}

// the steps of item `item` of the call (0 behind the call's last item), and of the group of ZL_LD_GROUP items `group`: its maximum
ZL_HD inline int32_t zl_ld_item_steps(const ZlLdRequest *reqs, int32_t nreq, int32_t items, int32_t item)
{
    if (item >= items) return 0;
    const ZlLdRequest &R = reqs[zl_ld_find(reqs, nreq, item)];
    return zl_ld_item(R, item - R.item_base).steps;
}
ZL_HD inline int32_t zl_ld_group_steps(const ZlLdRequest *reqs, int32_t nreq, int32_t items, int32_t group)
{
    int32_t m = 0;
    for (int32_t l = 0; l < ZL_LD_GROUP; ++l) {
        const int32_t s = zl_ld_item_steps(reqs, nreq, items, group * ZL_LD_GROUP + l);
        m = s > m ? s : m;
    }
    return m;
}

// a lane's accumulators per channel: the two biquads' states, the sum, the peak as bits (named members, not arrays: they stay in registers)
struct ZlLdChan { double s0, s1, s2, s3, sum; uint32_t peak; };
struct ZlLdAcc { ZlLdChan l, r; };

ZL_HD inline void zl_ld_acc_init(ZlLdAcc &a)
{
    a.l.s0 = a.l.s1 = a.l.s2 = a.l.s3 = a.l.sum = 0.0; a.l.peak = 0u;
    a.r = a.l;
}

// one sample (its 32 bits) of a channel at the frame `rel` frames behind w
ZL_HD inline __attribute__((always_inline)) void zl_ld_sample(const double *c, const ZlLdItem &I, ZlLdChan &a, int32_t rel, uint32_t bits)
{
    const bool finite = (bits & 0x7f800000u) != 0x7f800000u, own = rel >= I.own;
    const uint32_t mag = bits & 0x7fffffffu;
    a.peak = own && finite && mag > a.peak ? mag : a.peak;
    const double v = finite ? (double)__builtin_bit_cast(float, bits) : 0.0;
    const double y = c[0] * v + a.s0;
    a.s0 = (c[1] * v - c[3] * y) + a.s1;
    a.s1 = c[2] * v - c[4] * y;
    const double z = c[5] * y + a.s2;
    a.s2 = (c[6] * y - c[8] * z) + a.s3;
    a.s3 = c[7] * y - c[9] * z;
    const double q = z * z;
    a.sum += own && rel < I.end ? q : 0.0;                         // (the sums are never -0: adding +0 changes nothing)
}

// step n of an item of a sound of kChannels channels: the four words of group g0 + n.  (A template, and a walk per channel count
// around it: one body with a run-time choice of the channel makes the compiler address the accumulators through memory.)
template <int kChannels> ZL_HD inline __attribute__((always_inline)) void zl_ld_step(const double *c, const ZlLdItem &I, int32_t n, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, ZlLdAcc &a)
{
    const int32_t rel = 4 * n - I.head;
    if (kChannels == 2) {                                          // head and count are even: a frame never straddles two groups
        if (zl_ov_valid(n, 0, I.head, I.count)) { zl_ld_sample(c, I, a.l, rel >> 1, v0); zl_ld_sample(c, I, a.r, rel >> 1, v1); }
        if (zl_ov_valid(n, 2, I.head, I.count)) { zl_ld_sample(c, I, a.l, (rel + 2) >> 1, v2); zl_ld_sample(c, I, a.r, (rel + 2) >> 1, v3); }
    } else {
        if (zl_ov_valid(n, 0, I.head, I.count)) zl_ld_sample(c, I, a.l, rel, v0);
        if (zl_ov_valid(n, 1, I.head, I.count)) zl_ld_sample(c, I, a.l, rel + 1, v1);
        if (zl_ov_valid(n, 2, I.head, I.count)) zl_ld_sample(c, I, a.l, rel + 2, v2);
        if (zl_ov_valid(n, 3, I.head, I.count)) zl_ld_sample(c, I, a.l, rel + 3, v3);
    }
}

ZL_HD inline ZlLdSub zl_ld_record(const ZlLdAcc &a)
{
    ZlLdSub r;
    r.sum[0] = a.l.sum; r.sum[1] = a.r.sum;
    r.peak[0] = __builtin_bit_cast(float, a.l.peak); r.peak[1] = __builtin_bit_cast(float, a.r.peak);
    return r;
}

// The result from a request's records (host, double, sequential in index order; build without contraction)
inline void zl_ld_finish(const ZlLdSub *subs, int32_t num_frames, int32_t sub, ZlLdResult *out)
{
    const int64_t S = zl_ld_whole(num_frames, sub), items = zl_ld_items(num_frames, sub), blocks = S >= 4 ? S - 3 : 1;
    ZlLdResult o;
    o.lufs = -INFINITY; o.mean_square = 0.0; o.relative_gate = 0.0; o.peak[0] = 0.0f; o.peak[1] = 0.0f;
    o.sub_blocks = (int32_t)items; o.blocks = (int32_t)blocks; o.above_absolute = 0; o.above_relative = 0;
    for (int64_t k = 0; k < items; ++k)
        for (int ch = 0; ch < 2; ++ch) if (subs[k].peak[ch] > o.peak[ch]) o.peak[ch] = subs[k].peak[ch];      // (finite and >= 0: float order is bit order)
    auto u = [&](int64_t k) { return subs[k].sum[0] + subs[k].sum[1]; };
    auto z = [&](int64_t j) {
        if (S >= 4) return (((u(j) + u(j + 1)) + u(j + 2)) + u(j + 3)) / (double)(4 * (int64_t)sub);
        double t = 0.0;
        for (int64_t k = 0; k < items; ++k) t += u(k);
        return t / (double)num_frames;
    };
    double total = 0.0; int64_t A = 0;
    for (int64_t j = 0; j < blocks; ++j) { const double zj = z(j); if (zj > ZL_LD_GATE_ABS) { total += zj; ++A; } }
    if (A > 0) {
        const double rel = (total / (double)A) / 10.0;
        double pass = 0.0; int64_t B = 0;
        for (int64_t j = 0; j < blocks; ++j) { const double zj = z(j); if (zj > ZL_LD_GATE_ABS && zj > rel) { pass += zj; ++B; } }
        o.relative_gate = rel; o.above_absolute = (int32_t)A; o.above_relative = (int32_t)B;
        o.mean_square = pass / (double)B;                          // (B >= 1: the largest passing block is above their mean / 10)
        o.lufs = -ZL_LD_OFFSET + 10.0 * log10(o.mean_square);
    }
    *out = o;
}

// a whole request by one thread, item by item as the kernel walks it (the host route of scripts/loudness_bench.py).  data: the sound's
// playback data from frame 0 in the arena's layout, 16-byte aligned, whole groups readable
inline void zl_ld_item_serial(const ZlLdRequest &R, int32_t k, const uint32_t *data, ZlLdSub *out)
{
    const ZlLdItem I = zl_ld_item(R, k);
    ZlLdAcc a;
    zl_ld_acc_init(a);
    for (int32_t n = 0; n < I.steps; ++n) {
        const uint32_t *g = data + 4 * (I.g0 + n);
        if (R.channels == 2) zl_ld_step<2>(R.c, I, n, g[0], g[1], g[2], g[3], a); else zl_ld_step<1>(R.c, I, n, g[0], g[1], g[2], g[3], a);
    }
    *out = zl_ld_record(a);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launcher (zl_loudness.hip; 0 or a hipError_t value).  out [items] may be host memory mapped into the device: only the records are written
int zl_launch_loudness(const ZlLdRequest *reqs, int32_t nreq, int32_t items, ZlLdSub *out, hipStream_t s);
#endif
