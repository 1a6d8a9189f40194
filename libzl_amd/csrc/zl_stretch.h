// zl_stretch.h -- the clip re-render behind zlhip_sound_rerender: a SoundTouch-shaped WSOLA time stretch,
// a linear resampler and a gain, defined exactly so that the HIP kernels (zl_stretch.hip) and a host build of the same text
// (tests/cpu_harness/stretch_host.cpp) give the same bits.  Parity with tracktion's time-stretcher is not claimed.
//
//   r = 2^(pitch/12), tau = speed / r (double, host); output N = max(1, floor(len / speed)) frames at the source's rate
//   stretch (tau != 1):  x[k*(S-O) + i] = in[b_k + i], cross-faded over i < O from mid[i] = in[b_{k-1} + S-O + i] (k > 0);
//                        b_k = floor(k * (tau*(S-O))) + off_k, off_k = argmax over o in [0, W) of the integer correlation
//                        score against mid (zl_st_score; ties: the smallest o); x has N1 = floor(len / tau) frames
//   resample (pitch != 0): y[j] = x[i]*(1-a) + x[i+1]*a, p = j*r, i = floor(p), a = (float)(p - i); x is 0 beyond N1
//   gain (gain_db != 0): y[j] * (float)10^(gain_db/20)
// Every float operation is one rounded fp32 operation (built with -ffp-contract=off on both sides); the seek is exact integer
// arithmetic up to one correctly rounded double division and square root per candidate.
#pragma once
#include <math.h>
#include <stdint.h>

#include "zl_types.h"

// Valid parameter ranges (zlhip_sound_rerender rejects values outside them; the libzl setters clamp to them)
#define ZL_ST_SPEED_MIN   0.25f
#define ZL_ST_SPEED_MAX   4.0f
#define ZL_ST_PITCH_MIN  -24.0f
#define ZL_ST_PITCH_MAX   24.0f

// SoundTouch 2.x's automatic TDStretch settings as restated here -- unpinned (SoundTouch is not available to check them against):
// overlap 8 ms (16 .. 512 frames, a multiple of 8); sequence 90 ms at tau <= 0.5 falling linearly to 40 ms at tau >= 2;
// seek window 20 ms falling to 15 ms over the same range.
#define ZL_ST_OVERLAP_SEC     0.008
#define ZL_ST_OVERLAP_MIN     16
#define ZL_ST_OVERLAP_MAX     512
#define ZL_ST_SEQ_MS_AT_LO    90.0
#define ZL_ST_SEQ_MS_AT_HI    40.0
#define ZL_ST_SEEK_MS_AT_LO   20.0
#define ZL_ST_SEEK_MS_AT_HI   15.0
#define ZL_ST_TAU_LO          0.5
#define ZL_ST_TAU_SPAN        1.5
// seek quantisation: q(v) = clamp(rint(v * 4096), -32767, 32767), NaN -> 0
#define ZL_ST_Q_SCALE         4096.0f
#define ZL_ST_Q_MAX           32767
// the seek kernel stages W + O quantised frames per channel in LDS: renders whose window is longer (sample rates above ~200 kHz)
// are rejected
#define ZL_ST_MAX_WINDOW      4608
// zero frames behind every source and render in the arena (zlhip_sound_upload's layout)
#define ZL_ST_PAD             8

// Everything a render needs besides the samples, computed once on the host (zl_st_geometry)
struct ZlStretchGeom {
    double  r;                   // resample step 2^(pitch/12)
    double  tau;                 // stretch factor speed / r (input frames per output frame of x)
    double  seg_step;            // tau * (S - O): nominal input advance per segment
    int64_t len;                 // source frames
    int64_t N1;                  // frames of the stretched signal x (len when the stretch does not run)
    int64_t N;                   // output frames
    float   g;                   // linear gain
    int32_t stretch, resample, gain;   // which stages run
    int32_t O, S, W;             // overlap, sequence, seek window (frames)
    int32_t nseg;                // segments of the stretch (0 when it does not run)
};

ZL_HD inline double zl_st_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 0 = valid (g filled), -1 = a parameter out of range or a source the stretch cannot take (sample rate too low or too high)
inline int zl_st_geometry(double sr, int64_t len, float gain_db, float pitch, float speed, ZlStretchGeom *g)
{
    if (!(speed >= ZL_ST_SPEED_MIN && speed <= ZL_ST_SPEED_MAX) || !(pitch >= ZL_ST_PITCH_MIN && pitch <= ZL_ST_PITCH_MAX)
        || !isfinite(gain_db) || len < 1 || !(sr > 0.0))
        return -1;
    g->len = len;
    g->r = pow(2.0, (double)pitch / 12.0);
    g->tau = (double)speed / g->r;
    g->N = (int64_t)floor((double)len / (double)speed);
    if (g->N < 1) g->N = 1;
    g->stretch = g->tau != 1.0;
    g->resample = pitch != 0.0f;
    g->gain = gain_db != 0.0f;
    g->g = (float)pow(10.0, (double)gain_db / 20.0);
    int64_t O = (int64_t)floor(sr * ZL_ST_OVERLAP_SEC);
    O = O < ZL_ST_OVERLAP_MIN ? ZL_ST_OVERLAP_MIN : (O > ZL_ST_OVERLAP_MAX ? ZL_ST_OVERLAP_MAX : O);
    g->O = (int32_t)(O & ~(int64_t)7);
    const double seq_ms = zl_st_clamp(ZL_ST_SEQ_MS_AT_LO + (ZL_ST_SEQ_MS_AT_HI - ZL_ST_SEQ_MS_AT_LO) / ZL_ST_TAU_SPAN * (g->tau - ZL_ST_TAU_LO),
                                      ZL_ST_SEQ_MS_AT_HI, ZL_ST_SEQ_MS_AT_LO);
    const double seek_ms = zl_st_clamp(ZL_ST_SEEK_MS_AT_LO + (ZL_ST_SEEK_MS_AT_HI - ZL_ST_SEEK_MS_AT_LO) / ZL_ST_TAU_SPAN * (g->tau - ZL_ST_TAU_LO),
                                       ZL_ST_SEEK_MS_AT_HI, ZL_ST_SEEK_MS_AT_LO);
    const double S = floor(sr * seq_ms / 1000.0), W = floor(sr * seek_ms / 1000.0);
    g->S = S < 2e9 ? (int32_t)S : 2000000000;
    g->W = W < 2e9 ? (int32_t)W : 2000000000;
    g->seg_step = g->tau * (double)(g->S - g->O);
    g->N1 = g->stretch ? (int64_t)floor((double)len / g->tau) : len;
    g->nseg = 0;
    if (g->stretch) {
        if (g->S <= g->O || g->W < 1 || (int64_t)g->W + g->O > ZL_ST_MAX_WINDOW) return -1;
        const int64_t L = g->S - g->O, n = (g->N1 + L - 1) / L;
        if (n > 0x7fffffff) return -1;
        g->nseg = (int32_t)n;
    }
    if (g->N + ZL_ST_PAD > 0x7fffffff || g->N1 > ((int64_t)1 << 40)) return -1;
    return 0;
}

ZL_HD inline bool zl_st_identity(float gain_db, float pitch, float speed) { return gain_db == 0.0f && pitch == 0.0f && speed == 1.0f; }

// seek quantisation (rintf: round half to even in the default rounding mode, v_rndne_f32 on the device)
ZL_HD inline int32_t zl_st_q(float v)
{
    if (v != v) return 0;
    const float t = rintf(v * ZL_ST_Q_SCALE);
    if (t > (float)ZL_ST_Q_MAX) return ZL_ST_Q_MAX;
    if (t < -(float)ZL_ST_Q_MAX) return -ZL_ST_Q_MAX;
    return (int32_t)t;
}

// weighted reference: (q(mid_i) * i*(O-i)) >> 16, int64, arithmetic shift.  |ref| <= 32767 (i*(O-i) <= O*O/4 <= 65536), so every
// product ref * q below fits int32, and so does the sum of two of them
ZL_HD inline int32_t zl_st_ref(int32_t qmid, int32_t i, int32_t O)
{
    return (int32_t)(((int64_t)qmid * (int64_t)(i * (O - i))) >> 16);
}

ZL_HD inline double zl_st_score(int64_t corr, int64_t norm)
{
    return norm == 0 ? 0.0 : (double)corr / sqrt((double)norm);
}

// argmax order: the higher score, then the smaller offset
ZL_HD inline bool zl_st_better(double s, int32_t o, double bs, int32_t bo)
{
    return s > bs || (s == bs && o < bo);
}

ZL_HD inline int64_t zl_st_base(const ZlStretchGeom &g, int64_t k)
{
    return (int64_t)floor((double)k * g.seg_step);
}

ZL_HD inline float zl_st_xfade(float mid, float v, int64_t i, int32_t O)
{
    const float w = (float)i / (float)O;
    return mid * (1.0f - w) + v * w;
}

// x[n], one channel.  in(n, c): the source frame n of channel c, 0 at n >= len.  off: the segments' seek offsets
template <class In>
ZL_HD inline float zl_st_x(const ZlStretchGeom &g, const int32_t *off, int64_t n, int c, const In &in)
{
    if (n >= g.N1) return 0.0f;
    if (!g.stretch) return in(n, c);
    const int64_t L = g.S - g.O, k = n / L, i = n - k * L;
    const float v = in(zl_st_base(g, k) + off[k] + i, c);
    if (i < g.O && k > 0) return zl_st_xfade(in(zl_st_base(g, k - 1) + off[k - 1] + L + i, c), v, i, g.O);
    return v;
}

// output frame j < N, one channel
template <class In>
ZL_HD inline float zl_st_y(const ZlStretchGeom &g, const int32_t *off, int64_t j, int c, const In &in)
{
    float y;
    if (g.resample) {
        const double p = (double)j * g.r;
        const int64_t i = (int64_t)floor(p);
        const float a = (float)(p - (double)i);
        y = zl_st_x(g, off, i, c, in) * (1.0f - a) + zl_st_x(g, off, i + 1, c, in) * a;
    } else {
        y = zl_st_x(g, off, j, c, in);
    }
    if (g.gain) y = y * g.g;
    return y;
}

// One clip of a zlhip_sound_rerender_batch call as the kernels see it
struct ZlStretchJob {
    ZlStretchGeom geom;
    uint64_t src;                // device address of the original upload (interleaved, channels per frame)
    uint64_t dst;                // device address of the new extent: (N + ZL_ST_PAD) * channels floats
    int64_t  off_base;           // the clip's first seek offset in the call's offset buffer
    int32_t  channels;
    int32_t  pad;
};

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
// launchers (zl_stretch.hip; 0 or a hipError_t value).  seek_jobs: indices of the jobs whose stretch stage runs
int zl_launch_stretch_seek(const ZlStretchJob *jobs, const int32_t *seek_jobs, int nseek, int32_t *offsets, hipStream_t s);
int zl_launch_stretch_synth(const ZlStretchJob *jobs, int njobs, int64_t max_frames, const int32_t *offsets, hipStream_t s);
#endif
