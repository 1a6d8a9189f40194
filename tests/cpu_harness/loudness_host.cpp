// Host build of the loudness measurement (libzl_amd/csrc/zl_loudness.h) for the CPU tier: a call is walked as zl_k_loudness walks it --
// the items numbered over the call, ZL_LD_GROUP items per group, a lane per item, every lane of a group stepping to the group's largest
// number of steps (zl_ld_group_steps) and idling past its own (zl_ld_item_steps) -- with the same header code per step.  The walk counts
// what it touches: every frame a request sums must be summed exactly once, and no float outside a request is ever read (an element
// the mask keeps out is never fetched: the step gets a poison value in its place, which would show in the sums and the peak).
//   zlld_call    a whole call: records, results, counts
//   zlld_bank    the host route of scripts/loudness_bench.py: planar clips, interleaved and measured item by item on `threads` threads
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "zl_loudness.h"
#include "zlhip.h"

static_assert(sizeof(zlhip_loudness) == sizeof(ZlLdResult) && sizeof(zlhip_loudness_sub) == sizeof(ZlLdSub), "the ABI's layouts");

// the request as the kernel sees it (src stays 0: the harness reads through `data`); 0 = valid, -1 = not
static int geometry(const zlhip_loudness_request &q, double rate, int32_t length, int32_t channels, int32_t item_base, ZlLdRequest *R)
{
    int32_t sub = q.sub_frames;
    if (zl_ld_resolve(rate, q.first_frame, q.num_frames, &sub) != 0 || zl_ld_design(rate, R->c) != 0) return -1;
    if ((int64_t)q.first_frame + q.num_frames > length) return -1;
    R->src = 0; R->first = q.first_frame; R->frames = q.num_frames; R->sub = sub; R->channels = channels;
    R->items = (int32_t)zl_ld_items(q.num_frames, sub); R->item_base = item_base;
    return 0;
}

extern "C" {

int zlld_design(double rate, double *c) { return zl_ld_design(rate, c); }
int zlld_resolve(double rate, int32_t first, int32_t num, int32_t *sub) { return zl_ld_resolve(rate, first, num, sub); }
int64_t zlld_items(int64_t num, int32_t sub) { return zl_ld_items(num, sub); }
void zlld_finish(const ZlLdSub *subs, int32_t num, int32_t sub, ZlLdResult *out) { zl_ld_finish(subs, num, sub, out); }

// data[i]: request i's sound in the arena's layout (interleaved), exactly length[i] * channels[i] floats.  subs: [capacity] records,
// item_base: [nreq], out: [nreq].  walk: [0] samples summed, [1] frames of a request not summed exactly once, [2] elements outside a
// request that the mask let through, [3] lanes that did not run exactly their own steps, [4] idle lane-steps, [5] groups.
// Returns the call's items, or -1 for an invalid call (nothing is written then), -2 where capacity is too small.
int64_t zlld_call(int32_t nreq, const zlhip_loudness_request *reqs, const float *const *data, const int32_t *length, const int32_t *channels, const double *rate,
                  ZlLdSub *subs, int64_t capacity, int32_t *item_base, ZlLdResult *out, int64_t *walk)
{
    if (nreq < 0) return -1;
    std::vector<ZlLdRequest> R((size_t)nreq);
    int64_t items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        if (geometry(reqs[i], rate[i], length[i], channels[i], (int32_t)items, &R[(size_t)i]) != 0) return -1;
        items += R[(size_t)i].items;
        if (items > ZL_LD_MAX_CALL_ITEMS) return -1;
    }
    if (items > capacity) return -2;
    std::vector<std::vector<uint8_t>> summed((size_t)nreq);
    for (int32_t i = 0; i < nreq; ++i) summed[(size_t)i].assign((size_t)R[(size_t)i].frames, 0);
    int64_t w[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t poison = 0x7149f2cau;                           // 1e30f
    const int32_t groups = (int32_t)((items + ZL_LD_GROUP - 1) / ZL_LD_GROUP);
    for (int32_t g = 0; g < groups; ++g) {
        const int32_t gsteps = zl_ld_group_steps(R.data(), nreq, (int32_t)items, g);
        ZlLdAcc acc[ZL_LD_GROUP]; ZlLdItem I[ZL_LD_GROUP]; int32_t req[ZL_LD_GROUP], ran[ZL_LD_GROUP];
        for (int l = 0; l < ZL_LD_GROUP; ++l) {
            const int32_t item = g * ZL_LD_GROUP + l;
            zl_ld_acc_init(acc[l]); ran[l] = 0; req[l] = -1;
            if (item >= items) continue;
            req[l] = zl_ld_find(R.data(), nreq, item);
            I[l] = zl_ld_item(R[(size_t)req[l]], item - R[(size_t)req[l]].item_base);
        }
        for (int32_t n = 0; n < gsteps; ++n)
            for (int l = 0; l < ZL_LD_GROUP; ++l) {
                const int32_t item = g * ZL_LD_GROUP + l;
                if (n >= zl_ld_item_steps(R.data(), nreq, (int32_t)items, item)) { ++w[4]; continue; }
                const ZlLdRequest &Q = R[(size_t)req[l]];
                const int64_t lo = (int64_t)Q.first * Q.channels, hi = ((int64_t)Q.first + Q.frames) * Q.channels;
                uint32_t v[4];
                for (int j = 0; j < 4; ++j) {
                    const int64_t f = 4 * (I[l].g0 + n) + j;       // the element's float index in the sound
                    const bool inside = f >= lo && f < hi;
                    v[j] = poison;
                    if (inside) memcpy(&v[j], data[req[l]] + f, 4);
                    if (!inside && zl_ov_valid(n, j, I[l].head, I[l].count)) ++w[2];
                    // what the step sums: the element's frame, relative to w, in [own, end)
                    const int32_t rel = (4 * n + j - I[l].head) / Q.channels;
                    if (zl_ov_valid(n, j, I[l].head, I[l].count) && rel >= I[l].own && rel < I[l].end) {
                        ++w[0];
                        if (j % Q.channels == 0 || Q.channels == 1) {
                            int64_t fw, s0, s1, pe;
                            zl_ld_item_frames(Q, item - Q.item_base, &fw, &s0, &s1, &pe);
                            ++summed[(size_t)req[l]][(size_t)(fw + rel - Q.first)];
                        }
                    }
                }
                if (Q.channels == 2) zl_ld_step<2>(Q.c, I[l], n, v[0], v[1], v[2], v[3], acc[l]); else zl_ld_step<1>(Q.c, I[l], n, v[0], v[1], v[2], v[3], acc[l]);
                ++ran[l];
            }
        for (int l = 0; l < ZL_LD_GROUP; ++l) {
            const int32_t item = g * ZL_LD_GROUP + l;
            if (item >= items) { if (ran[l] != 0) ++w[3]; continue; }
            if (ran[l] != I[l].steps) ++w[3];
            subs[item] = zl_ld_record(acc[l]);
        }
        ++w[5];
    }
    for (int32_t i = 0; i < nreq; ++i) {
        const ZlLdRequest &Q = R[(size_t)i];
        const int64_t S = zl_ld_whole(Q.frames, Q.sub), covered = S >= 4 ? S * Q.sub : Q.frames;
        for (int64_t f = 0; f < Q.frames; ++f) if (summed[(size_t)i][(size_t)f] != (f < covered ? 1 : 0)) ++w[1];
        item_base[i] = Q.item_base;
        zl_ld_finish(subs + Q.item_base, Q.frames, Q.sub, &out[i]);
    }
    if (walk) memcpy(walk, w, sizeof(w));
    return items;
}

// The host route: clip i is planar (L[i], R[i] or NULL), length[i] frames at rate[i]; the whole clip with the default sub-block.
// base: [nclips] first record of clip i in subs ([capacity]).  Returns the records written, or -1 / -2 as zlld_call.
int64_t zlld_bank(int32_t nclips, const float *const *L, const float *const *Rp, const int32_t *length, const double *rate, int32_t threads,
                  ZlLdSub *subs, int64_t capacity, int64_t *base, ZlLdResult *out)
{
    std::vector<ZlLdRequest> R((size_t)nclips);
    int64_t items = 0;
    for (int32_t i = 0; i < nclips; ++i) {
        const zlhip_loudness_request q = {i, 0, length[i], 0};
        if (geometry(q, rate[i], length[i], Rp[i] ? 2 : 1, 0, &R[(size_t)i]) != 0) return -1;
        base[i] = items; items += R[(size_t)i].items;
    }
    if (items > capacity) return -2;
    auto work = [&](int32_t t) {
        std::vector<uint32_t> buf;
        for (int32_t i = t; i < nclips; i += threads) {
            const ZlLdRequest &Q = R[(size_t)i];
            const size_t floats = ((size_t)length[i] * (size_t)Q.channels + 3) / 4 * 4;
            buf.assign(floats, 0u);
            for (int32_t f = 0; f < length[i]; ++f) {
                if (Q.channels == 2) { memcpy(&buf[2 * (size_t)f], L[i] + f, 4); memcpy(&buf[2 * (size_t)f + 1], Rp[i] + f, 4); }
                else memcpy(&buf[(size_t)f], L[i] + f, 4);
            }
            for (int32_t k = 0; k < Q.items; ++k) zl_ld_item_serial(Q, k, buf.data(), &subs[base[i] + k]);
            zl_ld_finish(subs + base[i], Q.frames, Q.sub, &out[i]);
        }
    };
    std::vector<std::thread> pool;
    for (int32_t t = 1; t < threads; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    return items;
}

}  // extern "C"
