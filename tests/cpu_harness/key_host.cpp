// Host build of the key detection's definition (libzl_amd/csrc/zl_key.h) for the CPU tier -- TEST HARNESS ONLY.
// zlky_call walks a call the way the kernels do, with the header's own arithmetic: the gate frame by frame over the 16-byte groups of
// the arena's layout masked by float index, the correlate launch work item by work item (the request by bisection over item_base, the
// paired table, the group's widest window staged in chunks of ZL_KY_CHUNK samples, 32 lanes per bin striding j with phases advanced by
// addition modulo 2^32, the lanes' sums merged in another order), the fold with a lane per bin.  It counts every term, refuses -- and
// counts -- any float outside a request's frames and any staged sample outside the chunk, and holds every (frame, bin) to the header's
// one-thread form over T itself (zl_ky_bin_serial) and the fold to zl_ky_fold_serial.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "zl_key.h"
#include "zlhip.h"

namespace {

const int kThreads = ZL_KY_ITEM_BINS * ZL_KY_BIN_LANES;

struct Walk { int64_t terms = 0, refused = 0, staged_wrong = 0, disagree = 0; };

int32_t find(const ZlKyRequest *reqs, int32_t nreq, int32_t at, bool items)
{
    for (int32_t lo = 0, hi = nreq - 1; ; ) {
        if (lo >= hi) return lo;
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((items ? reqs[mid].item_base : reqs[mid].frame_base) <= at) lo = mid; else hi = mid - 1;
    }
}

// the mixed samples [lo, hi) of the sound (frames), the way a kernel reads them: whole 16-byte groups, the elements outside masked
// and never looked at.  out[i]: sample lo + i.  r_lo, r_hi: the floats of the request's frames
void mix_span(const ZlKyRequest &R, int64_t lo, int64_t hi, int64_t r_lo, int64_t r_hi, int32_t *out, int32_t capacity, Walk &w)
{
    int64_t f0, f1, g0, g1;
    zl_ov_groups(lo, hi, R.channels, &f0, &f1, &g0, &g1);
    const int32_t head = (int32_t)(f0 - 4 * g0), count = (int32_t)(f1 - f0), ngroups = (int32_t)(g1 - g0);
    const float *src = (const float *)(uintptr_t)R.src + 4 * g0;
    for (int32_t g = ngroups - 1; g >= 0; --g) {
        float v[4];
        for (int j = 0; j < 4; ++j) {
            const uint32_t nan = 0x7fc00000u;
            std::memcpy(&v[j], &nan, 4);
            if (!zl_ov_valid(g, j, head, count)) continue;
            const int64_t at = 4 * (g0 + g) + j;
            if (at < r_lo || at >= r_hi) { ++w.refused; continue; }
            v[j] = src[4 * g + j];
        }
        int32_t m[4], idx[4];
        zl_pt_group_mix(v[0], v[1], v[2], v[3], g, head, count, R.channels, m, idx);
        for (int j = 0; j < 4; ++j) {
            if (idx[j] < 0) continue;
            if (idx[j] >= capacity) { ++w.staged_wrong; continue; }
            out[idx[j]] = m[j];
        }
    }
}

void gate_frame(const ZlKyRequest &R, int32_t k, int64_t r_lo, int64_t r_hi, ZlKyStat *st, Walk &w)
{
    std::vector<int32_t> m((size_t)R.span, 0);
    const int64_t s0 = zl_ky_frame_start(R, k);
    mix_span(R, s0, s0 + R.span, r_lo, r_hi, m.data(), R.span, w);
    uint64_t e = 0;
    for (int32_t i = R.span - 1; i >= 0; --i) e += (uint64_t)((int64_t)m[(size_t)i] * m[(size_t)i]);
    st->energy = e; st->silent = e < R.floor_ ? 1 : 0; st->reserved = 0;
}

void correlate_item(const ZlKyRequest *reqs, int32_t nreq, int32_t item, const ZlKyBin *bins, const int16_t *T, const ZlKyStat *stat, ZlKyAcc *acc,
                    const int64_t *r_lo, const int64_t *r_hi, Walk &w)
{
    const int32_t r = find(reqs, nreq, item, true);
    const ZlKyRequest &R = reqs[r];
    int32_t frame, group;
    zl_ky_item_of(R, item - R.item_base, &frame, &group);
    ZlKyAcc *const dst = acc + R.acc_base + (int64_t)frame * R.nbins;
    const int32_t b0 = group * ZL_KY_ITEM_BINS;
    if (stat[R.frame_base + frame].silent) {
        for (int32_t b = b0; b < std::min(b0 + ZL_KY_ITEM_BINS, R.nbins); ++b) { dst[b].re = 0; dst[b].im = 0; }
        return;
    }
    std::vector<uint32_t> P((size_t)ZL_KY_TABLE);
    for (int32_t i = 0; i < ZL_KY_TABLE; ++i) P[(size_t)i] = zl_ky_pair(T, i);
    const ZlKyBin wide = bins[R.bin_base + b0];
    const int32_t w0 = zl_ky_bin_off(R, wide), w1 = w0 + wide.n;
    const int64_t s0 = zl_ky_frame_start(R, frame);
    std::vector<int64_t> re((size_t)kThreads, 0), im((size_t)kThreads, 0);
    std::vector<int32_t> sM((size_t)ZL_KY_CHUNK);
    for (int32_t c0 = w0; c0 < w1; c0 += ZL_KY_CHUNK) {
        const int32_t c1 = std::min(c0 + ZL_KY_CHUNK, w1);
        std::fill(sM.begin(), sM.end(), INT32_MIN);                // (a sample that was not staged shows in the sums)
        mix_span(R, s0 + c0, s0 + c1, r_lo[r], r_hi[r], sM.data(), c1 - c0, w);
        for (int tid = kThreads - 1; tid >= 0; --tid) {
            const int32_t b = b0 + tid / ZL_KY_BIN_LANES, lane = tid & (ZL_KY_BIN_LANES - 1);
            if (b >= R.nbins) continue;
            const ZlKyBin B = bins[R.bin_base + b];
            const int32_t off = zl_ky_bin_off(R, B);
            int32_t j0, j1;
            zl_ky_lane_range(off, B.n, c0, c1, lane, &j0, &j1);
            uint32_t ph = (uint32_t)j0 * B.step, wph = (uint32_t)j0 * B.wstep;
            const uint32_t dstep = B.step * (uint32_t)ZL_KY_BIN_LANES, dwstep = B.wstep * (uint32_t)ZL_KY_BIN_LANES;
            for (int32_t j = j0; j < j1; j += ZL_KY_BIN_LANES) {
                const int32_t at = j + off - c0;
                if (at < 0 || at >= c1 - c0 || (j & (ZL_KY_BIN_LANES - 1)) != lane) { ++w.staged_wrong; continue; }
                if (ph >> 20 != zl_ky_index(B.step, j) || wph >> 20 != zl_ky_index(B.wstep, j)) ++w.disagree;      // the added phase is the multiplied one
                zl_ky_term(P.data(), B, j, sM[(size_t)at], &re[(size_t)tid], &im[(size_t)tid]);
                ++w.terms;
                ph += dstep; wph += dwstep;
            }
        }
    }
    std::vector<int32_t> m((size_t)R.span, 0);
    Walk scratch;
    mix_span(R, s0, s0 + R.span, r_lo[r], r_hi[r], m.data(), R.span, scratch);
    for (int32_t b = b0; b < std::min(b0 + ZL_KY_ITEM_BINS, R.nbins); ++b) {
        ZlKyAcc a; a.re = 0; a.im = 0;
        for (int lane = ZL_KY_BIN_LANES - 1; lane >= 0; --lane) { a.re += re[(size_t)((b - b0) * ZL_KY_BIN_LANES + lane)]; a.im += im[(size_t)((b - b0) * ZL_KY_BIN_LANES + lane)]; }
        dst[b] = a;
        int64_t sr, si;
        const ZlKyBin B = bins[R.bin_base + b];
        zl_ky_bin_serial(T, B, m.data(), zl_ky_bin_off(R, B), &sr, &si);
        if (sr != a.re || si != a.im) ++w.disagree;
    }
}

// the fold of one request the way the workgroup does it: a lane per bin, twelve lanes for the chroma
void fold_walk(const ZlKyRequest &R, const ZlKyBin *bins, const ZlKyStat *stat, const ZlKyAcc *acc, uint64_t *totals, ZlKyResult *out, Walk &w)
{
    ZlKyResult o;
    std::memset(&o, 0, sizeof(o));
    o.frames = R.frames;
    for (int32_t b = R.nbins - 1; b >= 0; --b) {
        uint64_t t = 0;
        for (int32_t k = R.frames - 1; k >= 0; --k)
            if (!stat[k].silent) t += zl_ky_counted(acc[(int64_t)k * R.nbins + b].re, acc[(int64_t)k * R.nbins + b].im, bins[b].n, R.span, stat[k].energy);
        totals[b] = t;
    }
    for (int p = 11; p >= 0; --p) for (int32_t b = 0; b < R.nbins; ++b) if (bins[b].note % 12 == p) o.chroma[p] += totals[b];
    for (int32_t k = 0; k < R.frames; ++k) o.sounding += stat[k].silent ? 0 : 1;
    std::vector<uint64_t> B((size_t)R.nbins);
    ZlKyResult serial;
    zl_ky_fold_serial(R, bins, stat, acc, B.data(), &serial);
    if (std::memcmp(&serial, &o, sizeof(o)) != 0 || std::memcmp(B.data(), totals, B.size() * sizeof(uint64_t)) != 0) ++w.disagree;
    *out = o;
}

}  // namespace

extern "C" {

void zlky_sizes(int32_t *out) { out[0] = (int32_t)sizeof(ZlKyResult); out[1] = (int32_t)sizeof(ZlKyBin); out[2] = (int32_t)sizeof(ZlKyRequest); out[3] = (int32_t)sizeof(ZlKyAcc); }
int32_t zlky_match_shift(int32_t clip_tonic, int32_t clip_mode, int32_t tonic, int32_t mode) { return zl_ky_match_shift(clip_tonic, clip_mode, tonic, mode); }

// the finish over a hand-made integer record
void zlky_finish(const uint64_t *chroma, int32_t frames, int32_t sounding, ZlKyResult *out)
{
    std::memset(out, 0, sizeof(*out));
    out->frames = frames; out->sounding = sounding;
    std::memcpy(out->chroma, chroma, sizeof(out->chroma));
    zl_ky_finish(out);
}

// A call of nreq requests.  reqs[i].id is ignored: request i reads data[i], the sound in the arena's layout ([L0 R0 L1 R1] / [x0 x1 ..],
// length[i] frames, padded with zeros to a whole 16-byte group), channels[i], rate[i].  acc [acc_capacity] pairs, totals and bins
// [bin_capacity], silent [frame_capacity], geom [nreq][8] = (L, K, hop, nbins, items, frame_base, bin_base, groups), acc_base [nreq],
// out [nreq] results (finished), walk [4] = (terms entered, floats refused, samples staged or read outside a chunk, walks that
// disagree with the one-thread forms).  Returns the pairs used; -1: a capacity is too small; -2: a request is outside its limits.
int64_t zlky_call(int32_t nreq, const zlhip_key_request *reqs, const float *const *data, const int32_t *length, const int32_t *channels, const double *rate, ZlKyAcc *acc,
                  int64_t acc_capacity, uint64_t *totals, ZlKyBin *bins, int64_t bin_capacity, int32_t *silent, int64_t frame_capacity, int32_t *geom, int64_t *acc_base,
                  ZlKyResult *out, int64_t *walk)
{
    std::vector<ZlKyRequest> R((size_t)nreq);
    std::vector<int64_t> lo((size_t)nreq), hi((size_t)nreq);
    std::vector<int16_t> T((size_t)ZL_KY_TABLE);
    zl_ky_design(1.0, 0.0f, 1, 0, 0, nullptr, T.data());
    int64_t nf = 0, pairs = 0, items = 0, nb = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_key_request q = reqs[i];
        ZlKyRequest &X = R[(size_t)i];
        if (q.first_frame < 0 || q.num_frames < 1 || (int64_t)q.first_frame + q.num_frames > length[i]) return -2;
        if (zl_ky_resolve(rate[i], &q.hop, &q.max_frames, &q.a4_hz, &q.note_lo, &q.note_hi, &q.q, &q.gate) != 0) return -2;
        X.nbins = q.note_hi - q.note_lo + 1; X.bin_base = (int32_t)nb;
        if (nb + X.nbins > bin_capacity) return -1;
        zl_ky_design(rate[i], q.a4_hz, q.note_lo, q.note_hi, q.q, bins + nb, nullptr);
        X.src = (uint64_t)(uintptr_t)data[i];
        X.span = bins[nb].n;
        X.floor_ = (uint64_t)X.span * (uint64_t)channels[i] * (uint64_t)q.gate * (uint64_t)q.gate;
        X.first = q.first_frame; X.channels = channels[i]; X.reserved = 0;
        zl_ky_frames(q.num_frames, X.span, q.hop, q.max_frames, &X.frames, &X.hop);
        X.acc_base = pairs; X.frame_base = (int32_t)nf; X.item_base = (int32_t)items;
        lo[(size_t)i] = (int64_t)q.first_frame * channels[i];
        hi[(size_t)i] = ((int64_t)q.first_frame + q.num_frames) * channels[i];
        const int32_t g[8] = {X.span, X.frames, X.hop, X.nbins, zl_ky_items(X), X.frame_base, X.bin_base, zl_ky_groups(X)};
        std::memcpy(geom + 8 * i, g, sizeof(g));
        acc_base[i] = pairs;
        nb += X.nbins; nf += X.frames; pairs += (int64_t)X.frames * X.nbins; items += zl_ky_items(X);
    }
    if (pairs > acc_capacity || nf > frame_capacity || nf > ZL_KY_MAX_CALL_FRAMES) return -1;
    std::vector<ZlKyStat> stat((size_t)nf);
    Walk w;
    for (int64_t f = nf - 1; f >= 0; --f) {
        const int32_t r = find(R.data(), nreq, (int32_t)f, false);
        gate_frame(R[(size_t)r], (int32_t)(f - R[(size_t)r].frame_base), lo[(size_t)r], hi[(size_t)r], &stat[(size_t)f], w);
        silent[f] = stat[(size_t)f].silent;
    }
    for (int64_t it = items - 1; it >= 0; --it) correlate_item(R.data(), nreq, (int32_t)it, bins, T.data(), stat.data(), acc, lo.data(), hi.data(), w);
    for (int32_t i = 0; i < nreq; ++i) {
        const ZlKyRequest &X = R[(size_t)i];
        fold_walk(X, bins + X.bin_base, stat.data() + X.frame_base, acc + X.acc_base, totals + X.bin_base, &out[i], w);
        zl_ky_finish(&out[i]);
    }
    walk[0] = w.terms; walk[1] = w.refused; walk[2] = w.staged_wrong; walk[3] = w.disagree;
    return pairs;
}

}
