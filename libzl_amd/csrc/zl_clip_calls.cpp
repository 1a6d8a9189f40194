// zl_clip_calls.cpp -- the clip services of include/zlhip.h: loading from raw PCM, re-render, rate conversion, and the seven analyses
// (waveform overviews, transients, tempo, pitch, loudness, loop points, key), the loop crossfade, the clip edit and the warp.  Every one is a call on a loaded clip that validates everything before its
// first HIP call, reserves buffers that only grow, queues its launches on the engine's stream and waits once.  What they share is
// written once, below: the checks and the buffers of every service, and for the six that replace a clip's data -- the PCM upload, the
// re-render, the rate conversion, the loop crossfade, the clip edit, the warp -- the new arena extents of a call, taken all or none (ZlNewExtents), and
// the switch of a clip to its new extent (ZlClipSwap).  The engine itself -- arena, sound slots, rendering, the resident kernel -- is
// zl_engine.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>

#include "zl_engine_impl.h"
#include "zl_decode.h"
#include "zl_edit.h"
#include "zl_key.h"
#include "zl_limit.h"
#include "zl_loop.h"
#include "zl_loudness.h"
#include "zl_onset.h"
#include "zl_overview.h"
#include "zl_pitch.h"
#include "zl_resample.h"
#include "zl_stretch.h"
#include "zl_tempo.h"
#include "zl_warp.h"
#include "zl_xfade.h"

// ---- what every service does ---------------------------------------------------------------------------------------------------
static int fail_in(zlhip_engine *e, int code, const char *svc, const char *msg) { return fail(e, code, (std::string(svc) + ": " + msg).c_str()); }

static int check_sound(zlhip_engine *e, const char *svc, int32_t id)
{
    return id < 0 || id >= e->cfg.max_sounds || !e->hc.soundUsed[id] ? fail_in(e, ZLHIP_ERR_INVALID, svc, "no such sound") : ZLHIP_OK;
}

// An analysis request: its sound exists, its fields are inside their limits (`resolve` fills the defaults in and returns what is wrong,
// or nullptr), its window lies inside the data the sound plays.  In that order, before the first HIP call.
template <typename Q, typename Resolve> static int check_request(zlhip_engine *e, const char *svc, Q &q, Resolve resolve)
{
    { const int rc = check_sound(e, svc, q.id); if (rc != ZLHIP_OK) return rc; }
    const ZlSound &s = e->hc.sounds[q.id];
    if (const char *wrong = resolve(s)) return fail_in(e, ZLHIP_ERR_INVALID, svc, wrong);
    if (q.first_frame < 0 || q.num_frames < 1 || (int64_t)q.first_frame + q.num_frames > s.length)
        return fail_in(e, ZLHIP_ERR_INVALID, svc, "the frames do not lie inside the sound's playback data");
    return ZLHIP_OK;
}
static const char *const kOutsideLimits = "a field of the request is outside its limits";

// A call's buffers: `need` elements of `elem` bytes in scratch[buf], a too small one replaced by one of `new_cap` (grow_buf); where
// anything is replaced, a buffer is measured by `regrow` instead, if given.  And its results in mapped host memory.
struct ZlBufNeed { int buf; size_t need, elem, new_cap; bool twin; const char *what; size_t regrow = 0; };
struct ZlMapNeed { void *mapped; size_t cap, need; hipError_t (*grow)(void *, size_t); };
template <typename T> static ZlMapNeed mapped_need(ZlMapped<T> &m, size_t need) { return { &m, m.cap, need, [](void *p, size_t n) { return ((ZlMapped<T> *)p)->grow(n); } }; }
// hipMalloc, hipFree and hipHostFree wait for resident kernels, so the buffers are allocated by the first call and grow only: a call
// that fits them makes no device-synchronising HIP call.  One that does not stops this engine's kernel first (stop; a call that has
// stopped it already passes false) and has the others' step aside.
static int reserve(zlhip_engine *e, bool stop, std::initializer_list<ZlBufNeed> bufs, std::initializer_list<ZlMapNeed> maps = {})
{
    bool fits = true;
    for (const ZlBufNeed &b : bufs) fits = fits && b.need <= e->scratch[b.buf].cap;
    for (const ZlMapNeed &m : maps) fits = fits && m.need <= m.cap;
    if (fits) return ZLHIP_OK;
    if (stop) { int r_ = rt_stop(e); if (r_ != ZLHIP_OK) return r_; }
    ZlQuiesce quiet(e);
    for (const ZlBufNeed &b : bufs) {
        const int rc = grow_buf(e, e->scratch[b.buf], b.regrow ? b.regrow : b.need, b.elem, b.new_cap, b.twin, b.what);
        if (rc != ZLHIP_OK) return rc;
    }
    for (const ZlMapNeed &m : maps) ZL_HIP(e, m.grow(m.mapped, m.need));
    return ZLHIP_OK;
}

// ---- what the services that replace a clip's data do -------------------------------------------------------------------------
// No clip twice in a call.  Asked request by request, between a service's own checks: the first thing wrong with the first wrong
// request is what the caller reads.
struct ZlDistinct {
    std::vector<char> seen;
    explicit ZlDistinct(const zlhip_engine *e) : seen((size_t)e->cfg.max_sounds, 0) {}
    int check(zlhip_engine *e, const char *svc, int32_t id)
    {
        { const int rc = check_sound(e, svc, id); if (rc != ZLHIP_OK) return rc; }
        if (seen[(size_t)id]) return fail_in(e, ZLHIP_ERR_INVALID, (std::string(svc) + "_batch").c_str(), "a clip appears twice");
        seen[(size_t)id] = 1;
        return ZLHIP_OK;
    }
};

// A clip that plays a re-render keeps its original for the next one: a service that would replace the original refuses, with its own advice.
static int check_plays_original(zlhip_engine *e, int32_t id, const char *refusal)
{
    return e->soundSlots[(size_t)id].renderFloats != 0 ? fail(e, ZLHIP_ERR_STATE, refusal) : ZLHIP_OK;
}

// The new arena extents of a call, one per request that gets one, all or none: an arena that cannot hold the call keeps nothing of it
// and leaves every clip as it was; a segment the arena grew by goes back to the device (free_extent).  After call_begin(e, true).
struct ZlNewExtents {
    zlhip_engine *e;
    std::vector<size_t> off, floats;                               // per request; 0 floats: nothing taken
    std::function<void()> undo_first;                              // what else a failed call undoes, before its extents go back
    ZlNewExtents(zlhip_engine *e_, int32_t count) : e(e_), off((size_t)count, 0), floats((size_t)count, 0) {}
    int take(int32_t i, int64_t frames, int channels)
    {
        const size_t n = zl_extent_floats(frames, channels);
        const int rc = alloc_extent(e, n, &off[(size_t)i]);
        if (rc != ZLHIP_OK) { rollback(); return rc; }
        floats[(size_t)i] = n;
        return ZLHIP_OK;
    }
    void rollback()                                                // last taken first
    {
        if (undo_first) undo_first();
        for (size_t k = off.size(); k-- > 0;) { free_extent(e, off[k], floats[k]); floats[k] = 0; }
    }
    float *ptr(int32_t i) const { return arena_ptr(e, off[(size_t)i]); }
};

// The switch of a call's clips to their new extents, which become the slots' originals.  On the device zl_k_resample_publish switches
// the sound-table entries from one ZlRsPublish per job, ZL_SOUND_FINITE from the job's verdict word; `words` is what the words start
// as for a service that copies the original's samples -- set where the original lacks the flag, so that it stays without it.  The
// service reserves, copies and launches; this is what it fills while it adds its jobs, what a HIP error undoes, and the host's half
// behind the wait.
struct ZlClipSwap {
    zlhip_engine *e; const char *svc; ZlNewExtents &ext;
    std::vector<ZlRsPublish> pub; std::vector<uint32_t> words; std::vector<int32_t> jobReq;     // per job; jobReq: its request
    // request i's clip `id` will play `s`, its original with the length and rate the service gives it, from the request's extent.
    // Returns the job, which is the index of its verdict word as well.
    int32_t add(int32_t i, int32_t id, ZlSound s)
    {
        const int32_t j = (int32_t)pub.size();
        words.push_back((s.flags & ZL_SOUND_FINITE) ? 0u : 1u);
        s.offset = ext.off[(size_t)i]; s.flags &= ~(int32_t)ZL_SOUND_FINITE;
        pub.push_back(ZlRsPublish{ s, id, j });
        jobReq.push_back(i);
        return j;
    }
    int hip_failed(int krc)
    {
        e->err = std::string(svc) + ": " + hipGetErrorString((hipError_t)krc);
        (void)hipStreamSynchronize(e->stream);
        // (the table entries the device may have switched go back to what the host's mirror holds)
        for (const ZlRsPublish &p : pub) (void)hipMemcpy(e->dSounds + p.id, &e->hc.sounds[p.id], sizeof(ZlSound), hipMemcpyHostToDevice);
        ext.rollback();
        return ZLHIP_ERR_HIP;
    }
    // behind the call's last wait, with the verdict words read back: the new extent is the slot's original from now on, the old one
    // goes back to the arena.  per_job(job, slot): what a service keeps besides.
    template <typename PerJob> void commit(const std::vector<uint32_t> &verdicts, PerJob per_job)
    {
        e->outstanding = false;
        for (size_t j = 0; j < pub.size(); ++j) {
            const ZlRsPublish &p = pub[j];
            zlhip_engine::SoundSlot &slot = e->soundSlots[(size_t)p.id];
            const size_t oldOff = (size_t)slot.orig.offset, oldFloats = slot.floats;
            ZlSound s = p.s;
            if (verdicts[j] == 0u) s.flags |= ZL_SOUND_FINITE;
            slot.orig = s; slot.floats = ext.floats[(size_t)jobReq[j]];
            slot.renderOffsets.clear();
            per_job(j, slot);
            e->hc.sounds[p.id] = s;
            free_extent(e, oldOff, oldFloats);
        }
    }
    void commit(const std::vector<uint32_t> &verdicts) { commit(verdicts, [](size_t, zlhip_engine::SoundSlot &) {}); }
};

extern "C" {

// ---- clips from raw PCM (zl_decode.h, zl_decode.hip) ---------------------------------------------------------------------
// The other side of the file boundary: zlhip_bounce writes 16-bit PCM from the render kernel, this reads the bytes of a WAV `data`
// chunk.  The raw bytes cross the link (half of fp32 for 16-bit files, no host loop over the samples), one decode launch per staging
// pass writes the arena's layout, pad included, and the call waits for the device once -- whatever the number of clips.
// ZL_PCM_STAGE_BYTES: the size of the staging buffer, read per call (tests cut clips inside with a small one)
static uint32_t zl_pcm_stage_switch() { const char *v = std::getenv("ZL_PCM_STAGE_BYTES"); return zl_dec_stage_bytes(v ? std::atoll(v) : (long long)ZL_DEC_STAGE_DEFAULT); }

int zlhip_sound_upload_pcm_batch(zlhip_engine *e, const zlhip_pcm_source *srcs, int32_t count, int32_t *out_ids)
{
    if (!e || count < 0 || (count > 0 && (!srcs || !out_ids))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    for (int32_t i = 0; i < count; ++i) out_ids[i] = -1;
    // every argument before the first HIP call
    for (int32_t i = 0; i < count; ++i) {
        const zlhip_pcm_source &q = srcs[i];
        if (!q.frames) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: frames is NULL");
        if (q.format < ZLHIP_PCM_U8 || q.format > ZLHIP_PCM_F64) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: format outside 1 .. 6");
        if (q.channels < 1 || q.channels > ZLHIP_PCM_MAX_CHANNELS) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: channels outside 1 .. 64");
        if (q.length < 1) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: length below 1");
        if (!(q.sample_rate > 0.0)) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: sample rate not above 0");
        if (q.reserved != 0) return fail(e, ZLHIP_ERR_INVALID, "sound_upload_pcm: reserved is not 0");
    }
    // the slots: the first free ones in request order, as consecutive zlhip_sound_upload calls would take them
    std::vector<int32_t> ids;
    for (int i = 0; i < e->cfg.max_sounds && (int32_t)ids.size() < count; ++i) if (!e->hc.soundUsed[i]) ids.push_back(i);
    if ((int32_t)ids.size() < count) return fail(e, ZLHIP_ERR_CAPACITY, "sound_upload_pcm: too few free sound slots for the call");
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }     // (an extent freed earlier may be handed out again here)
    ZlNewExtents ext(e, count);                                    // the extents, all or none
    for (int32_t i = 0; i < count; ++i) { const int rc = ext.take(i, srcs[i].length, zl_dec_out_channels(srcs[i].channels)); if (rc != ZLHIP_OK) return rc; }
    // the cut into passes and pieces, the records
    const uint32_t stageBytes = zl_pcm_stage_switch();
    std::vector<ZlDecClip> clips((size_t)count);
    for (int32_t i = 0; i < count; ++i) clips[(size_t)i] = ZlDecClip{ srcs[i].length, srcs[i].channels, srcs[i].format };
    std::vector<ZlDecPiece> pieces; std::vector<ZlDecPass> passes;
    zl_dec_plan(clips.data(), count, stageBytes, pieces, passes);
    for (ZlDecPiece &R : pieces) R.dst = (uint64_t)(uintptr_t)ext.ptr(R.verdict);
    std::vector<ZlDecPublish> pub((size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        ZlSound s; s.offset = ext.off[(size_t)i]; s.length = srcs[i].length; s.channels = zl_dec_out_channels(srcs[i].channels);
        s.sample_rate = srcs[i].sample_rate; s.flags = 0; s.pad = 0;
        pub[(size_t)i] = ZlDecPublish{ s, ids[(size_t)i], zl_dec_is_float(srcs[i].format) ? 1 : 0 };
    }
    // (the piece records are measured by their doubled count: a call that grows anything also grows them once it fills more than half)
    const char *what = "sound_upload_pcm: no device memory for the staging buffer or the call's records";
    const size_t np = std::max<size_t>(pieces.size() * 2, 64), nc = std::max<size_t>((size_t)count * 2, 64);
    const int rsv = reserve(e, false, { { ZB_PCM_STAGE, stageBytes, 1, stageBytes, false, what }, { ZB_PCM_PIECES, pieces.size(), sizeof(ZlDecPiece), np, false, what, np },
                                       { ZB_PCM_PUB, (size_t)count, sizeof(ZlDecPublish), nc, false, what }, { ZB_PCM_VERDICTS, (size_t)count, sizeof(uint32_t), nc, false, what } });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    zlhip_engine::Pcm &P = e->pcm;
    unsigned char *const stage = (unsigned char *)e->scratch[ZB_PCM_STAGE].d; ZlDecPiece *const dPieces = (ZlDecPiece *)e->scratch[ZB_PCM_PIECES].d;
    ZlDecPublish *const dPub = (ZlDecPublish *)e->scratch[ZB_PCM_PUB].d; uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_PCM_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call
    std::vector<uint32_t> verdicts((size_t)count, 0u);
    const bool prof = e->profiling;
    const size_t nev = prof ? 2 * passes.size() + 1 : 0;
    int krc = 0;
    while (krc == 0 && P.ev.size() < nev) { ZlEvent ev; krc = (int)ev.create(); if (krc == 0) P.ev.push_back(std::move(ev)); }
    if (krc == 0) krc = (int)hipMemsetAsync(dVerdicts, 0, (size_t)count * sizeof(uint32_t), e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPieces, pieces.data(), pieces.size() * sizeof(ZlDecPiece), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, pub.data(), pub.size() * sizeof(ZlDecPublish), hipMemcpyHostToDevice, e->stream);
    for (size_t a = 0; krc == 0 && a < passes.size(); ++a) {
        const ZlDecPass &ps = passes[a];
        if (prof) krc = (int)hipEventRecord(P.ev[2 * a], e->stream);
        for (int32_t k = ps.first_piece; krc == 0 && k < ps.first_piece + ps.npieces; ++k) {
            const ZlDecPiece &R = pieces[(size_t)k];
            const unsigned char *src = (const unsigned char *)srcs[R.verdict].frames + zl_dec_source_offset(R);
            krc = (int)hipMemcpyAsync(stage + R.stage_off, src, (size_t)zl_dec_piece_bytes(R), hipMemcpyHostToDevice, e->stream);
        }
        if (prof && krc == 0) krc = (int)hipEventRecord(P.ev[2 * a + 1], e->stream);
        if (krc == 0) krc = zl_launch_pcm_decode(dPieces + ps.first_piece, ps.npieces, ps.items, stage, dVerdicts, e->stream);
    }
    if (prof && krc == 0) krc = (int)hipEventRecord(P.ev[2 * passes.size()], e->stream);
    if (krc == 0) krc = zl_launch_pcm_publish(dPub, count, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdicts.data(), dVerdicts, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) { const int w_ = engine_wait(e); if (w_ != ZLHIP_OK) { ext.rollback(); return w_; } }     // the call's one wait
    if (krc != 0) {
        e->err = std::string("sound_upload_pcm: ") + hipGetErrorString((hipError_t)krc);
        (void)hipStreamSynchronize(e->stream);
        ext.rollback();
        return ZLHIP_ERR_HIP;
    }
    if (prof) {
        float copy = 0.0f, dec = 0.0f;
        for (size_t a = 0; a < passes.size(); ++a) {
            float x = 0.0f, y = 0.0f;
            ZL_HIP(e, hipEventElapsedTime(&x, P.ev[2 * a], P.ev[2 * a + 1]));
            ZL_HIP(e, hipEventElapsedTime(&y, P.ev[2 * a + 1], P.ev[2 * a + 2]));
            copy += x; dec += y;
        }
        P.copyMs = copy; P.decodeMs = dec;
    }
    // the host's mirror of what the device has published, and every clip's default parameters (applied at the next render call)
    for (int32_t i = 0; i < count; ++i) {
        const int id = ids[(size_t)i];
        ZlSound s = pub[(size_t)i].s;
        if (!pub[(size_t)i].check || verdicts[(size_t)i] == 0u) s.flags |= ZL_SOUND_FINITE;
        adopt_sound(e, id, s, ext.floats[(size_t)i]);
        zlhip_clip_params p;
        zlhip_clip_params_default(&p, (float)(s.length / s.sample_rate));
        e->hc.forget_clip_params(id);                              // (the first edit of a slot carries the whole record)
        (void)zlhip_clip_set(e, id, &p);
        out_ids[i] = id;
    }
    return ZLHIP_OK;
}

int zlhip_sound_upload_pcm(zlhip_engine *e, const void *frames, int32_t format, int32_t channels, int32_t length, double sample_rate, int32_t *out_id)
{
    if (!e || !out_id) return ZLHIP_ERR_INVALID;
    const zlhip_pcm_source q = { frames, length, channels, format, 0, sample_rate };
    return zlhip_sound_upload_pcm_batch(e, &q, 1, out_id);
}

int zlhip_debug_upload_pcm_timings(zlhip_engine *e, float *copy_ms, float *decode_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (copy_ms) *copy_ms = e->pcm.copyMs;
    if (decode_ms) *decode_ms = e->pcm.decodeMs;
    return ZLHIP_OK;
}

// ---- clip re-render (zl_stretch.h, zl_stretch.hip) ----------------------------------------------------------------------
// ClipAudioSource::setPitch / setSpeedRatio / setGain re-render the clip's playback file from its source and the sound reloads it
// (ClipAudioSource.cpp:279-311,404-413, SamplerSynthSound.cpp:28-68).  Here: every clip of the call is rendered from its ORIGINAL
// upload into a new arena extent (one seek launch, one synthesis launch for the call), then the sound table entries switch -- at a
// block boundary: the resident kernel has left and every queued batch has finished -- and the extents the clips played before go
// back to the arena.  The clip id keeps its slot; a voice playing it reads the new data from its next block at its unchanged position,
// as the reference's voices read the sound's data pointer and length on every block (SamplerSynthVoice.cpp:186-191).
// (a call's device records, grown when a call needs more: the free waits for the device, other engines' kernels step aside)
static int st_reserve(zlhip_engine *e, GrowBuf &b, size_t need, size_t elem)
{
    const size_t n = std::max<size_t>(need, 64);
    const char *what = "sound_rerender: no device memory for the call's records";
    if (need <= b.cap || !b.d) return grow_buf(e, b, need, elem, n, false, what);      // (nothing to free: no wait for the device)
    ZlQuiesce quiet(e);
    return grow_buf(e, b, need, elem, n, false, what);
}

int zlhip_sound_rerender_batch(zlhip_engine *e, const int32_t *ids, const zlhip_rerender_params *params, int32_t count)
{
    if (!e || count < 0 || (count > 0 && (!ids || !params))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    if (count > 65535) return fail(e, ZLHIP_ERR_INVALID, "sound_rerender_batch: more than 65535 clips in one call");
    // validate everything before anything changes
    std::vector<ZlStretchGeom> geo((size_t)count);
    std::vector<char> ident((size_t)count, 0);
    {
        ZlDistinct distinct(e);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t id = ids[i];
            { const int rc = distinct.check(e, "sound_rerender", id); if (rc != ZLHIP_OK) return rc; }
            const zlhip_rerender_params &q = params[i];
            const ZlSound &o = e->soundSlots[(size_t)id].orig;
            if (zl_st_geometry(o.sample_rate, o.length, q.gain_db, q.pitch_semitones, q.speed_ratio, &geo[(size_t)i]) != 0)
                return fail(e, ZLHIP_ERR_INVALID, "sound_rerender: speed outside [0.25, 4], pitch outside [-24, 24], non-finite gain, or a sample rate the stretch cannot take");
            ident[(size_t)i] = zl_st_identity(q.gain_db, q.pitch_semitones, q.speed_ratio) ? 1 : 0;
        }
    }
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }

    ZlNewExtents ext(e, count);                                    // the rendered extents; an identity request gets none
    std::vector<ZlStretchJob> jobs;
    std::vector<int32_t> seekList, jobClip;
    int64_t maxFrames = 0, offs = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (ident[(size_t)i]) continue;
        const ZlSound &o = e->soundSlots[(size_t)ids[i]].orig;
        const ZlStretchGeom &g = geo[(size_t)i];
        { const int rc = ext.take(i, g.N, o.channels); if (rc != ZLHIP_OK) return rc; }
        ZlStretchJob J; std::memset(&J, 0, sizeof J);
        J.geom = g;
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.channels = o.channels;
        J.off_base = offs;
        if (g.stretch && g.nseg > 0) { seekList.push_back((int32_t)jobs.size()); offs += g.nseg; }
        maxFrames = std::max(maxFrames, g.N);
        jobs.push_back(J);
        jobClip.push_back(i);
    }
    std::vector<int32_t> hOffs((size_t)offs);
    if (!jobs.empty()) {
        int rc = st_reserve(e, e->scratch[ZB_ST_JOBS], jobs.size(), sizeof(ZlStretchJob));
        if (rc == ZLHIP_OK) rc = st_reserve(e, e->scratch[ZB_ST_LIST], std::max<size_t>(seekList.size(), 1), sizeof(int32_t));
        if (rc == ZLHIP_OK) rc = st_reserve(e, e->scratch[ZB_ST_OFFS], std::max<size_t>((size_t)offs, 1), sizeof(int32_t));
        if (rc != ZLHIP_OK) { ext.rollback(); return rc; }
        ZlStretchJob *const dStJobs = (ZlStretchJob *)e->scratch[ZB_ST_JOBS].d;
        int32_t *const dStList = (int32_t *)e->scratch[ZB_ST_LIST].d, *const dStOffs = (int32_t *)e->scratch[ZB_ST_OFFS].d;
        hipError_t st = hipMemcpyAsync(dStJobs, jobs.data(), jobs.size() * sizeof(ZlStretchJob), hipMemcpyHostToDevice, e->stream);
        if (st == hipSuccess && !seekList.empty())
            st = hipMemcpyAsync(dStList, seekList.data(), seekList.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        int krc = (int)st;
        zlhip_engine::Rerender &t = e->st;
        t.timer.on = e->profiling;
        if (krc == 0) krc = (int)t.timer.mark(0, e->stream);
        if (krc == 0) krc = zl_launch_stretch_seek(dStJobs, dStList, (int)seekList.size(), dStOffs, e->stream);
        if (krc == 0) krc = (int)t.timer.mark(1, e->stream);
        if (krc == 0) krc = zl_launch_stretch_synth(dStJobs, (int)jobs.size(), maxFrames, dStOffs, e->stream);
        if (krc == 0) krc = (int)t.timer.mark(2, e->stream);
        if (krc == 0 && offs > 0) krc = (int)hipMemcpyAsync(hOffs.data(), dStOffs, (size_t)offs * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
        if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);
        if (krc == 0) krc = (int)t.timer.elapsed(0, 1, &t.seekMs);
        if (krc == 0) krc = (int)t.timer.elapsed(1, 2, &t.synthMs);
        if (krc != 0) {
            e->err = std::string("sound_rerender: ") + hipGetErrorString((hipError_t)krc);
            (void)hipStreamSynchronize(e->stream);
            ext.rollback();
            return ZLHIP_ERR_HIP;
        }
    }
    // the swap: nothing queued can read the extents the clips played until now any more
    for (int32_t i = 0; i < count; ++i) {
        const int32_t id = ids[i];
        zlhip_engine::SoundSlot &slot = e->soundSlots[(size_t)id];
        free_extent(e, (size_t)e->hc.sounds[id].offset, slot.renderFloats);
        ZlSound s = slot.orig;
        // (a rendered extent has not been looked at: it plays without ZL_SOUND_FINITE; identity parameters play the original, with its own flag)
        if (!ident[(size_t)i]) { s.offset = ext.off[(size_t)i]; s.length = (int32_t)geo[(size_t)i].N; s.flags &= ~(int32_t)ZL_SOUND_FINITE; }
        e->hc.sounds[id] = s;
        slot.renderFloats = ext.floats[(size_t)i];
        slot.renderOffsets.clear();
    }
    for (size_t j = 0; j < jobs.size(); ++j) {
        const ZlStretchGeom &g = jobs[j].geom;
        if (g.stretch && g.nseg > 0)
            e->soundSlots[(size_t)ids[jobClip[j]]].renderOffsets.assign(hOffs.begin() + jobs[j].off_base, hOffs.begin() + jobs[j].off_base + g.nseg);
    }
    for (int32_t i = 0; i < count; ++i)
        ZL_HIP(e, hipMemcpyAsync(e->dSounds + ids[i], &e->hc.sounds[ids[i]], sizeof(ZlSound), hipMemcpyHostToDevice, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    return ZLHIP_OK;
}

int zlhip_sound_rerender(zlhip_engine *e, int32_t id, const zlhip_rerender_params *params)
{
    return zlhip_sound_rerender_batch(e, &id, params, 1);
}

// ---- sample-rate conversion (zl_resample.h, zl_resample.hip) --------------------------------------------------------------
// A clip whose rate differs from the engine's plays through the pitched voice path; converted once, band-limited, it is a unit-step
// integer-position source and K2 takes its on-grid form.  Every clip of the call is converted from its original upload into a new
// arena extent by ONE launch, a second one publishes the sound-table entries (ZL_SOUND_FINITE from the device's verdict), and the
// call waits once.  Synchronisation is zlhip_sound_rerender's: the resident kernel has left and every queued batch has finished before
// anything is written.  The converted extent becomes the slot's original: later re-renders start from it.
int zlhip_resample_design(double source_rate, double target_rate, int32_t *L, int32_t *M, int32_t *taps, int32_t *row_floats, float *table, size_t table_floats)
{
    ZlRsGeom g;
    if (zl_rs_geometry(source_rate, target_rate, &g) != 0) return ZLHIP_ERR_INVALID;
    if (L) *L = g.L;
    if (M) *M = g.M;
    if (taps) *taps = g.taps;
    if (row_floats) *row_floats = g.row;
    if (!table) return ZLHIP_OK;
    if (table_floats < (size_t)g.L * (size_t)g.row) return ZLHIP_ERR_CAPACITY;
    zl_rs_design(g, table);
    return ZLHIP_OK;
}

// the device table of a ratio: made by the first call that asks for the ratio, before the call takes anything from the arena, and cached
// for the engine's life once that call has succeeded -- a call that fails frees the tables it added (hipMalloc and hipFree wait for the
// device: other engines' kernels step aside).  The copy is queued on the engine's stream in front of the call's launches and shares
// the call's one wait: the host copy lives until then.
static int rs_table(zlhip_engine *e, const ZlRsGeom &g, float **out)
{
    for (const auto &t : e->rs.tables) if (t.L == g.L && t.M == g.M) { *out = t.d; return ZLHIP_OK; }
    e->rs.tables.emplace_back();
    zlhip_engine::Resample::Table &t = e->rs.tables.back();
    t.L = g.L; t.M = g.M; t.floats = (size_t)g.L * (size_t)g.row;
    t.pending.resize(t.floats);
    zl_rs_design(g, t.pending.data());
    bool ok;
    { ZlQuiesce quiet(e); ok = t.d.alloc(t.floats) == hipSuccess; }
    if (!ok) { (void)hipGetLastError(); e->rs.tables.pop_back(); return fail(e, ZLHIP_ERR_CAPACITY, "sound_convert_rate: no device memory for the filter table"); }
    if (hipMemcpyAsync(t.d, t.pending.data(), t.floats * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(e->stream);
        { ZlQuiesce quiet(e); t.d.reset(); }
        e->rs.tables.pop_back();
        return fail(e, ZLHIP_ERR_HIP, "sound_convert_rate: the filter table did not reach the device");
    }
    e->deviceBytes += t.floats * sizeof(float);
    *out = t.d;
    return ZLHIP_OK;
}
// after a wait for the engine's stream: the tables' host copies are no longer read
static void rs_tables_settled(zlhip_engine *e) { for (auto &t : e->rs.tables) std::vector<float>().swap(t.pending); }
// a failed call: the engine's stream runs dry, the tables behind the first `keep` go back to the device
static void rs_tables_undo(zlhip_engine *e, size_t keep)
{
    (void)hipStreamSynchronize(e->stream);
    rs_tables_settled(e);
    while (e->rs.tables.size() > keep) {
        { ZlQuiesce quiet(e); e->rs.tables.back().d.reset(); }
        e->deviceBytes -= e->rs.tables.back().floats * sizeof(float);
        e->rs.tables.pop_back();
    }
}

int zlhip_sound_convert_rate_batch(zlhip_engine *e, const int32_t *ids, int32_t count, double target_rate)
{
    if (!e || count < 0 || (count > 0 && !ids)) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    const double ft = target_rate == 0.0 ? e->cfg.playback_sample_rate : target_rate;
    // validate everything before the first HIP call
    std::vector<ZlRsGeom> geo((size_t)count);
    std::vector<int64_t> outN((size_t)count, 0);
    std::vector<char> skip((size_t)count, 0);
    {
        ZlDistinct distinct(e);
        int64_t wgs = 0;
        for (int32_t i = 0; i < count; ++i) { const int rc = distinct.check(e, "sound_convert_rate", ids[i]); if (rc != ZLHIP_OK) return rc; }
        for (int32_t i = 0; i < count; ++i) {
            const ZlSound &o = e->soundSlots[(size_t)ids[i]].orig;
            skip[(size_t)i] = o.sample_rate == ft ? 1 : 0;           // (already at the rate, whatever the rate: nothing to check, nothing to do)
            if (skip[(size_t)i]) continue;
            if (zl_rs_geometry(o.sample_rate, ft, &geo[(size_t)i]) != 0)
                return fail(e, ZLHIP_ERR_INVALID, "sound_convert_rate: a rate that is no integer in [1000, 768000], or a ratio beyond L <= 2048, M <= 8 L, 262144 table floats");
            outN[(size_t)i] = zl_rs_out_frames(geo[(size_t)i], o.length);
            if (outN[(size_t)i] < 1) return fail(e, ZLHIP_ERR_INVALID, "sound_convert_rate: the converted clip would exceed 2^31 - 9 frames");
            wgs += zl_rs_job_wgs((int32_t)outN[(size_t)i]);
        }
        if (wgs > (int64_t)INT32_MAX) return fail(e, ZLHIP_ERR_INVALID, "sound_convert_rate_batch: more than 2^31 - 1 workgroups in one call");
        for (int32_t i = 0; i < count; ++i) {
            if (skip[(size_t)i]) continue;
            const int rc = check_plays_original(e, ids[i], "sound_convert_rate: the clip plays a re-render (re-render it with gain 0, pitch 0, speed 1 first)");
            if (rc != ZLHIP_OK) return rc;
        }
    }
    int32_t njobs = 0;
    for (int32_t i = 0; i < count; ++i) njobs += skip[(size_t)i] ? 0 : 1;
    if (njobs == 0) return ZLHIP_OK;                               // every clip is at the target rate already: no launch, no copy
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }

    // the filter tables of the call's ratios first; a call that fails frees the ones it added
    const size_t tables0 = e->rs.tables.size();
    std::vector<float *> tables((size_t)count, nullptr);
    for (int32_t i = 0; i < count; ++i) {
        if (skip[(size_t)i]) continue;
        const int rc = rs_table(e, geo[(size_t)i], &tables[(size_t)i]);
        if (rc != ZLHIP_OK) { rs_tables_undo(e, tables0); return rc; }
    }
    // the new extents and the jobs; a call that fails from here on gives its tables back before its extents
    ZlNewExtents ext(e, count);
    ext.undo_first = [&]() { rs_tables_undo(e, tables0); };
    ZlClipSwap swap{ e, "sound_convert_rate", ext };
    std::vector<ZlRsJob> jobs;
    int32_t wgs = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (skip[(size_t)i]) continue;
        const ZlSound &o = e->soundSlots[(size_t)ids[i]].orig;
        const ZlRsGeom &g = geo[(size_t)i];
        { const int rc = ext.take(i, outN[(size_t)i], o.channels); if (rc != ZLHIP_OK) return rc; }
        ZlRsJob J; std::memset(&J, 0, sizeof J);
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.table = (uint64_t)(uintptr_t)tables[(size_t)i];
        J.len = o.length; J.N = (int32_t)outN[(size_t)i]; J.channels = o.channels;
        J.L = g.L; J.M = g.M; J.half = g.half; J.taps = g.taps; J.row = g.row;
        J.wg_base = wgs;
        wgs += zl_rs_job_wgs(J.N);
        ZlSound s = o; s.length = J.N; s.sample_rate = ft;
        J.verdict = swap.add(i, ids[i], s);
        jobs.push_back(J);
    }
    const char *what = "sound_convert_rate: no device memory for the call's records";
    const size_t nj = jobs.size(), n = std::max<size_t>(nj * 2, 64);
    const int rsv = reserve(e, false, { { ZB_RS_JOBS, nj, sizeof(ZlRsJob), n, false, what }, { ZB_RS_PUB, nj, sizeof(ZlRsPublish), n, false, what },
                                       { ZB_RS_VERDICTS, nj, sizeof(uint32_t), n, false, what } });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    ZlRsJob *const dJobs = (ZlRsJob *)e->scratch[ZB_RS_JOBS].d; ZlRsPublish *const dPub = (ZlRsPublish *)e->scratch[ZB_RS_PUB].d;
    uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_RS_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call
    std::vector<uint32_t> verdicts(jobs.size(), 0u);
    e->rs.timer.on = e->profiling;
    int krc = (int)hipMemsetAsync(dVerdicts, 0, jobs.size() * sizeof(uint32_t), e->stream);     // (every word starts clear here, not as swap.words)
    if (krc == 0) krc = (int)hipMemcpyAsync(dJobs, jobs.data(), jobs.size() * sizeof(ZlRsJob), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, swap.pub.data(), nj * sizeof(ZlRsPublish), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)e->rs.timer.mark(0, e->stream);
    if (krc == 0) krc = zl_launch_resample(dJobs, (int32_t)jobs.size(), wgs, dVerdicts, e->stream);
    if (krc == 0) krc = zl_launch_resample_publish(dPub, (int32_t)nj, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)e->rs.timer.mark(1, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdicts.data(), dVerdicts, jobs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's one wait
    if (krc == 0) krc = (int)e->rs.timer.elapsed(0, 1, &e->rs.ms);
    if (krc != 0) return swap.hip_failed(krc);
    rs_tables_settled(e);
    swap.commit(verdicts);
    return ZLHIP_OK;
}

int zlhip_sound_convert_rate(zlhip_engine *e, int32_t id, double target_rate)
{
    return zlhip_sound_convert_rate_batch(e, &id, 1, target_rate);
}

int zlhip_debug_convert_timings(zlhip_engine *e, float *device_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (device_ms) *device_ms = e->rs.ms;
    return ZLHIP_OK;
}

// ---- waveform overviews (zl_overview.h, zl_overview.hip) -----------------------------------------------------------------
// The data behind the reference's WaveFormItem (lib/WaveFormItem.cpp:130-139): per pixel column the minimum and maximum of the
// clip's playback data, reduced where the data lives -- after a re-render the clip that plays exists on the device only.  Like every
// analysis below, the call runs on the engine's stream behind what is queued there and does NOT ask the resident real-time kernel to
// leave (call_begin: it reads the arena, which only uploads, releases and re-renders change -- and those stop the kernel and wait
// themselves), and its buffers are allocated by the first call and grow only (reserve).
int zlhip_sound_overview_batch(zlhip_engine *e, const zlhip_overview_request *reqs, int32_t count, float *out, size_t out_floats)
{
    if (!e || count < 0 || (count > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    // validate everything before anything is written
    int64_t columns = 0;
    for (int32_t i = 0; i < count; ++i) {
        const zlhip_overview_request &q = reqs[i];
        auto resolve = [&](const ZlSound &) { return q.columns < 1 || q.columns > ZLHIP_OVERVIEW_MAX_COLUMNS ? "columns outside 1 .. 4096" : nullptr; };
        { const int rc = check_request(e, "sound_overview", q, resolve); if (rc != ZLHIP_OK) return rc; }
        columns += q.columns;
        if (columns > ZL_OV_MAX_CALL_COLUMNS) return fail(e, ZLHIP_ERR_INVALID, "sound_overview_batch: more than 262144 columns in one call");
    }
    if (out_floats < (size_t)columns * 4) return fail(e, ZLHIP_ERR_CAPACITY, "sound_overview: out holds fewer than 4 floats per column");
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    const size_t nreq = (size_t)count, ncols = (size_t)columns, ccap = std::min<size_t>(std::max<size_t>(ncols * 2, ZL_OV_MAX_COLUMNS), ZL_OV_MAX_CALL_COLUMNS);
    const int rsv = reserve(e, true, { { ZB_OV_REQ, nreq, sizeof(ZlOvRequest), std::max<size_t>(nreq * 2, 64), true, "sound_overview: no memory for the call's requests" },
                                      { ZB_OV_COLS, ncols, 4 * sizeof(float), ccap, true, "sound_overview: no memory for the call's columns" } });
    if (rsv != ZLHIP_OK) return rsv;
    zlhip_engine::Overview &o = e->ov;
    ZlOvRequest *const hReq = (ZlOvRequest *)e->scratch[ZB_OV_REQ].h, *const dReq = (ZlOvRequest *)e->scratch[ZB_OV_REQ].d;
    float *const hCols = (float *)e->scratch[ZB_OV_COLS].h; uint32_t *const dCols = (uint32_t *)e->scratch[ZB_OV_COLS].d;
    // the request records: where the extent lies (64-bit, per request: a grown arena's segments are far apart), what to cut it into
    int64_t items = 0; int32_t col = 0;
    for (int32_t i = 0; i < count; ++i) {
        const zlhip_overview_request &q = reqs[i];
        const ZlSound &s = e->hc.sounds[q.id];
        ZlOvRequest &R = hReq[i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, s.offset);
        R.item_base = items;
        R.first = q.first_frame; R.frames = q.num_frames; R.columns = q.columns;
        R.channels = s.channels;
        R.col_base = col;
        R.ppc = zl_ov_pieces_per_column(q.num_frames, q.columns);
        items += zl_ov_items(q.num_frames, q.columns);
        col += q.columns;
    }
    o.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)count * sizeof(ZlOvRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, o.timer.mark(0, e->stream));
    ZL_HIP(e, hipMemsetAsync(dCols, 0, (size_t)columns * 4 * sizeof(float), e->stream));
    ZL_KERNEL(e, zl_launch_overview_reduce(dReq, count, items, dCols, e->stream));
    ZL_KERNEL(e, zl_launch_overview_finish(dCols, (int32_t)columns, e->stream));
    ZL_HIP(e, o.timer.mark(1, e->stream));
    ZL_HIP(e, hipMemcpyAsync(hCols, dCols, (size_t)columns * 4 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, o.timer.elapsed(0, 1, &o.ms));
    std::memcpy(out, hCols, (size_t)columns * 4 * sizeof(float));
    return ZLHIP_OK;
}

int zlhip_sound_overview(zlhip_engine *e, int32_t id, int32_t first_frame, int32_t num_frames, int32_t columns, float *out)
{
    const zlhip_overview_request q = { id, first_frame, num_frames, columns };
    return zlhip_sound_overview_batch(e, &q, 1, out, columns > 0 ? (size_t)columns * 4 : 0);
}

int zlhip_debug_overview_timings(zlhip_engine *e, float *device_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (device_ms) *device_ms = e->ov.ms;
    return ZLHIP_OK;
}

// ---- transients (zl_onset.h, zl_onset.hip) ---------------------------------------------------------------------------------
// Where a sampler slices a loop.  The synchronisation and the buffers are the overviews'.  The counts and the onsets are written by
// the pick kernel into host memory mapped into the device, so only what was found crosses.
int zlhip_onset_resolve(double sample_rate, zlhip_onset_request *r)
{
    if (!r || r->first_frame < 0 || r->num_frames < 1) return ZLHIP_ERR_INVALID;
    zlhip_onset_request q = *r;
    if (zl_on_resolve(sample_rate, &q.hop_frames, &q.gate, &q.threshold, &q.min_gap_hops, &q.max_onsets) != 0) return ZLHIP_ERR_INVALID;
    if (zl_on_hops(q.num_frames, q.hop_frames) > ZL_ON_MAX_HOPS) return ZLHIP_ERR_INVALID;
    *r = q;
    return ZLHIP_OK;
}

int zlhip_sound_onsets_batch(zlhip_engine *e, const zlhip_onset_request *reqs, int32_t nreq, zlhip_onset *out, size_t capacity, int32_t *counts)
{
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out || !counts))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<zlhip_onset_request> res((size_t)nreq);
    int64_t hops = 0; size_t nout = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_onset_request &q = res[(size_t)i];
        q = reqs[i];
        auto resolve = [&](const ZlSound &s) { return zlhip_onset_resolve(s.sample_rate, &q) != ZLHIP_OK ? kOutsideLimits : nullptr; };
        { const int rc = check_request(e, "sound_onsets", q, resolve); if (rc != ZLHIP_OK) return rc; }
        hops += zl_on_hops(q.num_frames, q.hop_frames);
        if (hops > ZL_ON_MAX_CALL_HOPS) return fail(e, ZLHIP_ERR_INVALID, "sound_onsets_batch: more than 4194304 hops in one call");
        nout += (size_t)q.max_onsets;
    }
    if (capacity < nout) return fail(e, ZLHIP_ERR_CAPACITY, "sound_onsets: out holds fewer onsets than the requests' max_onsets");
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Onset &o = e->on;
    const char *what = "sound_onsets: no memory for the call's buffers";
    const size_t n = (size_t)nreq, h = (size_t)hops, hcap = std::min<size_t>(std::max<size_t>(h * 2, 4096), ZL_ON_MAX_CALL_HOPS);
    const int rsv = reserve(e, true, { { ZB_ON_REQ, n, sizeof(ZlOnRequest), std::max<size_t>(n * 2, 64), true, what }, { ZB_ON_E, h, sizeof(uint64_t), hcap, false, what },
                                      { ZB_ON_N, h, sizeof(int32_t), hcap, false, what }, { ZB_ON_PS, h, sizeof(uint32_t), hcap, false, what } },
                           { mapped_need(o.counts, std::max<size_t>(n, 32)), mapped_need(o.out, std::max<size_t>(nout, 512)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlOnRequest *const hReq = (ZlOnRequest *)e->scratch[ZB_ON_REQ].h, *const dReq = (ZlOnRequest *)e->scratch[ZB_ON_REQ].d;
    uint64_t *const dE = (uint64_t *)e->scratch[ZB_ON_E].d; int32_t *const dN = (int32_t *)e->scratch[ZB_ON_N].d; uint32_t *const dPs = (uint32_t *)e->scratch[ZB_ON_PS].d;
    o.last.clear();
    int32_t hop0 = 0, out0 = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        const zlhip_onset_request &q = res[(size_t)i];
        const ZlSound &s = e->hc.sounds[q.id];
        ZlOnRequest &R = hReq[i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, s.offset);
        R.floor_ = zl_on_floor(q.hop_frames, s.channels, q.gate);
        R.first = q.first_frame; R.frames = q.num_frames; R.hop = q.hop_frames; R.channels = s.channels;
        R.hops = (int32_t)zl_on_hops(q.num_frames, q.hop_frames);
        R.hop_base = hop0;
        R.threshold = q.threshold; R.min_gap = q.min_gap_hops; R.max_onsets = q.max_onsets;
        R.out_base = out0;
        o.last.emplace_back(hop0, R.hops);
        hop0 += R.hops; out0 += q.max_onsets;
    }
    o.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)nreq * sizeof(ZlOnRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, o.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_onset_energy(dReq, nreq, hops, dE, e->stream));
    ZL_HIP(e, o.timer.mark(1, e->stream));
    ZL_KERNEL(e, zl_launch_onset_pick(dReq, nreq, dE, dN, dPs, o.counts.d, o.out.d, e->stream));
    ZL_HIP(e, o.timer.mark(2, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, o.timer.elapsed(0, 1, &o.energyMs)); ZL_HIP(e, o.timer.elapsed(1, 2, &o.restMs));
    size_t at = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        const int32_t n = o.counts.h[i];
        std::memcpy(out + at, o.out.h + hReq[i].out_base, (size_t)n * sizeof(zlhip_onset));
        counts[i] = n;
        at += (size_t)n;
    }
    return ZLHIP_OK;
}

int zlhip_sound_onsets(zlhip_engine *e, const zlhip_onset_request *r, zlhip_onset *out, int32_t capacity, int32_t *count)
{
    if (capacity < 0) return ZLHIP_ERR_INVALID;
    return zlhip_sound_onsets_batch(e, r, 1, out, (size_t)capacity, count);
}

int zlhip_debug_onset_hops(zlhip_engine *e, int32_t request, uint64_t *energy, int32_t *strength, int32_t capacity, int32_t *hops)
{
    if (!e || request < 0 || (size_t)request >= e->on.last.size()) return ZLHIP_ERR_INVALID;
    const int32_t base = e->on.last[(size_t)request].first, n = e->on.last[(size_t)request].second;
    if (hops) *hops = n;
    if (!energy && !strength) return ZLHIP_OK;
    if (capacity < n) return fail(e, ZLHIP_ERR_CAPACITY, "debug_onset_hops: capacity below the request's hops");
    ZL_HIP(e, hipSetDevice(e->device));
    if (energy) ZL_HIP(e, hipMemcpyAsync(energy, (const uint64_t *)e->scratch[ZB_ON_E].d + base, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    if (strength) ZL_HIP(e, hipMemcpyAsync(strength, (const int32_t *)e->scratch[ZB_ON_N].d + base, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_onset_timings(zlhip_engine *e, float *energy_ms, float *rest_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (energy_ms) *energy_ms = e->on.energyMs;
    if (rest_ms) *rest_ms = e->on.restMs;
    return ZLHIP_OK;
}

// ---- tempo (zl_tempo.h, zl_tempo.hip) --------------------------------------------------------------------------------------
// How fast a loop is.  The samples are read once, by the transients' energy kernel; the flux, the autocorrelation and the pick are
// integer arithmetic on one word per hop.  Synchronisation and buffers as for the overviews.  The integer records are written by the
// pick kernel into host memory mapped into the device; bpm and confidence are derived here (zl_tp_finish).
int zlhip_tempo_resolve(double sample_rate, zlhip_tempo_request *r)
{
    if (!r || r->first_frame < 0 || r->num_frames < 1) return ZLHIP_ERR_INVALID;
    zlhip_tempo_request q = *r;
    if (zl_tp_resolve(sample_rate, &q.hop_frames, &q.bpm_min, &q.bpm_max) != 0) return ZLHIP_ERR_INVALID;
    if (zl_on_hops(q.num_frames, q.hop_frames) > ZL_TP_MAX_HOPS) return ZLHIP_ERR_INVALID;
    *r = q;
    return ZLHIP_OK;
}

static const size_t kTpRecordBytes = sizeof(ZlOnRequest) + sizeof(ZlTpRequest);     // per request: the energy pass's record and the tempo kernels'

int zlhip_sound_tempo_batch(zlhip_engine *e, const zlhip_tempo_request *reqs, int32_t nreq, zlhip_tempo *out)
{
    static_assert(sizeof(zlhip_tempo) == sizeof(ZlTpResult), "the device writes zlhip_tempo's layout");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<zlhip_tempo_request> res((size_t)nreq);
    std::vector<ZlTpRequest> geo((size_t)nreq);
    int64_t hops = 0, lags = 0, items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_tempo_request &q = res[(size_t)i];
        q = reqs[i];
        auto resolve = [&](const ZlSound &s) { return zlhip_tempo_resolve(s.sample_rate, &q) != ZLHIP_OK ? kOutsideLimits : nullptr; };
        { const int rc = check_request(e, "sound_tempo", q, resolve); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        ZlTpRequest &T = geo[(size_t)i];
        double lmin, lmax;
        zl_tp_lags(s.sample_rate, q.hop_frames, q.bpm_min, q.bpm_max, &lmin, &lmax);
        zl_tp_geometry(&T, (int32_t)zl_on_hops(q.num_frames, q.hop_frames), lmin, lmax);
        T.hop_base = (int32_t)hops; T.acf_base = (int32_t)lags; T.item_base = (int32_t)items;
        hops += T.hops; lags += T.nlags; items += zl_tp_items(T);
        if (hops > ZL_TP_MAX_CALL_HOPS) return fail(e, ZLHIP_ERR_INVALID, "sound_tempo_batch: more than 4194304 hops in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Tempo &t = e->tp;
    const char *what = "sound_tempo: no memory for the call's buffers";
    const size_t n = (size_t)nreq, h = (size_t)hops, l = (size_t)lags, rcap = std::max<size_t>(n * 2, 64);
    const size_t hcap = std::min<size_t>(std::max<size_t>(h * 2, 4096), ZL_TP_MAX_CALL_HOPS);
    const int rsv = reserve(e, true, { { ZB_TP_REQ, n, kTpRecordBytes, rcap, true, what }, { ZB_TP_E, h, sizeof(uint64_t), hcap, false, what },
                                      { ZB_TP_W, h, sizeof(uint16_t), hcap, false, what }, { ZB_TP_A, l, sizeof(uint64_t), std::max<size_t>(l * 2, 4096), false, what },
                                      { ZB_TP_STAT, n, sizeof(ZlTpStat), rcap, false, what } }, { mapped_need(t.out, std::max<size_t>(n, 32)) });
    if (rsv != ZLHIP_OK) return rsv;
    char *const hRec = (char *)e->scratch[ZB_TP_REQ].h, *const dRec = (char *)e->scratch[ZB_TP_REQ].d;
    ZlOnRequest *const hOn = (ZlOnRequest *)hRec, *const dOn = (ZlOnRequest *)dRec;
    ZlTpRequest *const hTp = (ZlTpRequest *)(hRec + (size_t)nreq * sizeof(ZlOnRequest)), *const dTp = (ZlTpRequest *)(dRec + (size_t)nreq * sizeof(ZlOnRequest));
    uint64_t *const dE = (uint64_t *)e->scratch[ZB_TP_E].d; uint16_t *const dW = (uint16_t *)e->scratch[ZB_TP_W].d;
    uint64_t *const dA = (uint64_t *)e->scratch[ZB_TP_A].d; ZlTpStat *const dStat = (ZlTpStat *)e->scratch[ZB_TP_STAT].d;
    t.last.clear();
    for (int32_t i = 0; i < nreq; ++i) {
        const zlhip_tempo_request &q = res[(size_t)i];
        const ZlSound &s = e->hc.sounds[q.id];
        const ZlTpRequest &T = geo[(size_t)i];
        ZlOnRequest &R = hOn[i];
        std::memset(&R, 0, sizeof(R));
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, s.offset);
        R.first = q.first_frame; R.frames = q.num_frames; R.hop = q.hop_frames; R.channels = s.channels;
        R.hops = T.hops; R.hop_base = T.hop_base;
        hTp[i] = T;
        t.last.push_back({T.hop_base, T.hops, T.acf_base, T.first_lag, T.nlags});
    }
    t.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dRec, hRec, (size_t)nreq * kTpRecordBytes, hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, t.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_onset_energy(dOn, nreq, hops, dE, e->stream));
    ZL_HIP(e, t.timer.mark(1, e->stream));
    ZL_KERNEL(e, zl_launch_tempo_flux(dTp, nreq, dE, dW, dA, dStat, e->stream));
    ZL_HIP(e, t.timer.mark(2, e->stream));
    ZL_KERNEL(e, zl_launch_tempo_acf(dTp, nreq, items, dW, dA, e->stream));
    ZL_HIP(e, t.timer.mark(3, e->stream));
    ZL_KERNEL(e, zl_launch_tempo_pick(dTp, nreq, dA, dStat, t.out.d, e->stream));
    ZL_HIP(e, t.timer.mark(4, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    if (t.timer.on) {
        float flux = 0.0f, pick = 0.0f;
        ZL_HIP(e, t.timer.elapsed(0, 1, &t.energyMs)); ZL_HIP(e, t.timer.elapsed(1, 2, &flux));
        ZL_HIP(e, t.timer.elapsed(2, 3, &t.acfMs)); ZL_HIP(e, t.timer.elapsed(3, 4, &pick));
        t.restMs = flux + pick;
    }
    for (int32_t i = 0; i < nreq; ++i) {
        ZlTpResult r = t.out.h[i];
        zl_tp_finish(e->hc.sounds[res[(size_t)i].id].sample_rate, res[(size_t)i].hop_frames, &r);
        std::memcpy(&out[i], &r, sizeof(r));
    }
    return ZLHIP_OK;
}

int zlhip_sound_tempo(zlhip_engine *e, const zlhip_tempo_request *r, zlhip_tempo *out) { return zlhip_sound_tempo_batch(e, r, 1, out); }

int zlhip_debug_tempo_acf(zlhip_engine *e, int32_t request, uint16_t *flux, uint64_t *acf, int32_t capacity, int32_t *hops, int32_t *first_lag, int32_t *lags)
{
    if (!e || request < 0 || (size_t)request >= e->tp.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Tempo::Last &l = e->tp.last[(size_t)request];
    if (hops) *hops = l.hops;
    if (first_lag) *first_lag = l.first_lag;
    if (lags) *lags = l.nlags;
    if (!flux && !acf) return ZLHIP_OK;
    if ((flux && capacity < l.hops) || (acf && capacity < l.nlags)) return fail(e, ZLHIP_ERR_CAPACITY, "debug_tempo_acf: capacity below the request's hops or lags");
    ZL_HIP(e, hipSetDevice(e->device));
    if (flux) ZL_HIP(e, hipMemcpyAsync(flux, (const uint16_t *)e->scratch[ZB_TP_W].d + l.hop_base, (size_t)l.hops * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
    if (acf && l.nlags > 0) ZL_HIP(e, hipMemcpyAsync(acf, (const uint64_t *)e->scratch[ZB_TP_A].d + l.acf_base, (size_t)l.nlags * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_tempo_timings(zlhip_engine *e, float *energy_ms, float *acf_ms, float *rest_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (energy_ms) *energy_ms = e->tp.energyMs;
    if (acf_ms) *acf_ms = e->tp.acfMs;
    if (rest_ms) *rest_ms = e->tp.restMs;
    return ZLHIP_OK;
}

// ---- pitch (zl_pitch.h, zl_pitch.hip) --------------------------------------------------------------------------------------
// What note a clip is.  The diff kernel reads the analysed frames' samples and leaves d per frame and lag; the pick and the vote are
// integer arithmetic on it.  Synchronisation and buffers as for the overviews.  The integer records are written by the vote kernel
// into host memory mapped into the device; hz, note, root_note, cents and confidence are derived here (zl_pt_finish).
int zlhip_pitch_resolve(double sample_rate, zlhip_pitch_request *r)
{
    if (!r || r->first_frame < 0 || r->num_frames < 1) return ZLHIP_ERR_INVALID;
    zlhip_pitch_request q = *r;
    if (zl_pt_resolve(sample_rate, &q.window, &q.max_frames, &q.f_min, &q.f_max, &q.threshold, &q.gate) != 0) return ZLHIP_ERR_INVALID;
    *r = q;
    return ZLHIP_OK;
}

int zlhip_sound_pitch_batch(zlhip_engine *e, const zlhip_pitch_request *reqs, int32_t nreq, zlhip_pitch *out)
{
    static_assert(sizeof(zlhip_pitch) == sizeof(ZlPtResult), "the device writes zlhip_pitch's layout");
    static_assert(sizeof(zlhip_pitch_frame) == sizeof(ZlPtFrame), "the device writes zlhip_pitch_frame's layout");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<ZlPtRequest> geo((size_t)nreq);
    std::vector<double> rate((size_t)nreq);
    int64_t frames = 0, words = 0, items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_pitch_request q = reqs[i];
        auto resolve = [&](const ZlSound &s) { return zlhip_pitch_resolve(s.sample_rate, &q) != ZLHIP_OK ? kOutsideLimits : nullptr; };
        { const int rc = check_request(e, "sound_pitch", q, resolve); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        ZlPtRequest &R = geo[(size_t)i];
        double tmin, tmax;
        zl_pt_lags(s.sample_rate, q.f_min, q.f_max, &tmin, &tmax);
        R.src = 0;                                                 // (the address: behind the reserve, with the other HIP-side state)
        R.floor_ = (uint64_t)q.window * (uint64_t)s.channels * (uint64_t)q.gate * (uint64_t)q.gate;
        R.first = q.first_frame; R.channels = s.channels;
        R.window = q.window; R.tmin = (int32_t)tmin; R.tmax = (int32_t)tmax; R.threshold = q.threshold;
        zl_pt_frames(q.num_frames, R.window, R.tmax, q.max_frames, &R.frames, &R.hop);
        R.d_base = words; R.frame_base = (int32_t)frames; R.item_base = (int32_t)items;
        rate[(size_t)i] = s.sample_rate;
        frames += R.frames; words += (int64_t)R.frames * zl_pt_nd(R); items += zl_pt_items(R);
        if (frames > ZL_PT_MAX_CALL_FRAMES) return fail(e, ZLHIP_ERR_INVALID, "sound_pitch_batch: more than 65536 analysis frames in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Pitch &t = e->pt;
    const char *what = "sound_pitch: no memory for the call's buffers";
    const size_t n = (size_t)nreq, f = (size_t)frames, w = (size_t)words, fcap = std::min<size_t>(std::max<size_t>(f * 2, 256), ZL_PT_MAX_CALL_FRAMES);
    const int rsv = reserve(e, true, { { ZB_PT_REQ, n, sizeof(ZlPtRequest), std::max<size_t>(n * 2, 64), true, what },
                                      { ZB_PT_D, w, sizeof(uint64_t), std::max<size_t>(w + w / 2, 65536), false, what },
                                      { ZB_PT_STAT, f, sizeof(ZlPtStat), fcap, false, what }, { ZB_PT_FRAME, f, sizeof(ZlPtFrame), fcap, false, what } },
                           { mapped_need(t.out, std::max<size_t>(n, 32)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlPtRequest *const hReq = (ZlPtRequest *)e->scratch[ZB_PT_REQ].h, *const dReq = (ZlPtRequest *)e->scratch[ZB_PT_REQ].d;
    uint64_t *const dD = (uint64_t *)e->scratch[ZB_PT_D].d; ZlPtStat *const dStat = (ZlPtStat *)e->scratch[ZB_PT_STAT].d;
    ZlPtFrame *const dFrame = (ZlPtFrame *)e->scratch[ZB_PT_FRAME].d;
    t.last.clear();
    for (int32_t i = 0; i < nreq; ++i) {
        ZlPtRequest &R = hReq[i];
        R = geo[(size_t)i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, e->hc.sounds[reqs[i].id].offset);
        t.last.push_back({R.d_base, R.frame_base, R.frames, zl_pt_nd(R)});
    }
    t.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)nreq * sizeof(ZlPtRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, t.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_pitch_diff(dReq, nreq, items, dD, dStat, e->stream));
    ZL_HIP(e, t.timer.mark(1, e->stream));
    ZL_KERNEL(e, zl_launch_pitch_pick(dReq, nreq, frames, dD, dStat, dFrame, e->stream));
    ZL_KERNEL(e, zl_launch_pitch_vote(dReq, nreq, dFrame, t.out.d, e->stream));
    ZL_HIP(e, t.timer.mark(2, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, t.timer.elapsed(0, 1, &t.diffMs)); ZL_HIP(e, t.timer.elapsed(1, 2, &t.restMs));
    for (int32_t i = 0; i < nreq; ++i) {
        ZlPtResult r = t.out.h[i];
        zl_pt_finish(rate[(size_t)i], &r);
        std::memcpy(&out[i], &r, sizeof(r));
    }
    return ZLHIP_OK;
}

int zlhip_sound_pitch(zlhip_engine *e, const zlhip_pitch_request *r, zlhip_pitch *out) { return zlhip_sound_pitch_batch(e, r, 1, out); }

int zlhip_debug_pitch_frames(zlhip_engine *e, int32_t request, zlhip_pitch_frame *records, int32_t capacity, int32_t *frames)
{
    if (!e || request < 0 || (size_t)request >= e->pt.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Pitch::Last &l = e->pt.last[(size_t)request];
    if (frames) *frames = l.frames;
    if (!records) return ZLHIP_OK;
    if (capacity < l.frames) return fail(e, ZLHIP_ERR_CAPACITY, "debug_pitch_frames: capacity below the request's frames");
    if (l.frames == 0) return ZLHIP_OK;
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(records, (const ZlPtFrame *)e->scratch[ZB_PT_FRAME].d + l.frame_base, (size_t)l.frames * sizeof(ZlPtFrame), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_pitch_diff(zlhip_engine *e, int32_t request, int32_t frame, uint64_t *d, int32_t capacity, int32_t *lags)
{
    if (!e || request < 0 || (size_t)request >= e->pt.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Pitch::Last &l = e->pt.last[(size_t)request];
    if (lags) *lags = l.nd;
    if (!d) return ZLHIP_OK;
    if (frame < 0 || frame >= l.frames) return fail(e, ZLHIP_ERR_INVALID, "debug_pitch_diff: no such frame");
    if (capacity < l.nd) return fail(e, ZLHIP_ERR_CAPACITY, "debug_pitch_diff: capacity below the request's lags");
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(d, (const uint64_t *)e->scratch[ZB_PT_D].d + l.d_base + (int64_t)frame * l.nd, (size_t)l.nd * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_pitch_timings(zlhip_engine *e, float *diff_ms, float *rest_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (diff_ms) *diff_ms = e->pt.diffMs;
    if (rest_ms) *rest_ms = e->pt.restMs;
    return ZLHIP_OK;
}

// ---- loudness (zl_loudness.h, zl_loudness.hip) -----------------------------------------------------------------------------
// How loud a clip is: BS.1770's integrated loudness and the sample peak.  The kernel filters and sums the sub-blocks, one lane each,
// and writes their records into host memory mapped into the device; the blocks, the gates and lufs are derived here (zl_ld_finish).
// Synchronisation and buffers as for the overviews.
int zlhip_loudness_design(double sample_rate, double *coeffs)
{
    if (!coeffs) return ZLHIP_ERR_INVALID;
    double c[10];
    if (zl_ld_design(sample_rate, c) != 0) return ZLHIP_ERR_INVALID;
    std::memcpy(coeffs, c, sizeof(c));
    return ZLHIP_OK;
}

int zlhip_loudness_resolve(double sample_rate, zlhip_loudness_request *r)
{
    if (!r) return ZLHIP_ERR_INVALID;
    int32_t sub = r->sub_frames;
    if (zl_ld_resolve(sample_rate, r->first_frame, r->num_frames, &sub) != 0) return ZLHIP_ERR_INVALID;
    r->sub_frames = sub;
    return ZLHIP_OK;
}

int zlhip_sound_loudness_batch(zlhip_engine *e, const zlhip_loudness_request *reqs, int32_t nreq, zlhip_loudness *out)
{
    static_assert(sizeof(zlhip_loudness) == sizeof(ZlLdResult), "zl_ld_finish writes zlhip_loudness's layout");
    static_assert(sizeof(zlhip_loudness_sub) == sizeof(ZlLdSub) && sizeof(ZlLdSub) == 24, "the device writes zlhip_loudness_sub's layout");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<ZlLdRequest> geo((size_t)nreq);
    int64_t items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_loudness_request q = reqs[i];
        ZlLdRequest &R = geo[(size_t)i];
        auto resolve = [&](const ZlSound &s) { return zlhip_loudness_resolve(s.sample_rate, &q) != ZLHIP_OK || zl_ld_design(s.sample_rate, R.c) != 0 ? kOutsideLimits : nullptr; };
        { const int rc = check_request(e, "sound_loudness", q, resolve); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        R.src = 0;                                                 // (the address: behind the reserve, with the other HIP-side state)
        R.first = q.first_frame; R.frames = q.num_frames; R.sub = q.sub_frames; R.channels = s.channels;
        R.items = (int32_t)zl_ld_items(q.num_frames, q.sub_frames); R.item_base = (int32_t)items;
        items += R.items;
        if (items > ZL_LD_MAX_CALL_ITEMS) return fail(e, ZLHIP_ERR_INVALID, "sound_loudness_batch: more than 1048576 sub-blocks in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Loudness &t = e->ld;
    const size_t n = (size_t)nreq;
    const int rsv = reserve(e, true, { { ZB_LD_REQ, n, sizeof(ZlLdRequest), std::max<size_t>(n * 2, 64), true, "sound_loudness: no memory for the call's buffers" } },
                           { mapped_need(t.out, std::max<size_t>((size_t)items, 512)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlLdRequest *const hReq = (ZlLdRequest *)e->scratch[ZB_LD_REQ].h, *const dReq = (ZlLdRequest *)e->scratch[ZB_LD_REQ].d;
    t.last.clear();
    for (int32_t i = 0; i < nreq; ++i) {
        ZlLdRequest &R = hReq[i];
        R = geo[(size_t)i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, e->hc.sounds[reqs[i].id].offset);
        t.last.push_back({R.item_base, R.items});
    }
    t.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)nreq * sizeof(ZlLdRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, t.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_loudness(dReq, nreq, (int32_t)items, t.out.d, e->stream));
    ZL_HIP(e, t.timer.mark(1, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, t.timer.elapsed(0, 1, &t.kernelMs));
    for (int32_t i = 0; i < nreq; ++i) {
        const ZlLdRequest &R = geo[(size_t)i];
        ZlLdResult r;
        zl_ld_finish(t.out.h + R.item_base, R.frames, R.sub, &r);
        std::memcpy(&out[i], &r, sizeof(r));
    }
    return ZLHIP_OK;
}

int zlhip_sound_loudness(zlhip_engine *e, const zlhip_loudness_request *r, zlhip_loudness *out) { return zlhip_sound_loudness_batch(e, r, 1, out); }

int zlhip_debug_loudness_subs(zlhip_engine *e, int32_t request, zlhip_loudness_sub *records, int32_t capacity, int32_t *count)
{
    if (!e || request < 0 || (size_t)request >= e->ld.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Loudness::Last &l = e->ld.last[(size_t)request];
    if (count) *count = l.items;
    if (!records) return ZLHIP_OK;
    if (capacity < l.items) return fail(e, ZLHIP_ERR_CAPACITY, "debug_loudness_subs: capacity below the request's sub-blocks");
    std::memcpy(records, e->ld.out.h + l.item_base, (size_t)l.items * sizeof(ZlLdSub));      // (the call has waited: the records are in host memory)
    return ZLHIP_OK;
}

int zlhip_debug_loudness_timings(zlhip_engine *e, float *kernel_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (kernel_ms) *kernel_ms = e->ld.kernelMs;
    return ZLHIP_OK;
}

// ---- loop finder (zl_loop.h, zl_loop.hip) ----------------------------------------------------------------------------------
// Where a clip's sustain loop wraps without a click.  The prep kernel reads the two strips around the nominal points and leaves them
// as int16 with E per candidate; the pairs kernel costs every pair, tile by tile; the pick reduces the tiles and writes the integer
// record into host memory mapped into the device; the three dB values are derived here (zl_lp_finish).  Synchronisation and buffers
// as for the overviews.

int zlhip_loop_resolve(double sample_rate, zlhip_loop_request *r)
{
    if (!r || r->start_frame < 0 || r->stop_frame <= r->start_frame) return ZLHIP_ERR_INVALID;
    zlhip_loop_request q = *r;
    if (zl_lp_resolve(sample_rate, &q.start_search, &q.stop_search, &q.window, &q.min_length) != 0) return ZLHIP_ERR_INVALID;
    *r = q;
    return ZLHIP_OK;
}

int zlhip_loop_seconds(double sample_rate, int64_t start_frame, int64_t stop_frame, float *start_seconds, float *length_seconds)
{
    if (!start_seconds || !length_seconds) return ZLHIP_ERR_INVALID;
    float a, l;
    if (zl_lp_seconds(sample_rate, start_frame, stop_frame, &a, &l) != 0) return ZLHIP_ERR_INVALID;
    *start_seconds = a; *length_seconds = l;
    return ZLHIP_OK;
}

int zlhip_sound_loop_batch(zlhip_engine *e, const zlhip_loop_request *reqs, int32_t nreq, zlhip_loop *out)
{
    static_assert(sizeof(zlhip_loop) == sizeof(ZlLpResult), "the device writes zlhip_loop's layout");
    static_assert(sizeof(zlhip_loop_item) == sizeof(ZlLpItem), "the device writes zlhip_loop_item's layout");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<ZlLpRequest> geo((size_t)nreq);
    int64_t items = 0, strip = 0, cands = 0, cpairs = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_loop_request q = reqs[i];
        { const int rc = check_sound(e, "sound_loop", q.id); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        if (zlhip_loop_resolve(s.sample_rate, &q) != ZLHIP_OK) return fail_in(e, ZLHIP_ERR_INVALID, "sound_loop", kOutsideLimits);
        if (q.stop_frame > s.length) return fail_in(e, ZLHIP_ERR_INVALID, "sound_loop", "the nominal loop does not lie inside the sound's playback data");
        ZlLpRequest &R = geo[(size_t)i];
        std::memset(&R, 0, sizeof R);
        R.s0 = q.start_frame; R.e0 = q.stop_frame; R.window = q.window; R.min_length = q.min_length; R.channels = s.channels;
        zl_lp_range(q.start_frame, q.start_search, q.window >> 1, s.length, &R.smin, &R.ns);
        zl_lp_range(q.stop_frame, q.stop_search, q.window >> 1, s.length, &R.emin, &R.ne);
        if (R.ns == 0 || R.ne == 0) { R.ns = 0; R.ne = 0; }       // an empty range: no candidates at all
        R.cost_base = cpairs; R.item_base = (int32_t)items;
        R.xs_base = (int32_t)strip; R.xe_base = R.xs_base + zl_lp_strip_room(R.ns, R.window);
        R.es_base = (int32_t)cands; R.ee_base = R.es_base + R.ns;
        items += zl_lp_items(R); strip += zl_lp_strip_room(R.ns, R.window) + zl_lp_strip_room(R.ne, R.window);
        cands += R.ns + R.ne; cpairs += (int64_t)R.ns * R.ne;
        if (items > ZL_LP_MAX_CALL_ITEMS) return fail(e, ZLHIP_ERR_INVALID, "sound_loop_batch: more than 65536 work items in one call");
        if (strip > ZL_LP_MAX_CALL_STRIP) return fail(e, ZLHIP_ERR_INVALID, "sound_loop_batch: more than 4194304 strip frames in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Loop &t = e->lp;
    const char *what = "sound_loop: no memory for the call's buffers";
    const bool keep = cpairs <= ZL_LP_MAX_COST_PAIRS;
    const size_t n = (size_t)nreq, ni = (size_t)items, nx = (size_t)strip, nc = (size_t)cands, np = keep ? (size_t)cpairs : 0;
    const int rsv = reserve(e, true, { { ZB_LP_REQ, n, sizeof(ZlLpRequest), std::max<size_t>(n * 2, 64), true, what },
                                      { ZB_LP_X, nx, sizeof(int16_t), std::min<size_t>(std::max<size_t>(nx * 2, 65536), ZL_LP_MAX_CALL_STRIP), false, what },
                                      { ZB_LP_E, nc, sizeof(uint32_t), std::max<size_t>(nc * 2, 8192), false, what },
                                      { ZB_LP_SHIFT, n, sizeof(int32_t), std::max<size_t>(n * 2, 64), false, what },
                                      { ZB_LP_ITEM, ni, sizeof(ZlLpItem), std::min<size_t>(std::max<size_t>(ni * 2, 1024), ZL_LP_MAX_CALL_ITEMS), false, what },
                                      { ZB_LP_COST, np, sizeof(uint32_t), np > 0 ? (size_t)ZL_LP_MAX_COST_PAIRS : 0, false, what } },
                           { mapped_need(t.out, std::max<size_t>(n, 32)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlLpRequest *const hReq = (ZlLpRequest *)e->scratch[ZB_LP_REQ].h, *const dReq = (ZlLpRequest *)e->scratch[ZB_LP_REQ].d;
    int16_t *const dX = (int16_t *)e->scratch[ZB_LP_X].d; uint32_t *const dE = (uint32_t *)e->scratch[ZB_LP_E].d;
    int32_t *const dShift = (int32_t *)e->scratch[ZB_LP_SHIFT].d; ZlLpItem *const dItem = (ZlLpItem *)e->scratch[ZB_LP_ITEM].d;
    uint32_t *const dCost = keep && np > 0 ? (uint32_t *)e->scratch[ZB_LP_COST].d : nullptr;
    t.last.clear();
    t.costs = keep;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlLpRequest &R = hReq[i];
        R = geo[(size_t)i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, e->hc.sounds[reqs[i].id].offset);
        t.last.push_back({R.cost_base, R.item_base, zl_lp_items(R), R.ns, R.ne});
    }
    t.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)nreq * sizeof(ZlLpRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, t.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_loop_prep(dReq, nreq, dX, dE, dShift, e->stream));
    ZL_HIP(e, t.timer.mark(1, e->stream));
    ZL_KERNEL(e, zl_launch_loop_pairs(dReq, nreq, items, dX, dE, dItem, dCost, e->stream));
    ZL_HIP(e, t.timer.mark(2, e->stream));
    ZL_KERNEL(e, zl_launch_loop_pick(dReq, nreq, dX, dE, dShift, dItem, t.out.d, e->stream));
    ZL_HIP(e, t.timer.mark(3, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    float prepMs = 0.0f, pickMs = 0.0f;
    ZL_HIP(e, t.timer.elapsed(0, 1, &prepMs)); ZL_HIP(e, t.timer.elapsed(1, 2, &t.pairsMs)); ZL_HIP(e, t.timer.elapsed(2, 3, &pickMs));
    if (t.timer.on) t.restMs = prepMs + pickMs;
    for (int32_t i = 0; i < nreq; ++i) {
        ZlLpResult r = t.out.h[i];
        zl_lp_finish(&r);
        std::memcpy(&out[i], &r, sizeof(r));
    }
    return ZLHIP_OK;
}

int zlhip_sound_loop(zlhip_engine *e, const zlhip_loop_request *r, zlhip_loop *out) { return zlhip_sound_loop_batch(e, r, 1, out); }

int zlhip_debug_loop_items(zlhip_engine *e, int32_t request, zlhip_loop_item *items, int32_t capacity, int32_t *count)
{
    if (!e || request < 0 || (size_t)request >= e->lp.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Loop::Last &l = e->lp.last[(size_t)request];
    if (count) *count = l.items;
    if (!items) return ZLHIP_OK;
    if (capacity < l.items) return fail(e, ZLHIP_ERR_CAPACITY, "debug_loop_items: capacity below the request's items");
    if (l.items == 0) return ZLHIP_OK;
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(items, (const ZlLpItem *)e->scratch[ZB_LP_ITEM].d + l.item_base, (size_t)l.items * sizeof(ZlLpItem), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_loop_costs(zlhip_engine *e, int32_t request, uint32_t *costs, int32_t capacity, int32_t *starts, int32_t *ends)
{
    if (!e || request < 0 || (size_t)request >= e->lp.last.size()) return ZLHIP_ERR_INVALID;
    if (!e->lp.costs) return fail(e, ZLHIP_ERR_STATE, "debug_loop_costs: the last call had more than 1048576 candidate pairs and stored no costs");
    const zlhip_engine::Loop::Last &l = e->lp.last[(size_t)request];
    if (starts) *starts = l.ns;
    if (ends) *ends = l.ne;
    if (!costs) return ZLHIP_OK;
    const int64_t n = (int64_t)l.ns * l.ne;
    if ((int64_t)capacity < n) return fail(e, ZLHIP_ERR_CAPACITY, "debug_loop_costs: capacity below starts * ends");
    if (n == 0) return ZLHIP_OK;
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(costs, (const uint32_t *)e->scratch[ZB_LP_COST].d + l.cost_base, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_loop_timings(zlhip_engine *e, float *pairs_ms, float *rest_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (pairs_ms) *pairs_ms = e->lp.pairsMs;
    if (rest_ms) *rest_ms = e->lp.restMs;
    return ZLHIP_OK;
}

// ---- loop crossfade (zl_xfade.h, zl_xfade.hip) ---------------------------------------------------------------------------------
// The loop finder chooses among points that exist; this bakes a crossfade into the data, so that the wrap from the loop's last frame to
// its start is the original's own step.  Every applied clip gets a new arena extent (ZlNewExtents), one launch measures the correlation
// of every request's two regions into mapped host memory, the call waits, the weight tables are made here in double from the measured
// or the fixed rho, one launch copies and fades every clip, the sound-table entries switch (ZlClipSwap: a clip whose original lacks
// ZL_SOUND_FINITE starts with its word set), and the call waits a second time.  The new extent becomes the slot's original.
int zlhip_xfade_resolve(double sample_rate, int32_t length, zlhip_xfade_request *r)
{
    if (!r) return ZLHIP_ERR_INVALID;
    int32_t X = r->fade_frames;
    if (zl_xf_resolve(sample_rate, length, r->start_frame, r->stop_frame, &X, r->curve) != 0) return ZLHIP_ERR_INVALID;
    r->fade_frames = X;
    return ZLHIP_OK;
}

int zlhip_xfade_design(int32_t fade_frames, double rho, float *ab)
{
    if (!ab || fade_frames < 1 || fade_frames > ZL_XF_MAX_FADE || !(rho >= 0.0 && rho <= 1.0)) return ZLHIP_ERR_INVALID;
    zl_xf_design(fade_frames, rho, ab);
    return ZLHIP_OK;
}

int zlhip_sound_loop_crossfade_batch(zlhip_engine *e, const zlhip_xfade_request *reqs, int32_t count, zlhip_xfade *out)
{
    static_assert(sizeof(zlhip_xfade) == 64, "zlhip_xfade's layout");
    static_assert(ZLHIP_XFADE_AUTO == ZL_XF_AUTO && ZLHIP_XFADE_LINEAR == ZL_XF_LINEAR && ZLHIP_XFADE_EQUAL_POWER == ZL_XF_EQUAL_POWER, "the curves");
    if (!e || count < 0 || (count > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    // validate and resolve everything before the first HIP call
    std::vector<zlhip_xfade_request> res((size_t)count);
    int32_t njobs = 0;
    {
        ZlDistinct distinct(e);
        int64_t wgs = 0, pairs = 0;
        for (int32_t i = 0; i < count; ++i) {
            zlhip_xfade_request &q = res[(size_t)i];
            q = reqs[i];
            { const int rc = distinct.check(e, "sound_loop_crossfade", q.id); if (rc != ZLHIP_OK) return rc; }
            const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
            if (zlhip_xfade_resolve(o.sample_rate, o.length, &q) != ZLHIP_OK)
                return fail_in(e, ZLHIP_ERR_INVALID, "sound_loop_crossfade", "the loop does not lie inside the sound's data, fade_frames outside 1 .. min(start, stop - start, 65536), or no such curve");
            if (q.fade_frames == 0) continue;
            ZlXfJob J; std::memset(&J, 0, sizeof J);
            J.length = o.length; J.channels = o.channels;
            wgs += zl_xf_job_wgs(J); pairs += q.fade_frames; ++njobs;
        }
        if (wgs > (int64_t)INT32_MAX || pairs > (int64_t)INT32_MAX) return fail(e, ZLHIP_ERR_INVALID, "sound_loop_crossfade_batch: more than 2^31 - 1 workgroups or fade frames in one call");
        for (int32_t i = 0; i < count; ++i) {
            if (res[(size_t)i].fade_frames == 0) continue;
            const int rc = check_plays_original(e, res[(size_t)i].id, "sound_loop_crossfade: the clip plays a re-render (crossfade first, re-render afterwards; re-render it with gain 0, pitch 0, speed 1 first)");
            if (rc != ZLHIP_OK) return rc;
        }
    }
    if (njobs == 0) {                                              // nothing to fade anywhere: no launch, no copy
        std::memset(out, 0, (size_t)count * sizeof(zlhip_xfade));
        return ZLHIP_OK;
    }
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }
    // the new extents and the jobs
    ZlNewExtents ext(e, count);
    ZlClipSwap swap{ e, "sound_loop_crossfade", ext };
    std::vector<ZlXfJob> jobs;
    int32_t wgs = 0, pairs = 0;
    for (int32_t i = 0; i < count; ++i) {
        const zlhip_xfade_request &q = res[(size_t)i];
        if (q.fade_frames == 0) continue;
        const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
        { const int rc = ext.take(i, o.length, o.channels); if (rc != ZLHIP_OK) return rc; }
        ZlXfJob J; std::memset(&J, 0, sizeof J);
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.length = o.length; J.channels = o.channels;
        J.s = q.start_frame; J.e = q.stop_frame; J.X = q.fade_frames;
        J.wg_base = wgs; J.weights = pairs; J.verdict = swap.add(i, q.id, o);
        wgs += zl_xf_job_wgs(J); pairs += J.X;
        jobs.push_back(J);
    }
    const std::vector<int32_t> &jobReq = swap.jobReq;
    const char *what = "sound_loop_crossfade: no memory for the call's records";
    const size_t nj = jobs.size(), n = std::max<size_t>(nj * 2, 64), np = (size_t)pairs;
    zlhip_engine::Xfade &t = e->xf;
    const int rsv = reserve(e, false, { { ZB_XF_JOBS, nj, sizeof(ZlXfJob), n, false, what }, { ZB_XF_WEIGHTS, np, 2 * sizeof(float), std::max<size_t>(np * 2, 4096), false, what },
                                       { ZB_XF_PUB, nj, sizeof(ZlRsPublish), n, false, what }, { ZB_XF_VERDICTS, nj, sizeof(uint32_t), n, false, what } },
                            { mapped_need(t.sums, std::max<size_t>(nj, 32)) });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    ZlXfJob *const dJobs = (ZlXfJob *)e->scratch[ZB_XF_JOBS].d; float *const dWeights = (float *)e->scratch[ZB_XF_WEIGHTS].d;
    ZlRsPublish *const dPub = (ZlRsPublish *)e->scratch[ZB_XF_PUB].d; uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_XF_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call
    t.timer.on = e->profiling;
    int krc = (int)hipMemcpyAsync(dJobs, jobs.data(), nj * sizeof(ZlXfJob), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(0, e->stream);
    if (krc == 0) krc = zl_launch_xfade_measure(dJobs, (int32_t)nj, t.sums.d, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(1, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's first wait: the sums are in host memory
    if (krc != 0) return swap.hip_failed(krc);
    // the tables, from the measured or the fixed rho
    std::vector<zlhip_xfade> results((size_t)count);
    std::memset(results.data(), 0, results.size() * sizeof(zlhip_xfade));
    std::vector<float> weights(np * 2);
    for (size_t j = 0; j < nj; ++j) {
        const zlhip_xfade_request &q = res[(size_t)jobReq[j]];
        const ZlXfSums m = t.sums.h[j];
        zlhip_xfade &r = results[(size_t)jobReq[j]];
        double corr, rho;
        zl_xf_finish(m.sab, m.saa, m.sbb, &corr, &rho);
        r.applied = 1; r.fade_frames = q.fade_frames; r.start_frame = q.start_frame; r.stop_frame = q.stop_frame; r.curve = q.curve;
        r.sab = m.sab; r.saa = m.saa; r.sbb = m.sbb; r.correlation = corr; r.rho = zl_xf_curve_rho(q.curve, rho);
        zl_xf_design(q.fade_frames, r.rho, weights.data() + 2 * (size_t)jobs[j].weights);
    }
    std::vector<uint32_t> verdictsOut(nj, 0u);
    krc = (int)hipMemcpyAsync(dWeights, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dVerdicts, swap.words.data(), nj * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, swap.pub.data(), nj * sizeof(ZlRsPublish), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(2, e->stream);
    if (krc == 0) krc = zl_launch_xfade_render(dJobs, (int32_t)nj, wgs, dWeights, dVerdicts, e->stream);
    if (krc == 0) krc = zl_launch_resample_publish(dPub, (int32_t)nj, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(3, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdictsOut.data(), dVerdicts, nj * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's second wait
    if (krc == 0) krc = (int)t.timer.elapsed(0, 1, &t.measureMs);
    if (krc == 0) krc = (int)t.timer.elapsed(2, 3, &t.renderMs);
    if (krc != 0) return swap.hip_failed(krc);
    swap.commit(verdictsOut);
    std::memcpy(out, results.data(), results.size() * sizeof(zlhip_xfade));
    return ZLHIP_OK;
}

int zlhip_sound_loop_crossfade(zlhip_engine *e, const zlhip_xfade_request *r, zlhip_xfade *out) { return zlhip_sound_loop_crossfade_batch(e, r, 1, out); }

int zlhip_debug_xfade_timings(zlhip_engine *e, float *measure_ms, float *render_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (measure_ms) *measure_ms = e->xf.measureMs;
    if (render_ms) *render_ms = e->xf.renderMs;
    return ZLHIP_OK;
}

// ---- clip edit (zl_edit.h, zl_edit.hip) -----------------------------------------------------------------------------------------
// Crop, trim silence, reverse, fade the ends: the clip's data changes under its own id.  The order is the loop crossfade's, but for the
// extents: a trimmed clip's new length is known only behind the scan, so the scan launch and the call's first wait come first -- the
// scan writes nothing but its own words, so that an arena that cannot hold the call still leaves every clip as it was -- and only
// then every applied clip gets its new extent (ZlNewExtents), the weight tables are made here in double, one launch copies and fades
// every clip, the sound-table entries switch (ZlClipSwap) and the call waits a last time.  A call without a TRIM request skips the
// scan and its wait.  The new extent becomes the slot's original.
int zlhip_edit_resolve(int32_t length, zlhip_edit_request *r)
{
    static_assert(sizeof(zlhip_edit_request) == 40 && sizeof(zlhip_edit_request) == sizeof(ZlEdRequest), "zlhip_edit_request's layout");
    if (!r) return ZLHIP_ERR_INVALID;
    ZlEdRequest q;
    std::memcpy(&q, r, sizeof q);
    if (zl_ed_resolve(length, &q) != 0) return ZLHIP_ERR_INVALID;
    std::memcpy(r, &q, sizeof q);
    return ZLHIP_OK;
}

int zlhip_edit_design(int32_t fade_frames, int32_t curve, float *w)
{
    if (!w || fade_frames < 1 || (curve != ZL_ED_LINEAR && curve != ZL_ED_SQRT && curve != ZL_ED_SMOOTH)) return ZLHIP_ERR_INVALID;
    zl_ed_design(fade_frames, curve, w);
    return ZLHIP_OK;
}

int zlhip_sound_edit_batch(zlhip_engine *e, const zlhip_edit_request *reqs, int32_t count, zlhip_edit *out)
{
    static_assert(sizeof(zlhip_edit) == 48, "zlhip_edit's layout");
    static_assert(ZLHIP_EDIT_TRIM == ZL_ED_TRIM && ZLHIP_EDIT_REVERSE == ZL_ED_REVERSE, "the flags");
    static_assert(ZLHIP_EDIT_LINEAR == ZL_ED_LINEAR && ZLHIP_EDIT_SQRT == ZL_ED_SQRT && ZLHIP_EDIT_SMOOTH == ZL_ED_SMOOTH, "the curves");
    if (!e || count < 0 || (count > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    // validate and resolve everything before the first HIP call
    std::vector<zlhip_edit_request> res((size_t)count);
    std::vector<ZlEdScan> scans; std::vector<int32_t> scanReq;
    int32_t scanWgs = 0;
    const char *const refusal = "sound_edit: the clip plays a re-render (edit first, re-render afterwards; re-render it with gain 0, pitch 0, speed 1 first)";
    {
        ZlDistinct distinct(e);
        int64_t wgs = 0, swgs = 0, fades = 0;                      // (the render's workgroups and weights: what the asked regions need at most)
        for (int32_t i = 0; i < count; ++i) {
            zlhip_edit_request &q = res[(size_t)i];
            q = reqs[i];
            { const int rc = distinct.check(e, "sound_edit", q.id); if (rc != ZLHIP_OK) return rc; }
            const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
            if (zlhip_edit_resolve(o.length, &q) != ZLHIP_OK)
                return fail_in(e, ZLHIP_ERR_INVALID, "sound_edit", "the region does not lie inside the sound's data, an unknown flag or curve, a negative count of frames, or a threshold that is not finite and above 0");
            ZlEdJob J; std::memset(&J, 0, sizeof J);
            J.n = q.num_frames; J.channels = o.channels;
            wgs += zl_ed_job_wgs(J); fades += (int64_t)(q.num_frames / 2) * 2;
            if (q.flags & ZL_ED_TRIM) {
                ZlEdScan S; std::memset(&S, 0, sizeof S);
                S.channels = o.channels; S.a = q.first_frame; S.b = q.first_frame + q.num_frames; S.threshold = q.threshold;
                S.wg_base = (int32_t)swgs; S.found = (int32_t)scans.size();
                swgs += zl_ed_scan_wgs(S);
                scans.push_back(S); scanReq.push_back(i);
            }
        }
        if (wgs > (int64_t)INT32_MAX || swgs > (int64_t)INT32_MAX || fades > (int64_t)INT32_MAX)
            return fail(e, ZLHIP_ERR_INVALID, "sound_edit_batch: more than 2^31 - 1 workgroups or fade frames in one call");
        scanWgs = (int32_t)swgs;
        for (int32_t i = 0; i < count; ++i) {                      // (a request that is the identity whatever the scan finds touches nothing)
            const zlhip_edit_request &q = res[(size_t)i];
            const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
            int32_t Xi, Xo;
            zl_ed_fades(q.num_frames, q.fade_in_frames, q.fade_out_frames, &Xi, &Xo);
            if (!(q.flags & ZL_ED_TRIM) && zl_ed_identity(o.length, q.first_frame, q.num_frames, (q.flags & ZL_ED_REVERSE) != 0, Xi, Xo)) continue;
            const int rc = check_plays_original(e, q.id, refusal);
            if (rc != ZLHIP_OK) return rc;
        }
    }
    zlhip_engine::Edit &t = e->ed;
    t.timer.on = e->profiling;
    if (e->profiling) { t.scanMs = 0.0f; t.renderMs = 0.0f; }
    const char *what = "sound_edit: no memory for the call's records";
    bool begun = false;
    // the scan: F and Z of every TRIM request
    std::vector<ZlEdFound> found(scans.size(), ZlEdFound{ INT32_MAX, -1 });
    if (!scans.empty()) {
        { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }
        begun = true;
        const size_t ns = scans.size(), n = std::max<size_t>(ns * 2, 64);
        const int rsv = reserve(e, false, { { ZB_ED_SCAN, ns, sizeof(ZlEdScan), n, false, what }, { ZB_ED_FOUND, ns, sizeof(ZlEdFound), n, false, what } });
        if (rsv != ZLHIP_OK) return rsv;
        ZlEdScan *const dScan = (ZlEdScan *)e->scratch[ZB_ED_SCAN].d; ZlEdFound *const dFound = (ZlEdFound *)e->scratch[ZB_ED_FOUND].d;
        for (size_t k = 0; k < ns; ++k) scans[k].src = (uint64_t)(uintptr_t)arena_ptr(e, e->soundSlots[(size_t)res[(size_t)scanReq[k]].id].orig.offset);
        int krc = (int)hipMemcpyAsync(dScan, scans.data(), ns * sizeof(ZlEdScan), hipMemcpyHostToDevice, e->stream);
        if (krc == 0) krc = (int)hipMemcpyAsync(dFound, found.data(), ns * sizeof(ZlEdFound), hipMemcpyHostToDevice, e->stream);
        if (krc == 0) krc = (int)t.timer.mark(0, e->stream);
        if (krc == 0) krc = zl_launch_edit_scan(dScan, (int32_t)ns, scanWgs, dFound, e->stream);
        if (krc == 0) krc = (int)t.timer.mark(1, e->stream);
        if (krc == 0) krc = (int)hipMemcpyAsync(found.data(), dFound, ns * sizeof(ZlEdFound), hipMemcpyDeviceToHost, e->stream);
        if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);  // the call's first wait: F and Z are in host memory
        if (krc == 0) krc = (int)t.timer.elapsed(0, 1, &t.scanMs);
        if (krc != 0) {                                            // (the scan has changed nothing: nothing to undo)
            e->err = std::string("sound_edit: ") + hipGetErrorString((hipError_t)krc);
            (void)hipStreamSynchronize(e->stream);
            return ZLHIP_ERR_HIP;
        }
    }
    // the regions, from F and Z
    std::vector<zlhip_edit> results((size_t)count);
    std::vector<ZlEdJob> plan((size_t)count);                      // per request; n = 0: not applied
    std::memset(plan.data(), 0, plan.size() * sizeof(ZlEdJob));
    int32_t njobs = 0;
    for (int32_t i = 0, k = 0; i < count; ++i) {
        const zlhip_edit_request &q = res[(size_t)i];
        const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
        const bool trim = (q.flags & ZL_ED_TRIM) != 0, reverse = (q.flags & ZL_ED_REVERSE) != 0;
        const ZlEdFound f = trim ? found[(size_t)k++] : ZlEdFound{ INT32_MAX, -1 };
        zlhip_edit &r = results[(size_t)i];
        std::memset(&r, 0, sizeof r);
        r.curve = q.curve; r.first_loud = -1; r.last_loud = -1;
        int32_t a2, b2, Xi = 0, Xo = 0;
        if (!zl_ed_region(q.first_frame, q.first_frame + q.num_frames, trim, f.first, f.last, q.pre_roll_frames, q.hold_frames, &a2, &b2)) {
            r.silent = 1; r.first_frame = q.first_frame; r.num_frames = q.num_frames; r.length = o.length;
            continue;
        }
        if (trim) { r.first_loud = f.first; r.last_loud = f.last; }
        zl_ed_fades(b2 - a2, q.fade_in_frames, q.fade_out_frames, &Xi, &Xo);
        r.first_frame = a2; r.num_frames = b2 - a2; r.length = b2 - a2;
        if (zl_ed_identity(o.length, a2, b2 - a2, reverse, Xi, Xo)) continue;
        r.applied = 1; r.fade_in_frames = Xi; r.fade_out_frames = Xo; r.reversed = reverse ? 1 : 0;
        ZlEdJob &J = plan[(size_t)i];
        J.channels = o.channels; J.a = a2; J.n = b2 - a2; J.reverse = reverse ? 1 : 0; J.Xi = Xi; J.Xo = Xo;
        ++njobs;
    }
    if (njobs == 0) {                                              // nothing to change anywhere: no extent, no copy, no render
        std::memcpy(out, results.data(), results.size() * sizeof(zlhip_edit));
        return ZLHIP_OK;
    }
    if (!begun) { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }
    // only now the new extents, and the jobs
    ZlNewExtents ext(e, count);
    ZlClipSwap swap{ e, "sound_edit", ext };
    std::vector<ZlEdJob> jobs;
    int32_t wgs = 0, nw = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (plan[(size_t)i].n == 0) continue;
        const ZlSound &o = e->soundSlots[(size_t)res[(size_t)i].id].orig;
        ZlEdJob J = plan[(size_t)i];
        { const int rc = ext.take(i, J.n, o.channels); if (rc != ZLHIP_OK) return rc; }
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.wg_base = wgs; J.w_in = nw; J.w_out = nw + J.Xi;
        ZlSound s = o; s.length = J.n;
        J.verdict = swap.add(i, res[(size_t)i].id, s);
        wgs += zl_ed_job_wgs(J); nw += J.Xi + J.Xo;
        jobs.push_back(J);
    }
    const size_t nj = jobs.size(), n = std::max<size_t>(nj * 2, 64), np = (size_t)nw;
    const int rsv = reserve(e, false, { { ZB_ED_JOBS, nj, sizeof(ZlEdJob), n, false, what }, { ZB_ED_WEIGHTS, np, sizeof(float), std::max<size_t>(np * 2, 4096), false, what },
                                       { ZB_ED_PUB, nj, sizeof(ZlRsPublish), n, false, what }, { ZB_ED_VERDICTS, nj, sizeof(uint32_t), n, false, what } });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    ZlEdJob *const dJobs = (ZlEdJob *)e->scratch[ZB_ED_JOBS].d; float *const dWeights = (float *)e->scratch[ZB_ED_WEIGHTS].d;
    ZlRsPublish *const dPub = (ZlRsPublish *)e->scratch[ZB_ED_PUB].d; uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_ED_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call.  The tables
    std::vector<float> weights(np);
    for (size_t j = 0; j < nj; ++j) {
        const int32_t curve = res[(size_t)swap.jobReq[j]].curve;
        zl_ed_design(jobs[j].Xi, curve, weights.data() + jobs[j].w_in);
        zl_ed_design(jobs[j].Xo, curve, weights.data() + jobs[j].w_out);
    }
    std::vector<uint32_t> verdictsOut(nj, 0u);
    int krc = (int)hipMemcpyAsync(dJobs, jobs.data(), nj * sizeof(ZlEdJob), hipMemcpyHostToDevice, e->stream);
    if (krc == 0 && np > 0) krc = (int)hipMemcpyAsync(dWeights, weights.data(), np * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dVerdicts, swap.words.data(), nj * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, swap.pub.data(), nj * sizeof(ZlRsPublish), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(2, e->stream);
    if (krc == 0) krc = zl_launch_edit_render(dJobs, (int32_t)nj, wgs, dWeights, dVerdicts, e->stream);
    if (krc == 0) krc = zl_launch_resample_publish(dPub, (int32_t)nj, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(3, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdictsOut.data(), dVerdicts, nj * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's last wait
    if (krc == 0) krc = (int)t.timer.elapsed(2, 3, &t.renderMs);
    if (krc != 0) return swap.hip_failed(krc);
    swap.commit(verdictsOut);
    std::memcpy(out, results.data(), results.size() * sizeof(zlhip_edit));
    return ZLHIP_OK;
}

int zlhip_sound_edit(zlhip_engine *e, const zlhip_edit_request *r, zlhip_edit *out) { return zlhip_sound_edit_batch(e, r, 1, out); }

int zlhip_debug_edit_timings(zlhip_engine *e, float *scan_ms, float *render_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (scan_ms) *scan_ms = e->ed.scanMs;
    if (render_ms) *render_ms = e->ed.renderMs;
    return ZLHIP_OK;
}

// ---- peaks and limiter (zl_limit.h, zl_limit.hip) -----------------------------------------------------------------------------------
// The analysis is the loudness measurement's shape: one launch that writes a record per chunk into mapped host memory, one wait, the
// maxima taken here; the resident real-time kernel stays.  The limiter is the clip edit's order: the detecting launch -- the same kernel,
// over the originals, into a device buffer the render reads -- and the call's first wait come first and write nothing but their own
// records, so that an arena that cannot hold the call leaves every clip as it was; only then every applied clip gets its new extent,
// the windows are made here, one launch renders every clip, the sound-table entries switch and the call waits a last time.
static void lm_tables(zlhip_engine *e)
{
    if (e->lm.tables.empty()) { e->lm.tables.resize(ZL_LM_TABLE_FLOATS); zl_lm_tables(e->lm.tables.data()); }
}

int zlhip_peak_resolve(double sample_rate, int32_t length, const zlhip_peak_request *r)
{
    static_assert(sizeof(zlhip_peak_request) == 16 && sizeof(zlhip_peak_request) == sizeof(ZlLmPeakRequest), "zlhip_peak_request's layout");
    if (!r) return ZLHIP_ERR_INVALID;
    ZlLmPeakRequest q;
    std::memcpy(&q, r, sizeof q);
    return zl_lm_peak_resolve(sample_rate, length, &q) != 0 ? ZLHIP_ERR_INVALID : ZLHIP_OK;
}

int zlhip_sound_peak_batch(zlhip_engine *e, const zlhip_peak_request *reqs, int32_t nreq, zlhip_peak *out)
{
    static_assert(sizeof(zlhip_peak) == 24, "zlhip_peak's layout");
    static_assert(sizeof(zlhip_peak_chunk) == sizeof(ZlLmRecord) && sizeof(ZlLmRecord) == 16, "the device writes zlhip_peak_chunk's layout");
    static_assert(ZLHIP_LIMIT_TRUE_PEAK == ZL_LM_TRUE_PEAK, "the flag");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate everything before anything is written and before the first HIP call
    std::vector<ZlLmScan> geo((size_t)nreq);
    int64_t chunks = 0;
    bool anyTp = false;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_peak_request q = reqs[i];
        auto resolve = [&](const ZlSound &s) {
            return (q.flags & ~ZL_LM_TRUE_PEAK) || ((q.flags & ZL_LM_TRUE_PEAK) && !zl_lm_rate_ok(s.sample_rate)) ? "an unknown flag, or the true peak at a rate that is no integer in [1000, 768000]" : nullptr;
        };
        { const int rc = check_request(e, "sound_peak", q, resolve); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        ZlLmScan &S = geo[(size_t)i];
        std::memset(&S, 0, sizeof S);
        S.channels = s.channels; S.a = q.first_frame; S.b = q.first_frame + q.num_frames; S.wg_base = (int32_t)chunks;
        S.F = (q.flags & ZL_LM_TRUE_PEAK) ? zl_lm_oversampling(s.sample_rate) : 1; S.sanitize = 1; S.gain = 1.0f;
        anyTp = anyTp || S.F > 1;
        chunks += zl_lm_chunks(q.num_frames);
        if (chunks > ZL_LM_MAX_CALL_CHUNKS) return fail(e, ZLHIP_ERR_INVALID, "sound_peak_batch: more than 4194304 chunks in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Limit &t = e->lm;
    const size_t n = (size_t)nreq;
    const char *what = "sound_peak: no memory for the call's buffers";
    const int rsv = reserve(e, true, { { ZB_LM_SCAN, n, sizeof(ZlLmScan), std::max<size_t>(n * 2, 64), true, what },
                                       { ZB_LM_TABLES, ZL_LM_TABLE_FLOATS, sizeof(float), ZL_LM_TABLE_FLOATS, true, what } },
                            { mapped_need(t.out, std::max<size_t>((size_t)chunks, 512)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlLmScan *const hReq = (ZlLmScan *)e->scratch[ZB_LM_SCAN].h, *const dReq = (ZlLmScan *)e->scratch[ZB_LM_SCAN].d;
    float *const hTab = (float *)e->scratch[ZB_LM_TABLES].h, *const dTab = (float *)e->scratch[ZB_LM_TABLES].d;
    t.last.clear();
    for (int32_t i = 0; i < nreq; ++i) {
        hReq[i] = geo[(size_t)i];
        hReq[i].src = (uint64_t)(uintptr_t)arena_ptr(e, e->hc.sounds[reqs[i].id].offset);
        t.last.push_back({ geo[(size_t)i].wg_base, zl_lm_chunks(geo[(size_t)i].b - geo[(size_t)i].a) });
    }
    t.peakTimer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, n * sizeof(ZlLmScan), hipMemcpyHostToDevice, e->stream));
    if (anyTp) {
        lm_tables(e);
        std::memcpy(hTab, t.tables.data(), ZL_LM_TABLE_FLOATS * sizeof(float));
        ZL_HIP(e, hipMemcpyAsync(dTab, hTab, ZL_LM_TABLE_FLOATS * sizeof(float), hipMemcpyHostToDevice, e->stream));
    }
    ZL_HIP(e, t.peakTimer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_limit_detect(dReq, nreq, (int32_t)chunks, dTab, t.out.d, e->stream));
    ZL_HIP(e, t.peakTimer.mark(1, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, t.peakTimer.elapsed(0, 1, &t.peakMs));
    for (int32_t i = 0; i < nreq; ++i) {
        const ZlLmScan &S = geo[(size_t)i];
        uint32_t m[4] = {0u, 0u, 0u, 0u};
        const int32_t nc = zl_lm_chunks(S.b - S.a);
        for (int32_t k = 0; k < nc; ++k) {
            const ZlLmRecord &r = t.out.h[S.wg_base + k];
            m[0] = zl_lm_max_bits(m[0], zl_lm_bits(r.sample_peak[0])); m[1] = zl_lm_max_bits(m[1], zl_lm_bits(r.sample_peak[1]));
            m[2] = zl_lm_max_bits(m[2], zl_lm_bits(r.inter_peak[0])); m[3] = zl_lm_max_bits(m[3], zl_lm_bits(r.inter_peak[1]));
        }
        zlhip_peak &o = out[i];
        o.sample_peak[0] = zl_lm_float(m[0]); o.sample_peak[1] = zl_lm_float(m[1]);
        o.true_peak[0] = zl_lm_float(zl_lm_max_bits(m[0], m[2])); o.true_peak[1] = zl_lm_float(zl_lm_max_bits(m[1], m[3]));
        o.oversampling = S.F; o.chunks = nc;
    }
    return ZLHIP_OK;
}

int zlhip_sound_peak(zlhip_engine *e, const zlhip_peak_request *r, zlhip_peak *out) { return zlhip_sound_peak_batch(e, r, 1, out); }

int zlhip_debug_peak_chunks(zlhip_engine *e, int32_t request, zlhip_peak_chunk *records, int32_t capacity, int32_t *count)
{
    if (!e || request < 0 || (size_t)request >= e->lm.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Limit::Last &l = e->lm.last[(size_t)request];
    if (count) *count = l.chunks;
    if (!records) return ZLHIP_OK;
    if (capacity < l.chunks) return fail(e, ZLHIP_ERR_CAPACITY, "debug_peak_chunks: capacity below the request's chunks");
    std::memcpy(records, e->lm.out.h + l.rec_base, (size_t)l.chunks * sizeof(ZlLmRecord));      // (the call has waited: the records are in host memory)
    return ZLHIP_OK;
}

int zlhip_limit_resolve(double sample_rate, zlhip_limit_request *r)
{
    static_assert(sizeof(zlhip_limit_request) == 24 && sizeof(zlhip_limit_request) == sizeof(ZlLmRequest), "zlhip_limit_request's layout");
    if (!r) return ZLHIP_ERR_INVALID;
    ZlLmRequest q;
    std::memcpy(&q, r, sizeof q);
    if (zl_lm_resolve(sample_rate, &q) != 0) return ZLHIP_ERR_INVALID;
    std::memcpy(r, &q, sizeof q);
    return ZLHIP_OK;
}

int zlhip_limit_design(int32_t lookahead_frames, float *w)
{
    if (!w || lookahead_frames < 1 || lookahead_frames > ZL_LM_MAX_L) return ZLHIP_ERR_INVALID;
    zl_lm_design(lookahead_frames, w);
    return ZLHIP_OK;
}

int zlhip_sound_limit_batch(zlhip_engine *e, const zlhip_limit_request *reqs, int32_t count, zlhip_limit *out)
{
    static_assert(sizeof(zlhip_limit) == 40, "zlhip_limit's layout");
    if (!e || count < 0 || (count > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    // validate and resolve everything before the first HIP call
    std::vector<zlhip_limit_request> res((size_t)count);
    std::vector<ZlLmScan> scans((size_t)count);
    int32_t scanWgs = 0;
    bool anyTp = false;
    {
        ZlDistinct distinct(e);
        int64_t swgs = 0, tiles = 0;
        for (int32_t i = 0; i < count; ++i) {
            zlhip_limit_request &q = res[(size_t)i];
            q = reqs[i];
            { const int rc = distinct.check(e, "sound_limit", q.id); if (rc != ZLHIP_OK) return rc; }
            const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
            if (zlhip_limit_resolve(o.sample_rate, &q) != ZLHIP_OK)
                return fail_in(e, ZLHIP_ERR_INVALID, "sound_limit", "an unknown flag, the true peak at a rate that is no integer in [1000, 768000], a ceiling outside (0, 1], a gain that is not finite and above 0, or lookahead_frames or hold_frames outside [0, 512]");
            ZlLmScan &S = scans[(size_t)i];
            std::memset(&S, 0, sizeof S);
            S.channels = o.channels; S.a = 0; S.b = o.length; S.wg_base = (int32_t)swgs;
            S.F = (q.flags & ZL_LM_TRUE_PEAK) ? zl_lm_oversampling(o.sample_rate) : 1; S.sanitize = 0; S.gain = q.gain;
            anyTp = anyTp || S.F > 1;
            ZlLmJob J; std::memset(&J, 0, sizeof J);
            J.n = o.length; J.channels = o.channels;
            swgs += zl_lm_chunks(o.length); tiles += zl_lm_job_tiles(J);
            if (swgs > ZL_LM_MAX_CALL_CHUNKS || tiles > (int64_t)INT32_MAX) return fail(e, ZLHIP_ERR_INVALID, "sound_limit_batch: more than 4194304 chunks in one call");
        }
        scanWgs = (int32_t)swgs;
        for (int32_t i = 0; i < count; ++i) {
            const int rc = check_plays_original(e, res[(size_t)i].id, "sound_limit: the clip plays a re-render (limit first, re-render afterwards; re-render it with gain 0, pitch 0, speed 1 first)");
            if (rc != ZLHIP_OK) return rc;
        }
        for (int32_t i = 0; i < count; ++i) {
            if (!(e->soundSlots[(size_t)res[(size_t)i].id].orig.flags & ZL_SOUND_FINITE))
                return fail(e, ZLHIP_ERR_STATE, "sound_limit: the clip holds a sample that is not finite (the limiter needs a finite detector)");
        }
    }
    zlhip_engine::Limit &t = e->lm;
    t.timer.on = e->profiling;
    if (e->profiling) { t.detectMs = 0.0f; t.renderMs = 0.0f; }
    const char *what = "sound_limit: no memory for the call's records";
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }
    const size_t nq = (size_t)count;
    {
        const int rsv = reserve(e, false, { { ZB_LM_SCAN, nq, sizeof(ZlLmScan), std::max<size_t>(nq * 2, 64), true, what },
                                            { ZB_LM_TABLES, ZL_LM_TABLE_FLOATS, sizeof(float), ZL_LM_TABLE_FLOATS, true, what },
                                            { ZB_LM_REC, (size_t)scanWgs, sizeof(ZlLmRecord), std::max<size_t>((size_t)scanWgs * 2, 512), false, what } });
        if (rsv != ZLHIP_OK) return rsv;
    }
    ZlLmScan *const hScan = (ZlLmScan *)e->scratch[ZB_LM_SCAN].h, *const dScan = (ZlLmScan *)e->scratch[ZB_LM_SCAN].d;
    float *const hTab = (float *)e->scratch[ZB_LM_TABLES].h, *const dTab = (float *)e->scratch[ZB_LM_TABLES].d;
    ZlLmRecord *const dRec = (ZlLmRecord *)e->scratch[ZB_LM_REC].d;
    // the detector over every clip: the chunk records
    std::vector<ZlLmRecord> records((size_t)scanWgs);
    {
        for (int32_t i = 0; i < count; ++i) {
            hScan[i] = scans[(size_t)i];
            hScan[i].src = (uint64_t)(uintptr_t)arena_ptr(e, e->soundSlots[(size_t)res[(size_t)i].id].orig.offset);
        }
        int krc = (int)hipMemcpyAsync(dScan, hScan, nq * sizeof(ZlLmScan), hipMemcpyHostToDevice, e->stream);
        if (krc == 0 && anyTp) {
            lm_tables(e);
            std::memcpy(hTab, t.tables.data(), ZL_LM_TABLE_FLOATS * sizeof(float));
            krc = (int)hipMemcpyAsync(dTab, hTab, ZL_LM_TABLE_FLOATS * sizeof(float), hipMemcpyHostToDevice, e->stream);
        }
        if (krc == 0) krc = (int)t.timer.mark(0, e->stream);
        if (krc == 0) krc = zl_launch_limit_detect(dScan, count, scanWgs, dTab, dRec, e->stream);
        if (krc == 0) krc = (int)t.timer.mark(1, e->stream);
        if (krc == 0) krc = (int)hipMemcpyAsync(records.data(), dRec, records.size() * sizeof(ZlLmRecord), hipMemcpyDeviceToHost, e->stream);
        if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);  // the call's first wait: the records are in host memory
        if (krc == 0) krc = (int)t.timer.elapsed(0, 1, &t.detectMs);
        if (krc != 0) {                                            // (the detector has changed nothing: nothing to undo)
            e->err = std::string("sound_limit: ") + hipGetErrorString((hipError_t)krc);
            (void)hipStreamSynchronize(e->stream);
            return ZLHIP_ERR_HIP;
        }
    }
    // who is applied
    std::vector<zlhip_limit> results((size_t)count);
    std::vector<char> applied((size_t)count, 0);
    int32_t njobs = 0;
    for (int32_t i = 0; i < count; ++i) {
        const zlhip_limit_request &q = res[(size_t)i];
        const ZlLmScan &S = scans[(size_t)i];
        uint32_t peak = 0u;
        for (int32_t k = 0; k < zl_lm_chunks(S.b); ++k) peak = zl_lm_max_bits(peak, zl_lm_record_bits(records[(size_t)(S.wg_base + k)]));
        zlhip_limit &r = results[(size_t)i];
        std::memset(&r, 0, sizeof r);
        r.lookahead_frames = q.lookahead_frames; r.hold_frames = q.hold_frames; r.oversampling = S.F; r.peak_before = zl_lm_float(peak);
        r.min_gain = 1.0f; r.ceiling = q.ceiling; r.gain = q.gain;
        if (q.gain == 1.0f && !(peak > zl_lm_bits(q.ceiling))) continue;
        r.applied = 1; applied[(size_t)i] = 1;
        ++njobs;
    }
    if (njobs == 0) {                                              // every clip is under its ceiling already: no extent, no render
        std::memcpy(out, results.data(), results.size() * sizeof(zlhip_limit));
        return ZLHIP_OK;
    }
    // only now the new extents, and the jobs
    ZlNewExtents ext(e, count);
    ZlClipSwap swap{ e, "sound_limit", ext };
    std::vector<ZlLmJob> jobs;
    std::vector<float> weights;
    std::vector<int32_t> weightsAt((size_t)ZL_LM_MAX_L + 1, -1);  // one window per look-ahead of the call
    int32_t wgs = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (!applied[(size_t)i]) continue;
        const zlhip_limit_request &q = res[(size_t)i];
        const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
        { const int rc = ext.take(i, o.length, o.channels); if (rc != ZLHIP_OK) return rc; }
        ZlLmJob J; std::memset(&J, 0, sizeof J);
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.channels = o.channels; J.n = o.length; J.L = q.lookahead_frames; J.H = q.hold_frames; J.F = scans[(size_t)i].F;
        J.ceiling = q.ceiling; J.gain = q.gain; J.wg_base = wgs; J.rec_base = scans[(size_t)i].wg_base;
        if (weightsAt[(size_t)J.L] < 0) {
            weightsAt[(size_t)J.L] = (int32_t)weights.size();
            weights.resize(weights.size() + (size_t)J.L + 1);
            zl_lm_design(J.L, weights.data() + weightsAt[(size_t)J.L]);
        }
        J.weights = weightsAt[(size_t)J.L];
        J.verdict = swap.add(i, q.id, o);
        wgs += zl_lm_job_tiles(J);
        jobs.push_back(J);
    }
    const size_t nj = jobs.size(), n = std::max<size_t>(nj * 2, 64), np = weights.size();
    const int rsv = reserve(e, false, { { ZB_LM_JOBS, nj, sizeof(ZlLmJob), n, false, what }, { ZB_LM_WEIGHTS, np, sizeof(float), std::max<size_t>(np * 2, 4096), false, what },
                                       { ZB_LM_STATS, nj, sizeof(ZlLmStats), n, false, what }, { ZB_LM_PUB, nj, sizeof(ZlRsPublish), n, false, what },
                                       { ZB_LM_VERDICTS, nj, sizeof(uint32_t), n, false, what } });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    ZlLmJob *const dJobs = (ZlLmJob *)e->scratch[ZB_LM_JOBS].d; float *const dWeights = (float *)e->scratch[ZB_LM_WEIGHTS].d;
    ZlLmStats *const dStats = (ZlLmStats *)e->scratch[ZB_LM_STATS].d;
    ZlRsPublish *const dPub = (ZlRsPublish *)e->scratch[ZB_LM_PUB].d; uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_LM_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call
    std::vector<ZlLmStats> stats(nj, ZlLmStats{ 0u, 0x3f800000u });
    std::vector<uint32_t> verdictsOut(nj, 0u);
    int krc = (int)hipMemcpyAsync(dJobs, jobs.data(), nj * sizeof(ZlLmJob), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dWeights, weights.data(), np * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dStats, stats.data(), nj * sizeof(ZlLmStats), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dVerdicts, swap.words.data(), nj * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, swap.pub.data(), nj * sizeof(ZlRsPublish), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(2, e->stream);
    if (krc == 0) krc = zl_launch_limit_render(dJobs, (int32_t)nj, wgs, dTab, dRec, dWeights, dStats, dVerdicts, e->stream);
    if (krc == 0) krc = zl_launch_resample_publish(dPub, (int32_t)nj, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(3, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdictsOut.data(), dVerdicts, nj * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(stats.data(), dStats, nj * sizeof(ZlLmStats), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's last wait
    if (krc == 0) krc = (int)t.timer.elapsed(2, 3, &t.renderMs);
    if (krc != 0) return swap.hip_failed(krc);
    swap.commit(verdictsOut);
    for (size_t j = 0; j < nj; ++j) {
        zlhip_limit &r = results[(size_t)swap.jobReq[j]];
        r.frames_reduced = (int32_t)stats[j].frames_reduced; r.min_gain = zl_lm_float(stats[j].min_gain_bits);
    }
    std::memcpy(out, results.data(), results.size() * sizeof(zlhip_limit));
    return ZLHIP_OK;
}

int zlhip_sound_limit(zlhip_engine *e, const zlhip_limit_request *r, zlhip_limit *out) { return zlhip_sound_limit_batch(e, r, 1, out); }

int zlhip_debug_limit_timings(zlhip_engine *e, float *detect_ms, float *render_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (detect_ms) *detect_ms = e->lm.detectMs;
    if (render_ms) *render_ms = e->lm.renderMs;
    return ZLHIP_OK;
}

// ---- warp (zl_warp.h, zl_warp.hip) ------------------------------------------------------------------------------------------------
// A clip fitted to the session grid: a time stretch cut at the clip's hits.  Every applied clip gets a new arena extent (ZlNewExtents),
// one copy each carries the call's job records, region records and seek list, one launch finds the seek offsets of every stretched
// region of the call (a workgroup each), one synthesises every extent, the sound-table entries switch (ZlClipSwap), and the call waits
// once.  The new extent becomes the slot's original.
int zlhip_warp_resolve(double sample_rate, int32_t length, const zlhip_warp_anchor *anchors, int32_t count, zlhip_warp *summary)
{
    static_assert(sizeof(zlhip_warp) == sizeof(ZlWpSummary) && sizeof(zlhip_warp_anchor) == sizeof(ZlWpAnchor), "the warp's records");
    static_assert(ZLHIP_WARP_MAX_ANCHORS == ZL_WP_MAX_ANCHORS, "the anchor limit");
    if (!anchors || !summary) return ZLHIP_ERR_INVALID;
    ZlWpSummary s;
    if (zl_wp_resolve(sample_rate, length, (const ZlWpAnchor *)anchors, count, &s, nullptr) != 0) return ZLHIP_ERR_INVALID;
    std::memcpy(summary, &s, sizeof s);
    return ZLHIP_OK;
}

int zlhip_warp_plan(double sample_rate, int32_t length, const int32_t *onset_frames, int32_t n, double src_bpm, double dst_bpm, int32_t steps_per_beat,
                    double strength, int32_t origin_frame, int32_t preroll_frames, zlhip_warp_anchor *anchors_out, int32_t capacity, int32_t *count, int32_t *dropped)
{
    if (capacity < 0) return ZLHIP_ERR_INVALID;
    int32_t c = 0, d = 0;
    // (planned into a buffer of its own: on any error the caller's is not written)
    std::vector<ZlWpAnchor> tmp((size_t)std::max(capacity, 2));
    const int rc = zl_wp_plan(sample_rate, length, onset_frames, n, src_bpm, dst_bpm, steps_per_beat, strength, origin_frame, preroll_frames,
                              anchors_out ? tmp.data() : nullptr, capacity, &c, &d);
    if (rc != 0) return rc == -2 ? ZLHIP_ERR_CAPACITY : ZLHIP_ERR_INVALID;
    std::memcpy(anchors_out, tmp.data(), (size_t)c * sizeof(ZlWpAnchor));
    if (count) *count = c;
    if (dropped) *dropped = d;
    return ZLHIP_OK;
}

int64_t zlhip_warp_map(const zlhip_warp_anchor *anchors, int32_t count, int64_t src_frame)
{
    if (!anchors || count < 2) return -1;
    return zl_wp_map((const ZlWpAnchor *)anchors, count, src_frame);
}

int zlhip_sound_warp_batch(zlhip_engine *e, const zlhip_warp_request *reqs, int32_t count, zlhip_warp *out)
{
    static_assert(sizeof(zlhip_warp) == 24 && sizeof(zlhip_warp_anchor) == 8 && sizeof(zlhip_warp_request) == 16, "the warp's layouts");
    if (!e || count < 0 || (count > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    // validate and resolve everything before the first HIP call
    std::vector<ZlWpSummary> sums((size_t)count);
    std::vector<std::vector<ZlWpRegion>> regs((size_t)count);
    int32_t njobs = 0;
    {
        ZlDistinct distinct(e);
        int64_t wgs = 0, nreg = 0, nseg = 0;
        for (int32_t i = 0; i < count; ++i) {
            const zlhip_warp_request &q = reqs[i];
            { const int rc = distinct.check(e, "sound_warp", q.id); if (rc != ZLHIP_OK) return rc; }
            const ZlSound &o = e->soundSlots[(size_t)q.id].orig;
            regs[(size_t)i].resize((size_t)(q.count > 1 && q.count <= ZL_WP_MAX_ANCHORS ? q.count - 1 : 0));
            if (!q.anchors || zl_wp_resolve(o.sample_rate, o.length, (const ZlWpAnchor *)q.anchors, q.count, &sums[(size_t)i], regs[(size_t)i].data()) != 0)
                return fail_in(e, ZLHIP_ERR_INVALID, "sound_warp", "the anchors do not start at (0, 0) and end at the sound's length, are not strictly increasing, or a region is outside its limits");
            if (!sums[(size_t)i].applied) continue;
            ZlWpJob J; std::memset(&J, 0, sizeof J);
            J.N = sums[(size_t)i].length; J.channels = o.channels;
            wgs += zl_wp_job_wgs(J); nreg += sums[(size_t)i].regions; nseg += sums[(size_t)i].segments; ++njobs;
        }
        if (wgs > (int64_t)INT32_MAX || nreg > (int64_t)INT32_MAX || nseg > (int64_t)INT32_MAX)
            return fail(e, ZLHIP_ERR_INVALID, "sound_warp_batch: more than 2^31 - 1 workgroups, regions or segments in one call");
        for (int32_t i = 0; i < count; ++i) {
            if (!sums[(size_t)i].applied) continue;
            const int rc = check_plays_original(e, reqs[i].id, "sound_warp: the clip plays a re-render (warp first, then tune and level; re-render it with gain 0, pitch 0, speed 1 first)");
            if (rc != ZLHIP_OK) return rc;
        }
    }
    if (njobs == 0) {                                              // the identity everywhere: no launch, no copy
        std::memcpy(out, sums.data(), (size_t)count * sizeof(zlhip_warp));
        return ZLHIP_OK;
    }
    { const int rc = call_begin(e, true); if (rc != ZLHIP_OK) return rc; }
    // the new extents and the jobs
    ZlNewExtents ext(e, count);
    ZlClipSwap swap{ e, "sound_warp", ext };
    std::vector<ZlWpJob> jobs; std::vector<ZlWpRegion> table; std::vector<int32_t> seekList;
    int32_t wgs = 0, offs = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (!sums[(size_t)i].applied) continue;
        const ZlSound &o = e->soundSlots[(size_t)reqs[i].id].orig;
        { const int rc = ext.take(i, sums[(size_t)i].length, o.channels); if (rc != ZLHIP_OK) return rc; }
        ZlWpJob J; std::memset(&J, 0, sizeof J);
        J.src = (uint64_t)(uintptr_t)arena_ptr(e, o.offset);
        J.dst = (uint64_t)(uintptr_t)ext.ptr(i);
        J.len = o.length; J.channels = o.channels; J.N = sums[(size_t)i].length; J.O = sums[(size_t)i].overlap;
        J.region_base = (int32_t)table.size(); J.nregions = sums[(size_t)i].regions;
        J.wg_base = wgs;
        ZlSound s = o; s.length = J.N;
        J.verdict = swap.add(i, reqs[i].id, s);
        wgs += zl_wp_job_wgs(J);
        for (ZlWpRegion R : regs[(size_t)i]) {
            R.off_base += offs; R.job = J.verdict;
            if (R.nseg > 1) seekList.push_back((int32_t)table.size());
            table.push_back(R);
        }
        offs += sums[(size_t)i].segments;
        jobs.push_back(J);
    }
    const char *what = "sound_warp: no memory for the call's records";
    const size_t nj = jobs.size(), n = std::max<size_t>(nj * 2, 64), nr = table.size(), ns = std::max<size_t>(seekList.size(), 1), no = (size_t)offs;
    const int rsv = reserve(e, false, { { ZB_WP_JOBS, nj, sizeof(ZlWpJob), n, false, what }, { ZB_WP_REGIONS, nr, sizeof(ZlWpRegion), std::max<size_t>(nr * 2, 1024), false, what },
                                       { ZB_WP_LIST, ns, sizeof(int32_t), std::max<size_t>(ns * 2, 1024), false, what }, { ZB_WP_OFFS, no, sizeof(int32_t), std::max<size_t>(no * 2, 4096), false, what },
                                       { ZB_WP_PUB, nj, sizeof(ZlRsPublish), n, false, what }, { ZB_WP_VERDICTS, nj, sizeof(uint32_t), n, false, what } });
    if (rsv != ZLHIP_OK) { ext.rollback(); return rsv; }
    ZlWpJob *const dJobs = (ZlWpJob *)e->scratch[ZB_WP_JOBS].d; ZlWpRegion *const dRegs = (ZlWpRegion *)e->scratch[ZB_WP_REGIONS].d;
    int32_t *const dList = (int32_t *)e->scratch[ZB_WP_LIST].d, *const dOffs = (int32_t *)e->scratch[ZB_WP_OFFS].d;
    ZlRsPublish *const dPub = (ZlRsPublish *)e->scratch[ZB_WP_PUB].d; uint32_t *const dVerdicts = (uint32_t *)e->scratch[ZB_WP_VERDICTS].d;
    // everything is decided: from here on only a HIP error fails the call
    zlhip_engine::Warp &t = e->wp;
    t.timer.on = e->profiling;
    std::vector<int32_t> hOffs(no, 0); std::vector<uint32_t> verdictsOut(nj, 0u);
    int krc = (int)hipMemcpyAsync(dJobs, jobs.data(), nj * sizeof(ZlWpJob), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dRegs, table.data(), nr * sizeof(ZlWpRegion), hipMemcpyHostToDevice, e->stream);
    if (krc == 0 && !seekList.empty()) krc = (int)hipMemcpyAsync(dList, seekList.data(), seekList.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dVerdicts, swap.words.data(), nj * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(dPub, swap.pub.data(), nj * sizeof(ZlRsPublish), hipMemcpyHostToDevice, e->stream);
    if (krc == 0) krc = (int)hipMemsetAsync(dOffs, 0, no * sizeof(int32_t), e->stream);     // (off[0] of every region, the copy regions' included)
    if (krc == 0) krc = (int)t.timer.mark(0, e->stream);
    if (krc == 0) krc = zl_launch_warp_seek(dJobs, dRegs, dList, (int32_t)seekList.size(), dOffs, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(1, e->stream);
    if (krc == 0) krc = zl_launch_warp_synth(dJobs, (int32_t)nj, wgs, dRegs, dOffs, dVerdicts, e->stream);
    if (krc == 0) krc = zl_launch_resample_publish(dPub, (int32_t)nj, dVerdicts, e->dSounds, e->stream);
    if (krc == 0) krc = (int)t.timer.mark(2, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(hOffs.data(), dOffs, no * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipMemcpyAsync(verdictsOut.data(), dVerdicts, nj * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream);
    if (krc == 0) krc = (int)hipStreamSynchronize(e->stream);      // the call's one wait
    if (krc == 0) krc = (int)t.timer.elapsed(0, 1, &t.seekMs);
    if (krc == 0) krc = (int)t.timer.elapsed(1, 2, &t.synthMs);
    if (krc != 0) return swap.hip_failed(krc);
    swap.commit(verdictsOut, [&](size_t j, zlhip_engine::SoundSlot &slot) {     // (and the seek offsets of the slot's last warp)
        const ZlWpRegion &first = table[(size_t)jobs[j].region_base];
        slot.warpOffsets.assign(hOffs.begin() + first.off_base, hOffs.begin() + first.off_base + sums[(size_t)swap.jobReq[j]].segments);
    });
    std::memcpy(out, sums.data(), (size_t)count * sizeof(zlhip_warp));
    return ZLHIP_OK;
}

int zlhip_sound_warp(zlhip_engine *e, const zlhip_warp_request *r, zlhip_warp *out) { return zlhip_sound_warp_batch(e, r, 1, out); }

int zlhip_debug_warp_offsets(zlhip_engine *e, int32_t id, int32_t *out, int32_t capacity, int32_t *count)
{
    if (!e || id < 0 || id >= e->cfg.max_sounds || !e->hc.soundUsed[id]) return ZLHIP_ERR_INVALID;
    const std::vector<int32_t> &o = e->soundSlots[(size_t)id].warpOffsets;
    if (count) *count = (int32_t)o.size();
    if (!out) return ZLHIP_OK;
    if ((size_t)capacity < o.size()) return fail(e, ZLHIP_ERR_CAPACITY, "debug_warp_offsets: capacity below the count");
    if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(int32_t));
    return ZLHIP_OK;
}

int zlhip_debug_warp_timings(zlhip_engine *e, float *seek_ms, float *synth_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (seek_ms) *seek_ms = e->wp.seekMs;
    if (synth_ms) *synth_ms = e->wp.synthMs;
    return ZLHIP_OK;
}

// ---- key (zl_key.h, zl_key.hip) --------------------------------------------------------------------------------------------
// What key a loop is in.  The gate kernel leaves every frame's energy verdict, the correlate kernel re and im per frame and bin, the
// fold the per-bin totals and the integer record in host memory mapped into the device; tonic, mode and the two confidences are
// derived here (zl_ky_finish).  The bin tables are made here, in double, and handed to the kernels: the device computes no
// frequency.  Synchronisation and buffers as for the overviews.
int zlhip_key_resolve(double sample_rate, zlhip_key_request *r)
{
    if (!r || r->first_frame < 0 || r->num_frames < 1) return ZLHIP_ERR_INVALID;
    zlhip_key_request q = *r;
    if (zl_ky_resolve(sample_rate, &q.hop, &q.max_frames, &q.a4_hz, &q.note_lo, &q.note_hi, &q.q, &q.gate) != 0) return ZLHIP_ERR_INVALID;
    *r = q;
    return ZLHIP_OK;
}

int zlhip_key_design(double sample_rate, const zlhip_key_request *r, zlhip_key_bin *bins, int32_t capacity, int32_t *nbins, int16_t *table)
{
    static_assert(sizeof(zlhip_key_bin) == sizeof(ZlKyBin), "zl_ky_design writes zlhip_key_bin's layout");
    if (!r) return ZLHIP_ERR_INVALID;
    zlhip_key_request q = *r;
    if (zlhip_key_resolve(sample_rate, &q) != ZLHIP_OK) return ZLHIP_ERR_INVALID;
    const int32_t n = q.note_hi - q.note_lo + 1;
    if (nbins) *nbins = n;
    if (bins && capacity < n) return ZLHIP_ERR_CAPACITY;
    zl_ky_design(sample_rate, q.a4_hz, q.note_lo, q.note_hi, q.q, (ZlKyBin *)bins, table);
    return ZLHIP_OK;
}

int zlhip_key_match_shift(int32_t clip_tonic, int32_t clip_mode, int32_t tonic, int32_t mode)
{
    if (clip_tonic < 0 || clip_tonic > 11 || tonic < 0 || tonic > 11 || clip_mode < 0 || clip_mode > 1 || mode < 0 || mode > 1) return 0;
    return zl_ky_match_shift(clip_tonic, clip_mode, tonic, mode);
}

int zlhip_sound_key_batch(zlhip_engine *e, const zlhip_key_request *reqs, int32_t nreq, zlhip_key *out)
{
    static_assert(sizeof(zlhip_key) == sizeof(ZlKyResult) && sizeof(ZlKyResult) == 136, "the device writes zlhip_key's layout");
    if (!e || nreq < 0 || (nreq > 0 && (!reqs || !out))) return ZLHIP_ERR_INVALID;
    if (nreq == 0) return ZLHIP_OK;
    // validate and resolve everything before anything is written and before the first HIP call
    std::vector<ZlKyRequest> geo((size_t)nreq);
    std::vector<ZlKyBin> table;
    int64_t frames = 0, pairs = 0, items = 0;
    for (int32_t i = 0; i < nreq; ++i) {
        zlhip_key_request q = reqs[i];
        auto resolve = [&](const ZlSound &s) { return zlhip_key_resolve(s.sample_rate, &q) != ZLHIP_OK ? kOutsideLimits : nullptr; };
        { const int rc = check_request(e, "sound_key", q, resolve); if (rc != ZLHIP_OK) return rc; }
        const ZlSound &s = e->hc.sounds[q.id];
        ZlKyRequest &R = geo[(size_t)i];
        R.nbins = q.note_hi - q.note_lo + 1; R.bin_base = (int32_t)table.size();
        table.resize(table.size() + (size_t)R.nbins);
        zl_ky_design(s.sample_rate, q.a4_hz, q.note_lo, q.note_hi, q.q, table.data() + R.bin_base, nullptr);
        R.src = 0;                                                 // (the address: behind the reserve, with the other HIP-side state)
        R.span = table[(size_t)R.bin_base].n;
        R.floor_ = (uint64_t)R.span * (uint64_t)s.channels * (uint64_t)q.gate * (uint64_t)q.gate;
        R.first = q.first_frame; R.channels = s.channels; R.reserved = 0;
        zl_ky_frames(q.num_frames, R.span, q.hop, q.max_frames, &R.frames, &R.hop);
        R.acc_base = pairs; R.frame_base = (int32_t)frames; R.item_base = (int32_t)items;
        frames += R.frames; pairs += (int64_t)R.frames * R.nbins; items += zl_ky_items(R);
        if (frames > ZL_KY_MAX_CALL_FRAMES) return fail(e, ZLHIP_ERR_INVALID, "sound_key_batch: more than 65536 analysis frames in one call");
    }
    { const int rc = call_begin(e, false); if (rc != ZLHIP_OK) return rc; }
    zlhip_engine::Key &t = e->ky;
    const char *what = "sound_key: no memory for the call's buffers";
    const size_t n = (size_t)nreq, f = (size_t)frames, p = (size_t)pairs, nb = table.size(), fcap = std::min<size_t>(std::max<size_t>(f * 2, 256), ZL_KY_MAX_CALL_FRAMES);
    const int rsv = reserve(e, true, { { ZB_KY_REQ, n, sizeof(ZlKyRequest), std::max<size_t>(n * 2, 64), true, what },
                                      { ZB_KY_BINS, nb, sizeof(ZlKyBin), std::max<size_t>(nb * 2, 4096), true, what },
                                      { ZB_KY_TABLE, ZL_KY_TABLE, sizeof(uint32_t), ZL_KY_TABLE, true, what },
                                      { ZB_KY_STAT, f, sizeof(ZlKyStat), fcap, false, what },
                                      { ZB_KY_ACC, p, sizeof(ZlKyAcc), std::max<size_t>(p + p / 2, 16384), false, what },
                                      { ZB_KY_TOTAL, nb, sizeof(uint64_t), std::max<size_t>(nb * 2, 4096), false, what } },
                           { mapped_need(t.out, std::max<size_t>(n, 32)) });
    if (rsv != ZLHIP_OK) return rsv;
    ZlKyRequest *const hReq = (ZlKyRequest *)e->scratch[ZB_KY_REQ].h, *const dReq = (ZlKyRequest *)e->scratch[ZB_KY_REQ].d;
    ZlKyBin *const hBins = (ZlKyBin *)e->scratch[ZB_KY_BINS].h, *const dBins = (ZlKyBin *)e->scratch[ZB_KY_BINS].d;
    uint32_t *const hP = (uint32_t *)e->scratch[ZB_KY_TABLE].h, *const dP = (uint32_t *)e->scratch[ZB_KY_TABLE].d;
    ZlKyStat *const dStat = (ZlKyStat *)e->scratch[ZB_KY_STAT].d; ZlKyAcc *const dAcc = (ZlKyAcc *)e->scratch[ZB_KY_ACC].d;
    uint64_t *const dTotal = (uint64_t *)e->scratch[ZB_KY_TOTAL].d;
    t.last.clear();
    for (int32_t i = 0; i < nreq; ++i) {
        ZlKyRequest &R = hReq[i];
        R = geo[(size_t)i];
        R.src = (uint64_t)(uintptr_t)arena_ptr(e, e->hc.sounds[reqs[i].id].offset);
        t.last.push_back({R.acc_base, R.bin_base, R.nbins, R.frames});
    }
    std::memcpy(hBins, table.data(), nb * sizeof(ZlKyBin));
    {                                                              // (the cosine table depends on nothing; the kernel takes it paired)
        int16_t T[ZL_KY_TABLE];
        zl_ky_design(1.0, 0.0f, 1, 0, 0, nullptr, T);
        for (int32_t i = 0; i < ZL_KY_TABLE; ++i) hP[i] = zl_ky_pair(T, i);
    }
    t.timer.on = e->profiling;
    ZL_HIP(e, hipMemcpyAsync(dReq, hReq, (size_t)nreq * sizeof(ZlKyRequest), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, hipMemcpyAsync(dBins, hBins, nb * sizeof(ZlKyBin), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, hipMemcpyAsync(dP, hP, ZL_KY_TABLE * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    ZL_HIP(e, t.timer.mark(0, e->stream));
    ZL_KERNEL(e, zl_launch_key_gate(dReq, nreq, frames, dStat, e->stream));
    ZL_HIP(e, t.timer.mark(1, e->stream));
    ZL_KERNEL(e, zl_launch_key_correlate(dReq, nreq, items, dBins, dP, dStat, dAcc, e->stream));
    ZL_HIP(e, t.timer.mark(2, e->stream));
    ZL_KERNEL(e, zl_launch_key_fold(dReq, nreq, dBins, dStat, dAcc, dTotal, t.out.d, e->stream));
    ZL_HIP(e, t.timer.mark(3, e->stream));
    { int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    ZL_HIP(e, t.timer.elapsed(0, 1, &t.gateMs)); ZL_HIP(e, t.timer.elapsed(1, 2, &t.correlateMs)); ZL_HIP(e, t.timer.elapsed(2, 3, &t.foldMs));
    for (int32_t i = 0; i < nreq; ++i) {
        ZlKyResult r = t.out.h[i];
        zl_ky_finish(&r);
        std::memcpy(&out[i], &r, sizeof(r));
    }
    return ZLHIP_OK;
}

int zlhip_sound_key(zlhip_engine *e, const zlhip_key_request *r, zlhip_key *out) { return zlhip_sound_key_batch(e, r, 1, out); }

int zlhip_debug_key_bins(zlhip_engine *e, int32_t request, uint64_t *totals, int32_t capacity, int32_t *bins)
{
    if (!e || request < 0 || (size_t)request >= e->ky.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Key::Last &l = e->ky.last[(size_t)request];
    if (bins) *bins = l.nbins;
    if (!totals) return ZLHIP_OK;
    if (capacity < l.nbins) return fail(e, ZLHIP_ERR_CAPACITY, "debug_key_bins: capacity below the request's bins");
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(totals, (const uint64_t *)e->scratch[ZB_KY_TOTAL].d + l.bin_base, (size_t)l.nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    return engine_wait(e);
}

int zlhip_debug_key_frame(zlhip_engine *e, int32_t request, int32_t frame, int64_t *re, int64_t *im, int32_t capacity, int32_t *bins, int32_t *frames)
{
    if (!e || request < 0 || (size_t)request >= e->ky.last.size()) return ZLHIP_ERR_INVALID;
    const zlhip_engine::Key::Last &l = e->ky.last[(size_t)request];
    if (bins) *bins = l.nbins;
    if (frames) *frames = l.frames;
    if (!re && !im) return ZLHIP_OK;
    if (frame < 0 || frame >= l.frames) return fail(e, ZLHIP_ERR_INVALID, "debug_key_frame: no such frame");
    if (capacity < l.nbins) return fail(e, ZLHIP_ERR_CAPACITY, "debug_key_frame: capacity below the request's bins");
    std::vector<ZlKyAcc> a((size_t)l.nbins);
    ZL_HIP(e, hipSetDevice(e->device));
    ZL_HIP(e, hipMemcpyAsync(a.data(), (const ZlKyAcc *)e->scratch[ZB_KY_ACC].d + l.acc_base + (int64_t)frame * l.nbins, a.size() * sizeof(ZlKyAcc), hipMemcpyDeviceToHost, e->stream));
    { const int w_ = engine_wait(e); if (w_ != ZLHIP_OK) return w_; }
    for (int32_t b = 0; b < l.nbins; ++b) { if (re) re[b] = a[(size_t)b].re; if (im) im[b] = a[(size_t)b].im; }
    return ZLHIP_OK;
}

int zlhip_debug_key_timings(zlhip_engine *e, float *gate_ms, float *correlate_ms, float *fold_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (gate_ms) *gate_ms = e->ky.gateMs;
    if (correlate_ms) *correlate_ms = e->ky.correlateMs;
    if (fold_ms) *fold_ms = e->ky.foldMs;
    return ZLHIP_OK;
}

int zlhip_debug_rerender_timings(zlhip_engine *e, float *seek_ms, float *synth_ms)
{
    if (!e) return ZLHIP_ERR_INVALID;
    if (seek_ms) *seek_ms = e->st.seekMs;
    if (synth_ms) *synth_ms = e->st.synthMs;
    return ZLHIP_OK;
}

int zlhip_debug_rerender_offsets(zlhip_engine *e, int32_t id, int32_t *out, int32_t capacity, int32_t *count)
{
    if (!e || id < 0 || id >= e->cfg.max_sounds || !e->hc.soundUsed[id]) return ZLHIP_ERR_INVALID;
    const std::vector<int32_t> &o = e->soundSlots[(size_t)id].renderOffsets;
    if (count) *count = (int32_t)o.size();
    if (!out) return ZLHIP_OK;
    if ((size_t)capacity < o.size()) return fail(e, ZLHIP_ERR_CAPACITY, "debug_rerender_offsets: capacity below the count");
    if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(int32_t));
    return ZLHIP_OK;
}

}  // extern "C"
