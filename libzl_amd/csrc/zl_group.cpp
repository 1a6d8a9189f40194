// zl_group.cpp -- the engine group of include/zlhip.h (zlhip_group_*): n engines in one process, one per listed device, driven as
// ONE synth.  The partition arithmetic and the command routing are zl_group.h's (HIP-free, tested on the CPU); this file owns the
// members, broadcasts sounds and clips, gathers reads into the global layouts and -- in the span partition -- orders the members'
// renders and the spanning-bus sum (zl_k_group_reduce_scan) with events only:
//   1. after every member's render one event per member; every member's stream waits for all of them before its share of the sum;
//   2. the root's stream waits for every member's sum, so the root engine's own host waits (read_bus, levels) cover the whole sum;
//   3. every member's next render waits for every sum of the call before: those launches read every member's partial bus and wrote
//      into the root's buffers.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/zlhip.h"
#include "zl_group.h"
#include "zl_kernels.h"
#include "zl_member.h"

struct zlhip_group {
    ZlGroupLayout L;
    zlhip_config cfg{};
    std::vector<int> dev;
    std::vector<zlhip_engine *> m;
    std::vector<hipEvent_t> evRendered, evReduced;
    bool reduced = false;                // evReduced marks the sums of the last call (step 3 waits for them)
    int lastK = 0, lastN = 0;
    std::string err;
};

namespace {
thread_local std::string g_createErr;     // why the last zlhip_group_create of this thread failed (zlhip_group_last_error(NULL))

int create_fail(int code, const std::string &msg)
{
    g_createErr = msg;
    return code;
}

int gfail(zlhip_group *g, int code, const std::string &msg)
{
    g->err = msg;
    return code;
}

// a member call failed: its own message, prefixed with the member
int member_fail(zlhip_group *g, int r, int code)
{
    g->err = "member " + std::to_string(r) + ": " + zlhip_last_error(g->m[(size_t)r]);
    return code;
}

#define ZL_GHIP(g, call)                                                                       \
    do {                                                                                       \
        hipError_t st_ = (call);                                                               \
        if (st_ != hipSuccess) return gfail((g), ZLHIP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(st_)); \
    } while (0)

// every member's control plane, voices that ended on the device released
int controls(zlhip_group *g, std::vector<ZlHostControl *> &ctl)
{
    ctl.resize((size_t)g->L.n);
    for (int r = 0; r < g->L.n; ++r) {
        int rc = ZLHIP_OK;
        ctl[(size_t)r] = zl_member_control(g->m[(size_t)r], &rc);
        if (!ctl[(size_t)r]) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

bool valid_voice(const zlhip_group *g, int bus, int slot)
{
    return bus >= 0 && bus < g->L.B && slot >= 0 && slot < g->L.VPB;
}

void destroy_members(zlhip_group *g)
{
    // a member's sum reads every other member's partial bus: nothing is freed before every member is idle
    for (zlhip_engine *e : g->m) if (e) (void)zlhip_synchronize(e);
    for (size_t r = 0; r < g->m.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        if (r < g->evRendered.size() && g->evRendered[r]) (void)hipEventDestroy(g->evRendered[r]);
        if (r < g->evReduced.size() && g->evReduced[r]) (void)hipEventDestroy(g->evReduced[r]);
    }
    for (zlhip_engine *e : g->m) if (e) zlhip_engine_destroy(e);
    g->m.clear();
}
}  // namespace

extern "C" {

void zlhip_group_config_default(zlhip_group_config *gc)
{
    if (!gc) return;
    gc->struct_size = sizeof(zlhip_group_config);
    gc->partition = ZLHIP_GROUP_AUTO;
    gc->root = 0;
    gc->reserved = 0;
}

const char *zlhip_group_last_error(const zlhip_group *g) { return g ? g->err.c_str() : g_createErr.c_str(); }

int zlhip_group_create(const int32_t *devices, int32_t n, const zlhip_config *cfg_in, const zlhip_group_config *gc_in, zlhip_group **out)
{
    if (!out) return create_fail(ZLHIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || !cfg_in) return create_fail(ZLHIP_ERR_INVALID, "devices and cfg are required");
    // every check before the first HIP call
    zlhip_config cfg;
    zlhip_config_default(&cfg);
    const size_t known = cfg_in->struct_size && cfg_in->struct_size < sizeof(zlhip_config) ? cfg_in->struct_size : sizeof(zlhip_config);
    std::memcpy(&cfg, cfg_in, known);
    zlhip_group_config gc;
    zlhip_group_config_default(&gc);
    if (gc_in) gc = *gc_in;
    ZlGroupLayout L;
    const char *why = "";
    if (zl_group_plan(n, cfg, gc, L, &why) != ZLHIP_OK) return create_fail(ZLHIP_ERR_INVALID, why);
    for (int r = 0; r < n; ++r) if (devices[r] < 0) return create_fail(ZLHIP_ERR_INVALID, "negative device ordinal");

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        return create_fail(ZLHIP_ERR_NO_DEVICE, "no usable HIP device (the library has no CPU render path)");
    }
    for (int r = 0; r < n; ++r)
        if (devices[r] >= count) return create_fail(ZLHIP_ERR_INVALID, "device " + std::to_string(devices[r]) + " does not exist");
    // peer access for every ordered pair of distinct devices; "already enabled" (torch, another group) is fine
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            const int a = devices[i], b = devices[j];
            if (a == b) continue;
            bool seen = false;                                     // (a pair listed twice is enabled once)
            for (int i2 = 0; i2 < i && !seen; ++i2) for (int j2 = 0; j2 < n && !seen; ++j2) seen = devices[i2] == a && devices[j2] == b;
            if (seen) continue;
            int can = 0;
            if (hipSetDevice(a) != hipSuccess || hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can)
                return create_fail(ZLHIP_ERR_HIP, "devices " + std::to_string(a) + " and " + std::to_string(b) +
                                   ": device " + std::to_string(a) + " cannot access the memory of device " + std::to_string(b) + " (peer access)");
            const hipError_t st = hipDeviceEnablePeerAccess(b, 0);
            if (st == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else if (st != hipSuccess)
                return create_fail(ZLHIP_ERR_HIP, "hipDeviceEnablePeerAccess(" + std::to_string(a) + " -> " + std::to_string(b) + "): " + hipGetErrorString(st));
        }
    }

    zlhip_group *g = new zlhip_group;
    g->L = L; g->cfg = cfg;
    g->dev.assign(devices, devices + n);
    g->m.assign((size_t)n, nullptr);
    g->evRendered.assign((size_t)n, nullptr);
    g->evReduced.assign((size_t)n, nullptr);
    for (int r = 0; r < n; ++r) {
        zlhip_config mc = zl_group_member_config(L, cfg, r);
        mc.device = devices[r];
        const int rc = zlhip_engine_create(&mc, &g->m[(size_t)r]);
        if (rc != ZLHIP_OK) {
            g->m[(size_t)r] = nullptr;
            destroy_members(g);
            delete g;
            return create_fail(rc, "member " + std::to_string(r) + " (device " + std::to_string(devices[r]) + "): zlhip_engine_create: " + zlhip_strerror(rc));
        }
        hipError_t st = hipSetDevice(devices[r]);
        if (st == hipSuccess) st = hipEventCreateWithFlags(&g->evRendered[(size_t)r], hipEventDisableTiming);
        if (st == hipSuccess) st = hipEventCreateWithFlags(&g->evReduced[(size_t)r], hipEventDisableTiming);
        if (st != hipSuccess) {
            destroy_members(g);
            delete g;
            return create_fail(ZLHIP_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(st));
        }
    }
    *out = g;
    return ZLHIP_OK;
}

void zlhip_group_destroy(zlhip_group *g)
{
    if (!g) return;
    destroy_members(g);
    delete g;
}

int zlhip_group_layout(zlhip_group *g, int32_t *partition, int32_t *first_bus, int32_t *num_buses, int32_t *first_slot, int32_t *slots)
{
    if (!g) return ZLHIP_ERR_INVALID;
    for (int r = 0; r < g->L.n; ++r) {
        if (partition) partition[r] = g->L.partition;
        if (first_bus) first_bus[r] = g->L.first_bus[r];
        if (num_buses) num_buses[r] = g->L.num_buses[r];
        if (first_slot) first_slot[r] = g->L.first_slot[r];
        if (slots) slots[r] = g->L.slots[r];
    }
    return ZLHIP_OK;
}

zlhip_engine *zlhip_group_member(zlhip_group *g, int32_t r)
{
    return g && r >= 0 && r < g->L.n ? g->m[(size_t)r] : nullptr;
}

// ---- sounds and clips: broadcast, in the same order on every member --------------------------------------------------------
int zlhip_group_sound_upload(zlhip_group *g, const float *left, const float *right, int32_t length, double sample_rate, int32_t *out_id)
{
    if (!g || !out_id) return ZLHIP_ERR_INVALID;
    int32_t id0 = -1;
    for (int r = 0; r < g->L.n; ++r) {
        int32_t id = -1;
        int rc = zlhip_sound_upload(g->m[(size_t)r], left, right, length, sample_rate, &id);
        if (rc == ZLHIP_OK && r > 0 && id != id0) {
            (void)zlhip_sound_release(g->m[(size_t)r], id);
            rc = gfail(g, ZLHIP_ERR_STATE, "member " + std::to_string(r) + " gave the sound id " + std::to_string(id) + ", member 0 gave " +
                       std::to_string(id0) + ": the members' sound tables disagree");
        } else if (rc != ZLHIP_OK) {
            rc = member_fail(g, r, rc);
        }
        if (rc != ZLHIP_OK) {
            for (int q = 0; q < r; ++q) (void)zlhip_sound_release(g->m[(size_t)q], id0);
            return rc;
        }
        if (r == 0) id0 = id;
    }
    *out_id = id0;
    return ZLHIP_OK;
}

int zlhip_group_sound_upload_pcm_batch(zlhip_group *g, const zlhip_pcm_source *srcs, int32_t count, int32_t *out_ids)
{
    if (!g || count < 0 || (count > 0 && (!srcs || !out_ids))) return ZLHIP_ERR_INVALID;
    if (count == 0) return ZLHIP_OK;
    std::vector<int32_t> ids0((size_t)count, -1), ids((size_t)count, -1);
    for (int r = 0; r < g->L.n; ++r) {
        int rc = zlhip_sound_upload_pcm_batch(g->m[(size_t)r], srcs, count, r == 0 ? ids0.data() : ids.data());
        if (rc == ZLHIP_OK && r > 0 && ids != ids0) {
            for (int32_t id : ids) (void)zlhip_sound_release(g->m[(size_t)r], id);
            rc = gfail(g, ZLHIP_ERR_STATE, "member " + std::to_string(r) + " gave other sound ids than member 0: the members' sound tables disagree");
        } else if (rc != ZLHIP_OK) {
            rc = member_fail(g, r, rc);                            // (a member's call is all or nothing: it kept nothing)
        }
        if (rc != ZLHIP_OK) {
            for (int q = 0; q < r; ++q) for (int32_t id : ids0) (void)zlhip_sound_release(g->m[(size_t)q], id);
            for (int32_t i = 0; i < count; ++i) out_ids[i] = -1;
            return rc;
        }
    }
    for (int32_t i = 0; i < count; ++i) out_ids[i] = ids0[(size_t)i];
    return ZLHIP_OK;
}

int zlhip_group_sound_release(zlhip_group *g, int32_t id)
{
    if (!g) return ZLHIP_ERR_INVALID;
    int first = ZLHIP_OK;
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_release(g->m[(size_t)r], id);
        if (rc != ZLHIP_OK && first == ZLHIP_OK) first = member_fail(g, r, rc);
    }
    return first;
}

int zlhip_group_clip_set(zlhip_group *g, int32_t id, const zlhip_clip_params *p)
{
    if (!g) return ZLHIP_ERR_INVALID;
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_clip_set(g->m[(size_t)r], id, p);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_rerender_batch(zlhip_group *g, const int32_t *ids, const zlhip_rerender_params *params, int32_t count)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (the members' arenas are alike: a call that does not fit fails on member 0 and leaves every member as it was)
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_rerender_batch(g->m[(size_t)r], ids, params, count);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_convert_rate_batch(zlhip_group *g, const int32_t *ids, int32_t count, double target_rate)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (the members hold the same clips in arenas that are alike: a call that is invalid or does not fit fails on member 0 and leaves every member as it was)
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_convert_rate_batch(g->m[(size_t)r], ids, count, target_rate);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

// sounds are broadcast: every member holds the same playback data, member 0 answers
int zlhip_group_sound_overview_batch(zlhip_group *g, const zlhip_overview_request *reqs, int32_t count, float *out, size_t out_floats)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_overview_batch(g->m[0], reqs, count, out, out_floats);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_overview(zlhip_group *g, int32_t id, int32_t first_frame, int32_t num_frames, int32_t columns, float *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_overview(g->m[0], id, first_frame, num_frames, columns, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_onsets_batch(zlhip_group *g, const zlhip_onset_request *reqs, int32_t nreq, zlhip_onset *out, size_t capacity, int32_t *counts)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_onsets_batch(g->m[0], reqs, nreq, out, capacity, counts);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_tempo_batch(zlhip_group *g, const zlhip_tempo_request *reqs, int32_t nreq, zlhip_tempo *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_tempo_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_pitch_batch(zlhip_group *g, const zlhip_pitch_request *reqs, int32_t nreq, zlhip_pitch *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_pitch_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_loudness_batch(zlhip_group *g, const zlhip_loudness_request *reqs, int32_t nreq, zlhip_loudness *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_loudness_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_loop_batch(zlhip_group *g, const zlhip_loop_request *reqs, int32_t nreq, zlhip_loop *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_loop_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_loop_crossfade_batch(zlhip_group *g, const zlhip_xfade_request *reqs, int32_t count, zlhip_xfade *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (the members hold the same clips in arenas that are alike: a call that is invalid or does not fit fails on member 0 and leaves every
    // member as it was; every member measures the same integers, member 0's results are the call's)
    std::vector<zlhip_xfade> rest((size_t)(count > 0 ? count : 0));
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_loop_crossfade_batch(g->m[(size_t)r], reqs, count, r == 0 ? out : rest.data());
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_edit_batch(zlhip_group *g, const zlhip_edit_request *reqs, int32_t count, zlhip_edit *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (as zlhip_group_sound_loop_crossfade_batch: a call that is invalid or does not fit fails on member 0 and leaves every member as it was)
    std::vector<zlhip_edit> rest((size_t)(count > 0 ? count : 0));
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_edit_batch(g->m[(size_t)r], reqs, count, r == 0 ? out : rest.data());
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_peak_batch(zlhip_group *g, const zlhip_peak_request *reqs, int32_t nreq, zlhip_peak *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_peak_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

int zlhip_group_sound_limit_batch(zlhip_group *g, const zlhip_limit_request *reqs, int32_t count, zlhip_limit *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (as zlhip_group_sound_loop_crossfade_batch: a call that is invalid or does not fit fails on member 0 and leaves every member as it was)
    std::vector<zlhip_limit> rest((size_t)(count > 0 ? count : 0));
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_limit_batch(g->m[(size_t)r], reqs, count, r == 0 ? out : rest.data());
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_warp_batch(zlhip_group *g, const zlhip_warp_request *reqs, int32_t count, zlhip_warp *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    // (as zlhip_group_sound_loop_crossfade_batch: a call that is invalid or does not fit fails on member 0 and leaves every member as it was)
    std::vector<zlhip_warp> rest((size_t)(count > 0 ? count : 0));
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_sound_warp_batch(g->m[(size_t)r], reqs, count, r == 0 ? out : rest.data());
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_sound_key_batch(zlhip_group *g, const zlhip_key_request *reqs, int32_t nreq, zlhip_key *out)
{
    if (!g) return ZLHIP_ERR_INVALID;
    const int rc = zlhip_sound_key_batch(g->m[0], reqs, nreq, out);
    return rc != ZLHIP_OK ? member_fail(g, 0, rc) : ZLHIP_OK;
}

// ---- commands (global buses, slots, voices and midi channels) ------------------------------------------------------------
int zlhip_group_handle_commands(zlhip_group *g, const zlhip_clip_command *cmds, int32_t count, uint64_t current_tick, int32_t *taken,
                                int32_t *voices)
{
    if (!g || (!cmds && count > 0) || count < 0) return ZLHIP_ERR_INVALID;
    std::vector<ZlHostControl *> ctl;
    int rc = controls(g, ctl);
    if (rc != ZLHIP_OK) return rc;
    int sum = 0;
    for (int32_t i = 0; i < count; ++i) {
        int v = -1;
        const int t = zl_group_route_command(g->L, ctl.data(), cmds[i], current_tick, &v);
        if (taken) taken[i] = t;
        if (voices) voices[i] = v;
        sum += t;
    }
    return sum;
}

int zlhip_group_start_voice(zlhip_group *g, int32_t bus, int32_t slot, const zlhip_clip_command *cmd, uint64_t current_tick)
{
    if (!g || !cmd || !valid_voice(g, bus, slot)) return ZLHIP_ERR_INVALID;
    std::vector<ZlHostControl *> ctl;
    int rc = controls(g, ctl);
    if (rc != ZLHIP_OK) return rc;
    return zl_group_route_start_voice(g->L, ctl.data(), bus, slot, *cmd, current_tick);
}

int zlhip_group_stop_voice(zlhip_group *g, int32_t bus, int32_t slot, int allow_tail_off)
{
    if (!g || !valid_voice(g, bus, slot)) return ZLHIP_ERR_INVALID;
    int lb, ls;
    const int r = zl_group_locate(g->L, bus, slot, &lb, &ls);
    const int rc = zlhip_stop_voice(g->m[(size_t)r], lb, ls, allow_tail_off);
    return rc < 0 ? member_fail(g, r, rc) : rc;
}

int zlhip_group_update_voice(zlhip_group *g, int32_t bus, int32_t slot, const zlhip_clip_command *cmd)
{
    if (!g || !cmd || !valid_voice(g, bus, slot)) return ZLHIP_ERR_INVALID;
    int lb, ls;
    const int r = zl_group_locate(g->L, bus, slot, &lb, &ls);
    const int rc = zlhip_update_voice(g->m[(size_t)r], lb, ls, cmd);
    return rc < 0 ? member_fail(g, r, rc) : rc;
}

int zlhip_group_voice_is_playing(zlhip_group *g, int32_t bus, int32_t slot)
{
    if (!g || !valid_voice(g, bus, slot)) return ZLHIP_ERR_INVALID;
    int lb, ls;
    const int r = zl_group_locate(g->L, bus, slot, &lb, &ls);
    const int rc = zlhip_voice_is_playing(g->m[(size_t)r], lb, ls);
    return rc < 0 ? member_fail(g, r, rc) : rc;
}

int zlhip_group_bus_set_enabled(zlhip_group *g, int32_t bus, int enabled)
{
    if (!g || bus < 0 || bus >= g->L.B) return ZLHIP_ERR_INVALID;
    for (int r = 0; r < g->L.n; ++r) {
        int lb = bus;
        if (g->L.partition == ZLHIP_GROUP_BUS_ALIGNED && zl_group_owner(g->L, bus, &lb) != r) continue;
        const int rc = zlhip_bus_set_enabled(g->m[(size_t)r], lb, enabled);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

// ---- render -------------------------------------------------------------------------------------------------------------
int zlhip_group_render_batch(zlhip_group *g, int32_t nblocks, int32_t nframes, const zlhip_clock *clocks, float *bus_out_dev)
{
    if (!g || !clocks) return ZLHIP_ERR_INVALID;
    const ZlGroupLayout &L = g->L;
    const int n = L.n;
    if (L.partition == ZLHIP_GROUP_BUS_ALIGNED) {
        if (bus_out_dev) return gfail(g, ZLHIP_ERR_INVALID, "bus_out_dev is for the span partition only (bus-aligned buses live on several devices)");
        for (int r = 0; r < n; ++r) {
            const int rc = zlhip_render_batch(g->m[(size_t)r], nblocks, nframes, clocks, nullptr, nullptr);
            if (rc != ZLHIP_OK) return member_fail(g, r, rc);
        }
        g->lastK = nblocks; g->lastN = nframes;
        return ZLHIP_OK;
    }
    // span.  Step 3: the previous call's sums read every member's partial bus and wrote the root's bus and levels -- every member's
    // render waits for all of them (its own is in order on its stream)
    if (g->reduced) {
        for (int r = 0; r < n; ++r) {
            ZL_GHIP(g, hipSetDevice(g->dev[(size_t)r]));
            for (int j = 0; j < n; ++j)
                if (j != r) ZL_GHIP(g, hipStreamWaitEvent(zl_member_stream(g->m[(size_t)r]), g->evReduced[(size_t)j], 0));
        }
    }
    for (int r = 0; r < n; ++r) {
        const int rc = zlhip_render_batch(g->m[(size_t)r], nblocks, nframes, clocks, r == L.root ? bus_out_dev : nullptr, nullptr);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
        ZL_GHIP(g, hipSetDevice(g->dev[(size_t)r]));
        ZL_GHIP(g, hipEventRecord(g->evRendered[(size_t)r], zl_member_stream(g->m[(size_t)r])));          // step 1
    }
    ZlGroupReduceArgs a;
    std::memset(&a, 0, sizeof a);
    for (int j = 0; j < n; ++j) a.part[j] = zl_member_last_bus(g->m[(size_t)j]);
    a.out = a.part[L.root] ? const_cast<float *>(a.part[L.root]) : nullptr;
    a.levels = zl_member_levels(g->m[(size_t)L.root]);
    a.B = L.B; a.K = nblocks; a.N = nframes;
    a.off = (g->cfg.mode & ZLHIP_MODE_FIX_DELAY) ? 0 : 1;          // the front frame of the RMS order (zl_scan_rows)
    for (int j = 0; j < n; ++j) if (!a.part[j]) return gfail(g, ZLHIP_ERR_STATE, "a member has no bus buffer");
    const long long P = (long long)nblocks * L.B;
    for (int r = 0; r < n; ++r) {
        hipStream_t s = zl_member_stream(g->m[(size_t)r]);
        ZL_GHIP(g, hipSetDevice(g->dev[(size_t)r]));
        for (int j = 0; j < n; ++j) if (j != r) ZL_GHIP(g, hipStreamWaitEvent(s, g->evRendered[(size_t)j], 0));
        a.p0 = P * r / n; a.p1 = P * (r + 1) / n;                  // member r's share of the (block, bus) pairs
        const int kr = zl_launch_group_reduce(a, n, s);
        if (kr != 0) return gfail(g, ZLHIP_ERR_HIP, std::string("zl_launch_group_reduce: ") + hipGetErrorString((hipError_t)kr));
        ZL_GHIP(g, hipEventRecord(g->evReduced[(size_t)r], s));
    }
    // step 2: the root's stream (and with it the root engine's own host waits) covers every member's share of the sum
    ZL_GHIP(g, hipSetDevice(g->dev[(size_t)L.root]));
    for (int j = 0; j < n; ++j)
        if (j != L.root) ZL_GHIP(g, hipStreamWaitEvent(zl_member_stream(g->m[(size_t)L.root]), g->evReduced[(size_t)j], 0));
    g->reduced = true;
    g->lastK = nblocks; g->lastN = nframes;
    return ZLHIP_OK;
}

int zlhip_group_synchronize(zlhip_group *g)
{
    if (!g) return ZLHIP_ERR_INVALID;
    for (int r = 0; r < g->L.n; ++r) {
        const int rc = zlhip_synchronize(g->m[(size_t)r]);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

// ---- reads, gathered into the global layouts -----------------------------------------------------------------------------
int zlhip_group_read_bus(zlhip_group *g, float *out, size_t out_floats)
{
    if (!g || !out) return ZLHIP_ERR_INVALID;
    const ZlGroupLayout &L = g->L;
    if (L.partition == ZLHIP_GROUP_SPAN) {
        const int rc = zlhip_read_bus(g->m[(size_t)L.root], out, out_floats);
        return rc != ZLHIP_OK ? member_fail(g, L.root, rc) : rc;
    }
    if (g->lastK <= 0) return gfail(g, ZLHIP_ERR_STATE, "nothing to read back: no batch rendered yet");
    const size_t row = 2 * (size_t)g->lastK * (size_t)g->lastN;   // one bus, both channels
    if (out_floats < (size_t)L.B * row) return gfail(g, ZLHIP_ERR_INVALID, "output buffer too small");
    for (int r = 0; r < L.n; ++r) {
        const int rc = zlhip_read_bus(g->m[(size_t)r], out + (size_t)L.first_bus[r] * row, (size_t)L.num_buses[r] * row);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_voice_reports(zlhip_group *g, zlhip_voice_report *out, int32_t count)
{
    if (!g || !out || count < g->L.B * g->L.VPB) return ZLHIP_ERR_INVALID;
    const ZlGroupLayout &L = g->L;
    std::vector<zlhip_voice_report> tmp;
    for (int r = 0; r < L.n; ++r) {
        const int V = L.num_buses[r] * L.vl;
        tmp.resize((size_t)V);
        const int rc = zlhip_voice_reports(g->m[(size_t)r], tmp.data(), V);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
        for (int v = 0; v < V; ++v) out[zl_group_global_voice(L, r, v)] = tmp[(size_t)v];
    }
    return ZLHIP_OK;
}

int zlhip_group_levels_tick(zlhip_group *g, int32_t block_index, int32_t with_hold_bus, zlhip_levels *out)
{
    if (!g || !out) return ZLHIP_ERR_INVALID;
    const ZlGroupLayout &L = g->L;
    if (L.partition == ZLHIP_GROUP_SPAN) {                         // the root meters the summed bus
        const int rc = zlhip_levels_tick(g->m[(size_t)L.root], block_index, with_hold_bus, out);
        return rc != ZLHIP_OK ? member_fail(g, L.root, rc) : rc;
    }
    for (int r = 0; r < L.n; ++r) {
        int lb = -1;
        const int hold = with_hold_bus >= 0 && with_hold_bus < L.B && zl_group_owner(L, with_hold_bus, &lb) == r ? lb : -1;
        const int rc = zlhip_levels_tick(g->m[(size_t)r], block_index, hold, out + L.first_bus[r]);
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
    }
    return ZLHIP_OK;
}

int zlhip_group_block_peaks(zlhip_group *g, int32_t *out, size_t out_ints)
{
    if (!g || !out) return ZLHIP_ERR_INVALID;
    const ZlGroupLayout &L = g->L;
    if (L.partition == ZLHIP_GROUP_SPAN) {
        const int rc = zlhip_block_peaks(g->m[(size_t)L.root], out, out_ints);
        return rc != ZLHIP_OK ? member_fail(g, L.root, rc) : rc;
    }
    const int K = g->lastK;
    if (K <= 0) return gfail(g, ZLHIP_ERR_STATE, "no batch rendered yet");
    if (out_ints < (size_t)K * L.B * 2) return gfail(g, ZLHIP_ERR_INVALID, "output buffer too small");
    std::vector<int32_t> tmp;
    for (int r = 0; r < L.n; ++r) {
        const int nb = L.num_buses[r];
        tmp.resize((size_t)K * nb * 2);
        const int rc = zlhip_block_peaks(g->m[(size_t)r], tmp.data(), tmp.size());
        if (rc != ZLHIP_OK) return member_fail(g, r, rc);
        for (int k = 0; k < K; ++k)
            for (int b = 0; b < nb; ++b)
                for (int c = 0; c < 2; ++c) out[((size_t)k * L.B + L.first_bus[r] + b) * 2 + c] = tmp[((size_t)k * nb + b) * 2 + c];
    }
    return ZLHIP_OK;
}

}  // extern "C"
