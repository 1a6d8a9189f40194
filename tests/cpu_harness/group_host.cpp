// Host build of the engine group's partition arithmetic and command routing (libzl_amd/csrc/zl_group.h) for the CPU tier -- TEST
// HARNESS ONLY.  zlgrp_route_compare drives n member control planes (ZlHostControl, zl_host.h) through the group's routing and one
// control plane with the whole config through the engine's own calls, step by step, and compares what they queue for the device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "zl_group.h"
#include "zl_host.h"

namespace {

void setup(ZlHostControl &hc, int B, int VPB, int nsounds)
{
    hc.init(B, VPB, nsounds, 48000.0);
    for (int i = 0; i < nsounds; ++i) {
        hc.soundUsed[(size_t)i] = 1;
        hc.sounds[(size_t)i] = ZlSound{0, 4000 + 100 * i, 2, i % 2 ? 44100.0 : 48000.0};
        ZlHostControl::default_clip_params(&hc.clipParams[(size_t)i], 0.5f + 0.1f * (float)i);
    }
}

// the device ended voice v (stopNote(.., false) inside process): the report the next refresh absorbs
void end_voice(ZlHostControl &hc, int v)
{
    std::vector<ZlReport> rep(hc.voices.size());
    std::memset(rep.data(), 0, rep.size() * sizeof(ZlReport));
    for (size_t i = 0; i < rep.size(); ++i) rep[i].playing = hc.voices[i].isPlaying && (int)i != v ? 1 : 0;
    hc.absorb_reports(rep.data());
}

std::vector<ZlVoiceOp> drain(ZlHostControl &hc)
{
    std::vector<ZlVoiceOp> ops;
    std::vector<ZlOpRange> ranges;
    hc.drain_ops(ops, ranges);
    return ops;
}

}  // namespace

extern "C" {

// zl_group_plan: returns its status; out [5][8] = partition, first_bus, num_buses, first_slot, slots per member
int zlgrp_plan(int n, int B, int VPB, int vpt, int partition, int root, int32_t *out)
{
    zlhip_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.num_buses = B; cfg.voices_per_bus = VPB; cfg.voices_per_task = vpt;
    zlhip_group_config gc{ (uint32_t)sizeof(zlhip_group_config), partition, root, 0 };
    ZlGroupLayout L;
    const int rc = zl_group_plan(n, cfg, gc, L, nullptr);
    if (rc != ZLHIP_OK) return rc;
    for (int r = 0; r < ZLHIP_GROUP_MAX_MEMBERS; ++r) {
        out[r] = r < n ? L.partition : 0;
        out[8 + r] = L.first_bus[r]; out[16 + r] = L.num_buses[r]; out[24 + r] = L.first_slot[r]; out[32 + r] = L.slots[r];
    }
    return rc;
}

// Step i: kind[i] 0 = a ClipCommand by midi channel (zlhip_handle_commands_voices), 1 = zlhip_start_voice(arg0 = bus, arg1 = slot),
// 2 = the device ends global voice arg0, 3 = zlhip_stop_voice(bus, slot, arg2 = allow tail-off), 4 = zlhip_update_voice(bus, slot).
// out / voice [count]: the return value and the started voice of every step on the single control plane (ref_*) and through the group
// (grp_*).  *ops: voice operations queued in all.  Returns the number of steps whose queued operations (mapped to global voices, in
// voice order, arrival order per voice) differ.
int zlgrp_route_compare(int n, int partition, int B, int VPB, int nsounds, int count, const int32_t *kind, const int32_t *args,
                        const zlhip_clip_command *cmds, int32_t *ref_out, int32_t *ref_voice, int32_t *grp_out, int32_t *grp_voice, int64_t *ops)
{
    zlhip_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.num_buses = B; cfg.voices_per_bus = VPB;
    zlhip_group_config gc{ (uint32_t)sizeof(zlhip_group_config), partition, 0, 0 };
    ZlGroupLayout L;
    if (zl_group_plan(n, cfg, gc, L, nullptr) != ZLHIP_OK) return -1;
    ZlHostControl ref;
    setup(ref, B, VPB, nsounds);
    std::vector<ZlHostControl> mem((size_t)n);
    std::vector<ZlHostControl *> m((size_t)n);
    for (int r = 0; r < n; ++r) { setup(mem[(size_t)r], L.num_buses[r], L.vl, nsounds); m[(size_t)r] = &mem[(size_t)r]; }
    int mismatches = 0;
    *ops = 0;
    for (int i = 0; i < count; ++i) {
        const int a0 = args[3 * i], a1 = args[3 * i + 1], a2 = args[3 * i + 2];
        int ro = 0, rv = -1, go = 0, gv = -1;
        if (kind[i] == 0) {
            ref.lastStartedVoice = -1;
            ro = ref.handle_command(cmds[i], 7);
            rv = ref.lastStartedVoice;
            go = zl_group_route_command(L, m.data(), cmds[i], 7, &gv);
        } else if (kind[i] == 1) {
            ro = ref.handle_on_bus(a0, cmds[i], 7, a1);
            go = zl_group_route_start_voice(L, m.data(), a0, a1, cmds[i], 7);
        } else if (kind[i] == 2) {
            end_voice(ref, a0);
            int lb, ls;
            const int bus = a0 / VPB, slot = a0 % VPB;
            const int r = zl_group_locate(L, bus, slot, &lb, &ls);
            end_voice(mem[(size_t)r], lb * L.vl + ls);
        } else {
            int lb, ls;
            const int r = zl_group_locate(L, a0, a1, &lb, &ls);
            if (kind[i] == 3) { ro = ref.stop_voice(a0, a1, a2 != 0); go = mem[(size_t)r].stop_voice(lb, ls, a2 != 0); }
            else              { ro = ref.update_voice(a0, a1, cmds[i]); go = mem[(size_t)r].update_voice(lb, ls, cmds[i]); }
        }
        ref_out[i] = ro; ref_voice[i] = rv; grp_out[i] = go; grp_voice[i] = gv;
        std::vector<ZlVoiceOp> want = drain(ref), got;
        for (int r = 0; r < n; ++r) {
            for (ZlVoiceOp op : drain(mem[(size_t)r])) { op.voice = zl_group_global_voice(L, r, op.voice); got.push_back(op); }
        }
        std::stable_sort(got.begin(), got.end(), [](const ZlVoiceOp &x, const ZlVoiceOp &y) { return x.voice < y.voice; });
        *ops += (int64_t)want.size();
        bool same = want.size() == got.size();
        for (size_t j = 0; same && j < want.size(); ++j) same = std::memcmp(&want[j], &got[j], sizeof(ZlVoiceOp)) == 0;
        if (!same) ++mismatches;
    }
    return mismatches;
}

}  // extern "C"
