// zl_group.h -- partition arithmetic and command routing of an engine group (zlhip_group_*, include/zlhip.h), HIP-free.
//
// A group drives n engines as ONE synth.  Bus-aligned: member r owns whole buses (the contiguous split of sharding.bus_owner).
// Span: every member has every bus with VPB / n voices, member r the global slots [r * VPB / n, (r + 1) * VPB / n) of each bus
// (sharding.slots_for_rank).  The routing reproduces SamplerChannel::handleCommand (SamplerSynth.cpp:187-230) over a spanning
// bus's voices in global slot order on top of the members' own control planes (ZlHostControl, zl_host.h), one command at a time.
// Used by zl_group.cpp (product) and by tests/cpu_harness/group_host.cpp (CPU unit tests of the same logic).
#pragma once
#include <cstdint>

#include "../../include/zlhip.h"

struct ZlGroupLayout {
    int n = 0, partition = 0, root = 0;
    int B = 0, VPB = 0;
    int vl = 0;                                                   // voices per bus of a member
    int first_bus[ZLHIP_GROUP_MAX_MEMBERS] = {}, num_buses[ZLHIP_GROUP_MAX_MEMBERS] = {};
    int first_slot[ZLHIP_GROUP_MAX_MEMBERS] = {}, slots[ZLHIP_GROUP_MAX_MEMBERS] = {};
};

inline int zl_group_bus_owner(int bus, int B, int n) { return (int)(((long long)bus * n) / B); }   // sharding.bus_owner

// The argument checks of zlhip_group_create (no HIP): ZLHIP_OK and the layout, or ZLHIP_ERR_INVALID and why.
inline int zl_group_plan(int n, const zlhip_config &cfg, const zlhip_group_config &gc, ZlGroupLayout &L, const char **why)
{
    auto bad = [&](const char *m) { if (why) *why = m; return ZLHIP_ERR_INVALID; };
    if (n < 1 || n > ZLHIP_GROUP_MAX_MEMBERS) return bad("a group has 1 .. ZLHIP_GROUP_MAX_MEMBERS members");
    if (gc.struct_size < sizeof(zlhip_group_config) || gc.reserved != 0) return bad("zlhip_group_config: struct_size / reserved");
    const int B = cfg.num_buses, VPB = cfg.voices_per_bus;
    if (B < 1 || VPB < 1) return bad("num_buses and voices_per_bus must be positive");
    int part = gc.partition;
    if (part == ZLHIP_GROUP_AUTO) part = B >= n ? ZLHIP_GROUP_BUS_ALIGNED : ZLHIP_GROUP_SPAN;
    if (part != ZLHIP_GROUP_BUS_ALIGNED && part != ZLHIP_GROUP_SPAN) return bad("unknown partition");
    if (gc.root < 0 || gc.root >= n) return bad("root must name a member");
    if (part == ZLHIP_GROUP_BUS_ALIGNED && B < n) return bad("bus-aligned needs num_buses >= members");
    if (part == ZLHIP_GROUP_SPAN) {
        if (VPB % n != 0) return bad("span needs voices_per_bus to be a multiple of the members");
        if (cfg.voices_per_task != 0 && cfg.voices_per_task != VPB / n) return bad("span needs voices_per_task 0 or voices_per_bus / members");
    }
    L = ZlGroupLayout();
    L.n = n; L.partition = part; L.root = part == ZLHIP_GROUP_SPAN ? gc.root : 0; L.B = B; L.VPB = VPB;
    L.vl = part == ZLHIP_GROUP_SPAN ? VPB / n : VPB;
    for (int r = 0; r < n; ++r) {
        if (part == ZLHIP_GROUP_BUS_ALIGNED) {
            int first = -1, cnt = 0;
            for (int g = 0; g < B; ++g) if (zl_group_bus_owner(g, B, n) == r) { if (first < 0) first = g; ++cnt; }
            L.first_bus[r] = first; L.num_buses[r] = cnt; L.first_slot[r] = 0; L.slots[r] = VPB;
        } else {
            L.first_bus[r] = 0; L.num_buses[r] = B; L.first_slot[r] = r * L.vl; L.slots[r] = L.vl;
        }
    }
    return ZLHIP_OK;
}

// member config: cfg with the member's buses / voices (device set by the caller)
inline zlhip_config zl_group_member_config(const ZlGroupLayout &L, const zlhip_config &cfg, int r)
{
    zlhip_config c = cfg;
    c.struct_size = sizeof(zlhip_config);
    c.num_buses = L.num_buses[r];
    c.voices_per_bus = L.vl;
    if (L.partition == ZLHIP_GROUP_SPAN) c.voices_per_task = 0;
    return c;
}

// bus-aligned: the member that owns a global bus and the bus's local index there
inline int zl_group_owner(const ZlGroupLayout &L, int bus, int *local)
{
    const int r = zl_group_bus_owner(bus, L.B, L.n);
    *local = bus - L.first_bus[r];
    return r;
}

// a member's local voice -> the global voice (bus * VPB + slot); -1 stays -1
inline int zl_group_global_voice(const ZlGroupLayout &L, int r, int local)
{
    if (local < 0) return -1;
    const int b = local / L.vl, s = local - b * L.vl;
    return (L.first_bus[r] + b) * L.VPB + L.first_slot[r] + s;
}

// One ClipCommand addressed by global midi channel (SamplerSynth::handleClipCommand + SamplerChannel::handleCommand) on the members'
// control planes m[0 .. n).  Returns what one engine with the whole config would return; *voice: the global voice it started, or -1.
template <class Ctl>
int zl_group_route_command(const ZlGroupLayout &L, Ctl *const *m, const zlhip_clip_command &c, uint64_t tick, int *voice)
{
    *voice = -1;
    const int bus = c.midi_channel + 2;                            // SamplerSynth.cpp:330-331
    if (bus < 0 || bus >= L.B) { for (int r = 0; r < L.n; ++r) m[r]->lastStartedVoice = -1; return 0; }
    if (L.partition == ZLHIP_GROUP_BUS_ALIGNED) {
        int lb;
        const int r = zl_group_owner(L, bus, &lb);
        zlhip_clip_command lc = c;
        lc.midi_channel = lb - 2;                                  // = midi_channel - first_bus: the member's own channel of the bus
        const int t = m[r]->handle_command(lc, tick);
        *voice = zl_group_global_voice(L, r, m[r]->lastStartedVoice);
        return t;
    }
    // span: the bus's voices in global slot order are member 0's slice, then member 1's ...
    int consumed = 0;
    if (c.start_playback) {
        // the start goes to the first member with a free voice; it applies the stop first (SamplerSynth.cpp:191-215), as the members
        // before it have, and the members after it apply the stop alone
        zlhip_clip_command stopOnly = c;
        stopOnly.start_playback = 0;
        for (int r = 0; r < L.n; ++r) {
            if (!consumed) {
                const int t = m[r]->handle_command(c, tick);
                if (t) { consumed = 1; *voice = zl_group_global_voice(L, r, m[r]->lastStartedVoice); }
            } else if (c.stop_playback) {
                m[r]->handle_command(stopOnly, tick);
            }
        }
    } else {
        // a stop or a merge (setCurrentCommand on every equivalent voice, :216-229) reaches every voice of the bus
        for (int r = 0; r < L.n; ++r) consumed |= m[r]->handle_command(c, tick);
    }
    return consumed;
}

// zlhip_start_voice over the group: the command on one addressed slot (its stop / merge still reach every voice of the bus, as
// handle_on_bus with a forced slot does)
template <class Ctl>
int zl_group_route_start_voice(const ZlGroupLayout &L, Ctl *const *m, int bus, int slot, const zlhip_clip_command &c, uint64_t tick)
{
    if (L.partition == ZLHIP_GROUP_BUS_ALIGNED) {
        int lb;
        const int r = zl_group_owner(L, bus, &lb);
        zlhip_clip_command lc = c;
        lc.midi_channel = c.midi_channel - L.first_bus[r];         // the shift of every command a member keeps (voice equivalence compares it)
        return m[r]->handle_on_bus(lb, lc, tick, slot);
    }
    const int owner = slot / L.vl;
    zlhip_clip_command stopOnly = c;
    stopOnly.start_playback = 0;
    int consumed = 0;
    for (int r = 0; r < L.n; ++r) {
        if (r == owner) consumed |= m[r]->handle_on_bus(bus, c, tick, slot - owner * L.vl);
        else if (!c.start_playback) consumed |= m[r]->handle_on_bus(bus, c, tick, 0);          // a merge of every equivalent voice
        else if (c.stop_playback) m[r]->handle_on_bus(bus, stopOnly, tick, 0);                   // the stop half of a stop + start
    }
    return consumed;
}

// (bus, slot) of the global surface -> (member, local bus, local slot)
inline int zl_group_locate(const ZlGroupLayout &L, int bus, int slot, int *lbus, int *lslot)
{
    if (L.partition == ZLHIP_GROUP_BUS_ALIGNED) { *lslot = slot; return zl_group_owner(L, bus, lbus); }
    *lbus = bus;
    const int r = slot / L.vl;
    *lslot = slot - r * L.vl;
    return r;
}
