"""What the engine-group tests share (no GPU, no HIP): the comparison helpers of tests/test_group_gpu.py, the slot-addressed scenes
of the span partition's shape tests and their case lists.  tests/test_group_shapes_cpu.py shows on the oracle alone that every
scene can fail -- the rank-order sum of the members' partials is the grouped mix and any other order is not --
tests/test_group_shapes_gpu.py runs the same scenes through a group on the device."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from libzl_amd import MODE_FAITHFUL, MODE_FIX_DELAY, MODE_HERMITE
from scenario import Scene, _segments, compare_runs, play_cmd, rand_source, run_backend, run_oracle

LEVEL_FIELDS = ("peak_a", "peak_b", "peak_a_hold_signal", "peak_b_hold_signal", "peak_db_a", "peak_db_b", "combined_db", "hold_db_a",
                "hold_db_b", "rms_a", "rms_b")
REPORT_FIELDS = ("playing", "valid", "gain", "progress", "clip", "source_sample_position")


def group(devices, partition, **extra):
    from libzl_amd import SamplerSynthGroup
    return lambda **kw: SamplerSynthGroup(devices, partition=partition, **kw, **extra)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def assert_same_bus(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), f"{what}: max abs diff {np.abs(a - b).max()} at {np.argwhere(a != b)[:3].tolist()}"


def assert_same_reports(r1, r2, V, what):
    for v in range(V):
        for f in REPORT_FIELDS:
            x, y = getattr(r1[v], f), getattr(r2[v], f)
            assert np.array(x).tobytes() == np.array(y).tobytes(), f"{what}: voice {v} {f}: {x} vs {y}"


def assert_same_levels(l1, l2, B, what):
    for b in range(B):
        for f in LEVEL_FIELDS:
            x, y = getattr(l1[b], f), getattr(l2[b], f)
            assert np.float32(x).tobytes() == np.float32(y).tobytes() if isinstance(x, float) else x == y, f"{what}: bus {b} {f}: {x} vs {y}"


def meters(syn, K, hold):
    """every block's levels (the hold bus kept across the ticks) and the block peaks of the last call"""
    return [syn.levels_tick(block_index=k, with_hold_bus=hold) for k in range(K)], syn.block_peaks()


def check_against(sc, factory, batch=1 << 30, hold=1):
    """run the scene on the oracle, one engine and the group; bus, reports, levels and peaks must agree bit for bit"""
    from libzl_amd import SamplerSynth
    ref, orep, osyn = run_oracle(sc, batch=batch)
    one, rep1, syn1, _ = run_backend(sc, SamplerSynth, batch=batch)
    grp, repg, syng, _ = run_backend(sc, factory, batch=batch)
    V = sc.num_buses * sc.voices_per_bus
    compare_runs(ref, orep, osyn, grp, repg, V)
    assert_same_bus(one, grp, "group vs one engine")
    assert_same_reports(rep1, repg, V, "group vs one engine")
    K = syn1._last[0]
    lv1, pk1 = meters(syn1, K, hold)
    lvg, pkg = meters(syng, K, hold)
    for k in range(K):
        assert_same_levels(lv1[k], lvg[k], sc.num_buses, f"levels, block {k}")
    assert np.array_equal(pk1, pkg)
    assert any(lv1[-1][b].rms_a > 0 for b in range(sc.num_buses))
    syn1.close()
    syng.close()
    return grp


# ---- the span partition's shape scenes ---------------------------------------------------------------------------------------
TILE = 64             # frames per tile of the sum kernel's scan


def _slot_idle(bus, slot, VPB):
    return (bus * VPB + slot) % 7 == 3


def _start(bus, slot, nsounds, restart=False):
    """the start of one slot: within a bus no two slots share (clip, note), so that no start stops another slot's voice
    (ClipCommand::equivalentTo) and a run filtered to one slice plays what the slice plays in the whole scene"""
    clip = (slot + 3 * bus) % nsounds
    return ("start", bus, slot, play_cmd(clip, midi_channel=bus - 2, loop=(slot % 9 != 4), note=50 + clip % 7 + slot // nsounds + (24 if restart else 0),
                                         volume=float(np.float32(0.15 + 0.02 * (slot % 13) + 0.05 * bus))), 0)


def span_scene(n, vl, B, N, K, mode, seed, only=None, mix=None, voice_calls=False, idle=None, cuts=()):
    """B buses of VPB = n * vl voices for a span group of n members, K blocks of N frames, mix_group = vl (or `mix`).  Seven to twelve
    sounds, mono and stereo, at 44.1 and 48 kHz, every one with its length set so that the voices move.  Block 0 starts every slot
    of every bus by slot -- notes, volumes and loop flags differ by slot, a few slots stay idle, never a whole slice.
    voice_calls: later events addressed by slot or by bus only -- stop_voice with and without tail-off, update_voice changing a
    volume, one bus disabled and enabled again.  idle = (member, stop, again): every slot of the member's slice is stopped without
    tail-off at block `stop` and started again at block `again`.  cuts: blocks at which the run is cut into calls with no event.
    only = r keeps the events addressed to slots of slice r (and every enable): the scene of member r's partial."""
    rng = np.random.default_rng(seed)
    VPB = n * vl
    sc = Scene(num_buses=B, voices_per_bus=VPB, fs=48000.0, mode=mode, mix_group=vl if mix is None else mix, nframes=N, nblocks=K)
    nsounds = 7 + seed % 6
    for i in range(nsounds):
        L, R = rand_source(rng, 2600 + 173 * i, stereo=(i % 3 != 2))
        sr = 44100.0 if i % 2 else 48000.0
        sc.sounds.append((L, R, sr))

        def setup(lib, clip, i=i):
            lib.zlo_clip_set_length(clip, C.c_float(0.06 + 0.007 * i), 120)      # 30 .. 70 ms of the 54 ms and more the sound holds
            lib.zlo_clip_set_pan(clip, C.c_float(-0.7 + 0.2 * (i % 8)))
            lib.zlo_clip_set_volume_absolute(clip, C.c_float(0.5 + 0.04 * i))
        sc.clip_setup[i] = setup
    ev = {0: [_start(b, s, nsounds) for b in range(B) for s in range(VPB) if not _slot_idle(b, s, VPB)]}
    for b in range(B):
        for r in range(n):
            assert any(e[1] == b and e[2] // vl == r for e in ev[0]), "a whole slice idle"
    if voice_calls:
        assert K >= 11 and B >= 2
        started = {(e[1], e[2]): e[3] for e in ev[0]}

        def volume(bus, slot, v):                                  # the voice's own command with another volume (SamplerSynthVoice::setCurrentCommand)
            f = started[(bus, slot)]
            return ("update", bus, slot, dict(clip=f["clip"], midiChannel=f["midiChannel"], midiNote=f["midiNote"], changeVolume=1, volume=v))
        first = min(s for (b, s) in started if b == 0)
        last = max(s for (b, s) in started if b == B - 1)          # in the last member's slice
        mid = min(s for (b, s) in started if b == 0 and s >= vl)   # in member 1's
        assert last >= VPB - vl and mid < 2 * vl
        ev[3] = [("stopv", 0, first, True), ("stopv", B - 1, last, False)]
        other = max(s for (b, s) in started if b == B - 1 and s != last)                 # a voice that still plays, of the highest slice that has one
        ev[5] = [volume(0, mid, 0.45), volume(B - 1, other, 0.07)]
        ev[7] = [("enable", 1, False)]
        ev[10] = [("enable", 1, True)]
    if idle is not None:
        member, stop, again = idle
        ev.setdefault(stop, []).extend(("stopv", b, s, False) for b in range(B) for s in range(member * vl, (member + 1) * vl))
        ev.setdefault(again, []).extend(_start(b, s, nsounds, restart=True) for b in range(B) for s in range(member * vl, (member + 1) * vl))
    for k in cuts:
        ev.setdefault(k, [])
    if only is not None:
        ev = {k: [e for e in lst if e[0] == "enable" or e[2] // vl == only] for k, lst in ev.items()}
    sc.events = ev
    return sc


@dataclass(frozen=True)
class SpanCase:
    name: str
    n: int
    N: int
    K: int
    mode: int
    seed: int
    vl: int = 2
    B: int = 2
    root: int = 0
    batch: int = 1 << 30
    voice_calls: bool = False
    idle: Optional[Tuple[int, int, int]] = None      # (member, stop block, start-again block)
    cuts: Tuple[int, ...] = ()
    uneven: bool = False                             # listed: some call has P % n != 0
    empty: bool = False                              # listed: some call leaves a member without a pair

    @property
    def tail(self):
        """frames of the last tile that the f < N mask keeps, 0 = a whole tile: off = 1 (the front frame) or 0 by mode"""
        return (self.N - (0 if self.mode & MODE_FIX_DELAY else 1)) % TILE

    def scene(self, only=None, mix=None):
        return span_scene(self.n, self.vl, self.B, self.N, self.K, self.mode, self.seed, only=only, mix=mix, voice_calls=self.voice_calls,
                          idle=self.idle, cuts=self.cuts)

    def calls(self):
        """(first block, blocks) of every render call of the scene"""
        return _segments(self.scene(), self.batch)

    def factory(self):
        return group([0] * self.n, "span", root=self.root)


def shares(P, n):
    """the pairs of each member of a call with P = K * B (block, bus) pairs, as zlhip_group_render_batch cuts them"""
    return [P * (r + 1) // n - P * r // n for r in range(n)]


_MODE_NAMES = {MODE_FAITHFUL: "faithful", MODE_FIX_DELAY: "fixdelay", MODE_HERMITE: "hermite"}

# every member count the sum kernel is instantiated for and that tests/test_group_gpu.py leaves out; K = 12 cut by the voice-level
# events into calls of 3, 2, 2, 3 and 2 blocks: P = 9 and 6 with B = 3, no multiple of 5, 7 or 8
MEMBER_CASES = [SpanCase(f"n{n}-{_MODE_NAMES[mode]}", n, 128, 12, mode, 40 + n, B=3, voice_calls=True, uneven=n != 3, empty=n >= 7)
                for n, mode in [(3, MODE_FAITHFUL), (5, MODE_FAITHFUL), (6, MODE_FAITHFUL), (7, MODE_FAITHFUL), (8, MODE_FAITHFUL),
                                (3, MODE_HERMITE), (8, MODE_HERMITE), (3, MODE_FIX_DELAY), (8, MODE_FIX_DELAY)]]

# one call of K = 5 blocks on B = 2 buses, n = 3: P = 10, shares 3, 3 and 4.  N: one partial tile; a tile that exactly fills (off = 0) or
# falls one short (off = 1); one frame into a second tile; a partial second tile; seven tiles with a tail
BLOCK_SIZE_CASES = [SpanCase(f"N{N}-{_MODE_NAMES[mode]}", 3, N, 5, mode, 60 + N % 17, uneven=True)
                    for N in (33, 64, 65, 100, 441) for mode in (MODE_FAITHFUL, MODE_FIX_DELAY)]
# ... and the four-tap interpolation with the fixed delay (mode 6): the sum kernel's front-frame handling goes by MODE_FIX_DELAY alone
BLOCK_SIZE_CASES.append(SpanCase("N100-hermite-fixdelay", 3, 100, 5, MODE_HERMITE | MODE_FIX_DELAY, 66, uneven=True))

ROOT_CASES = [SpanCase("n3-root1", 3, 128, 12, MODE_FAITHFUL, 71, B=3, root=1, voice_calls=True),
              SpanCase("n3-root2", 3, 100, 12, MODE_FIX_DELAY, 72, B=3, root=2, voice_calls=True),
              SpanCase("n8-root7", 8, 128, 12, MODE_FAITHFUL, 73, B=3, root=7, voice_calls=True, uneven=True, empty=True)]

# P = 2 pairs for 8 members: six members have nothing to sum; then a call of K = 3 on the same group (P = 6: two still have nothing)
EMPTY_SHARE_CASES = [SpanCase("n8-K1-then-K3", 8, 128, 4, MODE_FAITHFUL, 81, cuts=(1,), uneven=True, empty=True)]

# one-block calls of members 32 voices wide: every member splits its bus into one voice per workgroup before the group sums
WIDE_CASES = [SpanCase(f"n{n}-vl32-N{N}", n, N, 2, MODE_FAITHFUL, 90 + n + N % 7, vl=32, batch=1, uneven=n == 4, empty=n == 4)
              for n in (2, 4) for N in (128, 100)]

IDLE_CASES = [SpanCase("n4-member2-idle", 4, 128, 12, MODE_FAITHFUL, 97, idle=(2, 4, 8))]

SPAN_CASES = MEMBER_CASES + BLOCK_SIZE_CASES + ROOT_CASES + EMPTY_SHARE_CASES + WIDE_CASES + IDLE_CASES

# the three calls of the bus_out_dev test (n = 3, root = 2): the layout [B][2][K * N] changes between the calls
ROOT_OUT_CALLS = (5, 2, 5)
ROOT_OUT_CASE = SpanCase("n3-root2-bus-out", 3, 100, sum(ROOT_OUT_CALLS), MODE_FAITHFUL, 75, root=2, cuts=(5, 7), uneven=True)


def case_id(c):
    return c.name


_partials = {}


def oracle_runs(case):
    """(the oracle's grouped mix, its reports, its synth, [member r's partial: the oracle with mix_group = 0 on the events of slice r]),
    computed once per session and shared read-only"""
    if case not in _partials:
        ref, orep, osyn = run_oracle(case.scene(), batch=case.batch)
        parts = [run_oracle(case.scene(only=r, mix=0), batch=case.batch)[0] for r in range(case.n)]
        for a in [ref] + parts:
            a.setflags(write=False)
        _partials[case] = (ref, orep, osyn, parts)
    return _partials[case]


def rank_sum(parts, order):
    """((0 + p[order[0]]) + p[order[1]]) + ... in fp32"""
    acc = np.zeros_like(parts[0])
    for r in order:
        acc = acc + parts[r]
    return acc
