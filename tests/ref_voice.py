"""Drives oracle/_ref/libzl_refvoice.so -- the reference's own SamplerSynthVoice.cpp, compiled unmodified (libzl_amd/build.py
build_reference, oracle/ref_driver.cpp) -- with a scenario.Scene, in lockstep with the C oracle.  TEST INFRASTRUCTURE ONLY.

What the anchor pins is the voice: setCurrentCommand, startNote, stopNote and process.  Everything around it stays a restatement and
is handed to BOTH sides by this module, so that a difference can only come from the voice:
  * SamplerSynth::handleClipCommand (which voice takes a command) is decided here from the oracle's voice state and issued to both
    sides as the same voice-level calls;
  * slice start / stop positions, the root note, the envelope parameters and subbeatCountToSeconds come from the oracle's clip
    functions and are copied into the driver's getters;
  * juce::ADSR and the positions model's row bookkeeping are the oracle's code on both sides (linked into the library).
The reference stores frame f to buffer[f + 1], up to buffer[nframes]: a channel's buffers in the driver are nframes + 1 floats.
Elements 0 .. nframes - 1 are the block the oracle renders; element [nframes] is the frame the oracle computes and drops, which the
oracle in ZLO_MODE_FIX_DELAY (same arithmetic, frame f stored to [f]) keeps as the block's last frame -- compared as `tail`.

Outside the anchor (OutsideAnchor): a note started with startTick + lengthInBeats * 96 negative (or not below 2^64).  The conversion
of such a float to quint64 is undefined in C++; the oracle takes the aarch64 result (saturation to 0, quirk Q10), an x86-64 build yields another."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from oracle import zl_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libzl_refvoice.so")
SLICE_ENTRIES = zo.MAX_SLICES + 1
_FP = C.POINTER(C.c_float)


class OutsideAnchor(Exception):
    pass


_libs = {}


def build():
    """-> path of the library, or None where there is neither a reference tree nor a library that travelled here.  Raises where the
    tree is present and the build fails."""
    from libzl_amd import build as b
    path = b.build_reference()
    if path is None and os.path.exists(REF_LIB):
        path = REF_LIB
    return path


def load(path=None):
    path = path or build()
    if path is None:
        return None
    if path in _libs:
        return _libs[path]
    lib = C.CDLL(path)
    sig = {
        "zr_world_new": (C.c_void_p, [C.c_int, C.c_int, C.c_double]),
        "zr_world_free": (None, [C.c_void_p]),
        "zr_add_sound": (C.c_int, [C.c_void_p, _FP, _FP, C.c_int, C.c_double]),
        "zr_set_clip": (None, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(zo.AdsrParams), C.c_void_p, C.c_void_p]),
        "zr_set_timer": (None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_float]),
        "zr_set_current_command": (None, [C.c_void_p, C.c_int, C.c_int, C.POINTER(zo.ClipCommand)]),
        "zr_set_start_tick": (None, [C.c_void_p, C.c_int, C.c_int, C.c_uint64]),
        "zr_start_note": (None, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]),
        "zr_stop_note": (None, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        "zr_is_playing": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
        "zr_channel_process": (None, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(zo.Report)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _libs[path] = lib
    return lib


class _Pair:
    """One scene on both sides: every voice-level call goes to the oracle's voice and to the reference's."""

    def __init__(self, scene, ref):
        assert scene.mode == 0, "the anchor is the reference-faithful mode"
        self.sc, self.ref, self.olib = scene, ref, zo.load()
        self.B, self.VPB = scene.num_buses, scene.voices_per_bus
        self.osyn = zo.OracleSynth(self.B, self.VPB, scene.fs, 0, max_sounds=max(8, len(scene.sounds)))
        self.w = ref.zr_world_new(self.B, self.VPB, scene.fs)
        for i, (L, R, sr) in enumerate(scene.sounds):
            assert self.osyn.register_clip(L, R, sr) == i
            s = self.osyn.sounds[i]
            assert ref.zr_add_sound(self.w, s.L, s.R, s.length, s.sampleRate) == i
            if i in scene.clip_setup:
                scene.clip_setup[i](self.olib, self.osyn.clips[i])
            self.sync_clip(i)

    def close(self):
        self.ref.zr_world_free(self.w)
        self.w = None

    def sync_clip(self, i):
        clip, rate = self.osyn.clips[i], self.osyn.sounds[i].sampleRate
        start = np.zeros(SLICE_ENTRIES, dtype=np.float32)
        stop = np.zeros(SLICE_ENTRIES, dtype=np.int32)
        for e in range(SLICE_ENTRIES):
            start[e] = self.olib.zlo_clip_get_start_position(C.byref(clip), e - 1)
            stop[e] = int(float(self.olib.zlo_clip_get_stop_position(C.byref(clip), e - 1)) * rate)     # SamplerSynthSound.cpp:101-104: (int)(float * double)
        self.ref.zr_set_clip(self.w, i, clip.volumeAbsolute, clip.pan, clip.lengthInBeats, clip.duration, clip.rootNote, C.byref(clip.adsr.p),
                             start.ctypes.data, stop.ctypes.data)

    # ---- the voice-level calls, to both sides
    def voice(self, bus, slot):
        return self.osyn.channels[bus].voices[slot]

    def set_cmd(self, bus, slot, cmd):
        self.olib.zlo_voice_set_current_command(C.byref(self.voice(bus, slot)), C.byref(cmd), self.osyn.clips, self.osyn.sounds)
        self.ref.zr_set_current_command(self.w, bus, slot, C.byref(cmd))

    def start_tick(self, bus, slot, tick):
        self.voice(bus, slot).startTick = tick
        self.ref.zr_set_start_tick(self.w, bus, slot, tick)

    def start_note(self, bus, slot, cmd):
        v = self.voice(bus, slot)
        assert v.sound < 0, "a voice that is not playing but still holds a sound: the reference dereferences a null command here"
        beats = np.float32(self.osyn.clips[cmd.clip].lengthInBeats)
        if not (0 <= np.float32(v.startTick) + beats * np.float32(96) < np.float32(2.0 ** 64)):
            raise OutsideAnchor("startTick + lengthInBeats * 96 is negative or beyond 2^64: float -> quint64 is undefined (quirk Q10)")
        self.olib.zlo_voice_start_note(C.byref(v), cmd.midiNote, cmd.volume, cmd.clip, self.osyn.sounds, self.osyn.clips, self.sc.fs, 0)
        self.ref.zr_start_note(self.w, bus, slot, cmd.midiNote, cmd.volume, cmd.clip)

    def stop_note(self, bus, slot, tail):
        self.olib.zlo_voice_stop_note(C.byref(self.voice(bus, slot)), 1 if tail else 0, self.osyn.clips, 0)
        self.ref.zr_stop_note(self.w, bus, slot, 1 if tail else 0)

    # ---- SamplerSynth.cpp:187-230 / the engine's voice-level entry points, decided on the oracle's voice state
    def _matches(self, v, cmd):
        return v.sound >= 0 and v.sound == cmd.clip and v.hasCommand and self.olib.zlo_clip_command_equivalent(C.byref(v.cmd), C.byref(cmd))

    def _stop_equivalent(self, bus, cmd):
        for i in range(self.VPB):
            if self._matches(self.voice(bus, i), cmd):
                self.stop_note(bus, i, True)

    def _start_on(self, bus, slot, cmd, tick):
        self.set_cmd(bus, slot, cmd)
        self.start_tick(bus, slot, tick)
        self.start_note(bus, slot, cmd)

    def handle(self, cmd, tick):
        bus = cmd.midiChannel + 2
        if bus < 0 or bus >= self.B or cmd.clip < 0 or cmd.clip >= self.osyn.nsounds:
            return
        if cmd.stopPlayback or cmd.startPlayback:
            if cmd.stopPlayback:
                self._stop_equivalent(bus, cmd)
            if cmd.startPlayback:
                for i in range(self.VPB):
                    if not self.voice(bus, i).isPlaying:
                        self._start_on(bus, i, cmd, tick)
                        break
        else:
            for i in range(self.VPB):
                if self._matches(self.voice(bus, i), cmd):
                    self.set_cmd(bus, i, cmd)

    def event(self, ev):
        if ev[0] == "cmd":
            self.handle(zo.clip_command(**ev[1]), ev[2])
        elif ev[0] == "start":
            cmd = zo.clip_command(**ev[3])
            if cmd.stopPlayback:
                self._stop_equivalent(ev[1], cmd)
            if cmd.startPlayback and not self.voice(ev[1], ev[2]).isPlaying:
                self._start_on(ev[1], ev[2], cmd, ev[4])
        elif ev[0] == "update":
            if self.voice(ev[1], ev[2]).isPlaying:
                self.set_cmd(ev[1], ev[2], zo.clip_command(**ev[3]))
        elif ev[0] == "stopv":
            if self.voice(ev[1], ev[2]).isPlaying:
                self.stop_note(ev[1], ev[2], bool(ev[3]))
        elif ev[0] == "enable":
            self.osyn.set_bus_enabled(ev[1], ev[2])
        elif ev[0] == "clip":
            ev[2](self.olib, self.osyn.clips[ev[1]])
            self.sync_clip(ev[1])
        else:
            raise AssertionError(ev[0])

    def kept_last_frame(self, bus, N, clk):
        """the block's last frame as ZLO_MODE_FIX_DELAY keeps it, rendered on copies of the channel's voices and of the clips"""
        voices = (zo.Voice * self.VPB)()
        C.memmove(voices, self.osyn.channels[bus].voices, C.sizeof(voices))
        clips = type(self.osyn.clips)()
        C.memmove(clips, self.osyn.clips, C.sizeof(clips))
        ch = zo.Channel(C.cast(voices, C.POINTER(zo.Voice)), self.VPB, bus - 2, 1)
        L, R = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
        self.olib.zlo_channel_process(C.byref(ch), L.ctypes.data, R.ctypes.data, N, C.byref(clk), self.osyn.sounds, clips, zo.MODE_FIX_DELAY, 0, None)
        return L[N - 1], R[N - 1]


def run_reference(scene, lib_path=None):
    """Plays `scene` (mode 0) on the compiled reference voice and on the C oracle, block by block.
    -> dict of two sides, "ref" and "oracle", each with bus [B][2][K*N] f32, tail [K][B][2] f32 (the frame stored to [nframes]; the
    oracle's from ZLO_MODE_FIX_DELAY), reports [K][V][3] f32 (valid, gain, progress), playing [K][V] u8 (isPlaying after the block)."""
    ref = load(lib_path)
    if ref is None:
        raise RuntimeError("no reference library")
    p = _Pair(scene, ref)
    try:
        B, VPB, K = p.B, p.VPB, scene.nblocks
        N, total = scene.nframes, K * scene.nframes
        out = {side: dict(bus=np.zeros((B, 2, total), dtype=np.float32), tail=np.zeros((K, B, 2), dtype=np.float32),
                          reports=np.zeros((K, B * VPB, 3), dtype=np.float32), playing=np.zeros((K, B * VPB), dtype=np.uint8))
               for side in ("ref", "oracle")}
        one_subbeat = p.olib.zlo_subbeat_count_to_seconds(scene.bpm, 1)
        at = 0
        for k in range(K):
            for ev in scene.events.get(k, []):
                p.event(ev)
            ck = scene.make_clocks(k, 1)[0]
            clk = zo.Clock(int(ck.current_usecs), int(ck.next_usecs), int(ck.jack_playhead), int(ck.jack_playhead_usecs), int(ck.jack_subbeat_length_usecs))
            ref.zr_set_timer(clk.jackPlayhead, clk.jackPlayheadUsecs, clk.jackSubbeatLengthInMicroseconds, scene.bpm, 96, one_subbeat)
            for b in range(B):
                if not p.osyn.channels[b].enabled:          # SamplerSynth.cpp:123: the channel is not processed at all
                    for i in range(VPB):
                        out["oracle"]["playing"][k, b * VPB + i] = p.voice(b, i).isPlaying
                        out["ref"]["playing"][k, b * VPB + i] = ref.zr_is_playing(p.w, b, i)
                    continue
                out["oracle"]["tail"][k, b] = p.kept_last_frame(b, N, clk)
                L, R = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
                oreps = (zo.Report * VPB)()
                p.olib.zlo_channel_process(C.byref(p.osyn.channels[b]), L.ctypes.data, R.ctypes.data, N, C.byref(clk), p.osyn.sounds, p.osyn.clips, 0, 0, oreps)
                rL, rR = np.zeros(N + 1, dtype=np.float32), np.zeros(N + 1, dtype=np.float32)
                rreps = (zo.Report * VPB)()
                ref.zr_channel_process(p.w, b, N, clk.current_usecs, clk.next_usecs, rL.ctypes.data, rR.ctypes.data, rreps)
                out["oracle"]["bus"][b, 0, at:at + N], out["oracle"]["bus"][b, 1, at:at + N] = L, R
                out["ref"]["bus"][b, 0, at:at + N], out["ref"]["bus"][b, 1, at:at + N] = rL[:N], rR[:N]
                out["ref"]["tail"][k, b] = (rL[N], rR[N])
                for i in range(VPB):
                    out["oracle"]["reports"][k, b * VPB + i] = (oreps[i].valid, oreps[i].gain, oreps[i].progress)
                    out["ref"]["reports"][k, b * VPB + i] = (rreps[i].valid, rreps[i].gain, rreps[i].progress)
                    out["oracle"]["playing"][k, b * VPB + i] = p.voice(b, i).isPlaying
                    out["ref"]["playing"][k, b * VPB + i] = ref.zr_is_playing(p.w, b, i)
            at += N
        return out
    finally:
        p.close()


def same_bits_nan_aware(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def assert_sides_equal(out, what=""):
    """the reference voice and the oracle, bit for bit: audio (NaN frames as "NaN in the same frames"), the frame stored to
    [nframes], isPlaying after every block, every block's report (validity, gain, progress = sourceSamplePosition / length)"""
    r, o = out["ref"], out["oracle"]
    if not same_bits_nan_aware(r["bus"], o["bus"]):
        d = np.argwhere(r["bus"].view(np.int32) != o["bus"].view(np.int32))
        raise AssertionError(f"{what}: audio differs in {len(d)} samples, first at [bus, channel, frame] {d[0].tolist()}: "
                             f"reference {r['bus'][tuple(d[0])]!r}, oracle {o['bus'][tuple(d[0])]!r}")
    assert np.array_equal(r["playing"], o["playing"]), f"{what}: isPlaying differs at [block, voice] {np.argwhere(r['playing'] != o['playing'])[:3].tolist()}"
    assert same_bits_nan_aware(r["reports"], o["reports"]), \
        f"{what}: reports differ at [block, voice, field] {np.argwhere(r['reports'].view(np.int32) != o['reports'].view(np.int32))[:3].tolist()}"
    assert same_bits_nan_aware(r["tail"], o["tail"]), \
        f"{what}: the frame stored to [nframes] differs at [block, bus, channel] {np.argwhere(r['tail'].view(np.int32) != o['tail'].view(np.int32))[:3].tolist()}"
