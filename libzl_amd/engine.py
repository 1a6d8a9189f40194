"""Python binding of the C-ABI in include/zlhip.h (ctypes; no torch types cross the boundary).

Names follow the reference's domain: a SamplerSynth owns `num_buses` SamplerChannels of
`voices_per_bus` voices (SamplerSynth.cpp:254-278); clips are registered once
(SamplerSynth::registerClip, :285-295) and played through ClipCommands (ClipCommand.h:11-32).
Every sample is produced by the HIP kernels behind libzlhip.so; this module only marshals.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import (Clock, ClipCommand, ClipParams, Config, Levels, PassthroughParams, RerenderParams, Timings, VoiceReport,
                   MODE_FAITHFUL, MODE_FIX_DELAY, MODE_FIX_GAIN, MODE_HERMITE, ZlHipError)

__all__ = ["SamplerSynth", "SamplerSynthGroup", "Clock", "ClipCommand", "ClipParams", "Levels", "PassthroughParams", "VoiceReport",
           "MODE_FAITHFUL", "MODE_FIX_GAIN", "MODE_FIX_DELAY", "MODE_HERMITE", "ZlHipError", "clip_command", "synthetic_clocks", "running_playhead", "live_resources"]


def clip_command(lib=None, **fields) -> ClipCommand:
    """ClipCommand with the reference's defaults (ClipCommand.h:13-32) and the given fields set."""
    c = ClipCommand()
    c.clip = -1
    c.midi_note = -1
    c.midi_channel = -1
    c.slice = -1
    for k, v in fields.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


_running_playheads: dict = {}


def running_playhead(block: int, period: int, bpm: int):
    """(jackPlayhead, jackPlayheadUsecs) as a SyncTimer that was started at time 0 leaves them after its process call for the
    JACK cycle [block * period, (block + 1) * period): one step per subbeat while its time lies before the cycle's end, the step
    time accumulated as `quint64 += double` (SyncTimer.cpp:484,512,660-667,990-1004)."""
    key = (period, bpm)
    rows = _running_playheads.setdefault(key, [])
    sub = float((60000000000 // (bpm * 96))) / 1000.0
    # jackNextPlaybackPosition = current_usecs of the first cycle = 0; the step clock runs in parallel from 0 as well
    n, pos = rows[-1] if rows else (0, 0)
    while len(rows) <= block:
        nxt = (len(rows) + 1) * period
        while pos < nxt:
            n += 1
            pos = int(float(pos) + sub)
        rows.append((n, pos))
    return rows[block]


def synthetic_clocks(nblocks: int, nframes: int, sample_rate: float, start_block: int = 0, bpm: int = 120,
                     moving_playhead: bool = False) -> "C.Array[Clock]":
    """Monotone JACK-like cycle times: current_usecs = k * round(1e6 * nframes / fs).
    The SyncTimer playhead is held at tick 0 / usec 0 with the subbeat length of `bpm` (SyncTimer.cpp:180-183,959) -- a
    stopped timer before its first cycle -- or, with moving_playhead, advances as a running timer's does (running_playhead)."""
    period = int(round(1e6 * nframes / sample_rate))
    subbeat = ((1 * 60000000000) // (bpm * 96)) // 1000
    arr = (Clock * nblocks)()
    for k in range(nblocks):
        kk = start_block + k
        arr[k].current_usecs = kk * period
        arr[k].next_usecs = (kk + 1) * period
        if moving_playhead:
            arr[k].jack_playhead, arr[k].jack_playhead_usecs = running_playhead(kk, period, bpm)
        else:
            arr[k].jack_playhead = 0
            arr[k].jack_playhead_usecs = 0
        arr[k].jack_subbeat_length_usecs = subbeat
    return arr


def pinned_array(lib, shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (zlhip_host_alloc); freed when the array and its views are gone."""
    import weakref
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    if lib.zlhip_host_alloc(max(nbytes, 1), C.byref(p)) != 0 or not p.value:
        raise MemoryError(f"zlhip_host_alloc({nbytes}) failed")
    buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
    weakref.finalize(buf, lib.zlhip_host_free, p.value)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def live_resources(lib=None) -> tuple:
    """debug: (device buffers, page-locked host buffers, events, streams) the process's engines hold now (zlhip_debug_live_resources)"""
    counts = (C.c_int32 * 4)()
    if (lib or _abi.load()).zlhip_debug_live_resources(counts) != 0:
        raise ZlHipError("zlhip_debug_live_resources failed")
    return tuple(counts)


def _overview_requests(requests, length_of):
    """(clip, columns[, first_frame[, num_frames]]) tuples -> the C request array; num_frames None / missing = to the end of the clip"""
    reqs = (_abi.OverviewRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        clip, columns = int(r[0]), int(r[1])
        first = int(r[2]) if len(r) > 2 else 0
        n = r[3] if len(r) > 3 else None
        reqs[i] = _abi.OverviewRequest(clip, first, int(length_of(clip) - first if n is None else n), columns)
    return reqs


def _overview_split(out, reqs, count):
    """the packed columns of a batch -> one [columns, 4] view per request"""
    res, at = [], 0
    for i in range(count):
        res.append(out[at:at + reqs[i].columns])
        at += reqs[i].columns
    return res


def _onset_requests(requests, length_of):
    """(clip[, first_frame[, num_frames[, hop[, gate[, threshold[, min_gap[, max_onsets]]]]]]]) tuples -> the C request array and the
    onsets `out` must hold; num_frames None / missing = to the end of the clip, every other field 0 / missing = its default"""
    reqs = (_abi.OnsetRequest * max(1, len(requests)))()
    capacity = 0
    for i, r in enumerate(requests):
        r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
        clip = int(r[0])
        first = int(r[1]) if len(r) > 1 else 0
        n = r[2] if len(r) > 2 else None
        rest = [int(v) for v in r[3:8]] + [0] * (8 - max(3, len(r)))
        reqs[i] = _abi.OnsetRequest(clip, first, int(length_of(clip) - first if n is None else n), *rest)
        capacity += rest[4] if rest[4] > 0 else 128                # (zl_onset.h: the default of max_onsets)
    return reqs, capacity


def _onsets_call(fn, handle, requests, length_of):
    """one zlhip_sound_onsets_batch-shaped call -> one int32 [count, 2] array (frame, strength) per request; (status, arrays)"""
    reqs, capacity = _onset_requests(requests, length_of)
    out = np.zeros((max(capacity, 1), 2), np.int32)
    counts = np.zeros(max(1, len(requests)), np.int32)
    rc = fn(handle, reqs, len(requests), out.ctypes.data, capacity, counts.ctypes.data)
    res, at = [], 0
    for i in range(len(requests)):
        res.append(out[at:at + counts[i]])
        at += int(counts[i])
    return rc, res


PITCH_FIELDS = tuple(name for name, _ in _abi.Pitch._fields_)
PITCH_FRAME_FIELDS = tuple(name for name, _ in _abi.PitchFrame._fields_)
_PITCH_KEYS = ("first_frame", "num_frames", "window", "max_frames", "f_min", "f_max", "threshold", "gate")


def _pitch_call(fn, handle, requests, length_of):
    """one zlhip_sound_pitch_batch-shaped call over (clip[, first_frame[, num_frames[, window[, max_frames[, f_min[, f_max[, threshold[, gate]]]]]]]])
    tuples, or dicts with "clip" and any of those keys (num_frames None / missing = to the end of the clip, every other field 0 / missing =
    its default) -> (status, one dict of zlhip_pitch's fields per request)"""
    reqs = (_abi.PitchRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        if isinstance(r, dict):
            r = (r["clip"],) + tuple(r.get(k, None if k == "num_frames" else 0) for k in _PITCH_KEYS)
        r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
        r = r + (0, None, 0, 0, 0.0, 0.0, 0, 0)[len(r) - 1:]
        clip, first = int(r[0]), int(r[1])
        reqs[i] = _abi.PitchRequest(clip, first, int(length_of(clip) - first if r[2] is None else r[2]), int(r[3]), int(r[4]), float(r[5]), float(r[6]), int(r[7]), int(r[8]))
    out = (_abi.Pitch * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in PITCH_FIELDS} for i in range(len(requests))]


LOUDNESS_FIELDS = tuple(name for name, _ in _abi.Loudness._fields_)


def _loudness_call(fn, handle, requests, length_of):
    """one zlhip_sound_loudness_batch-shaped call over (clip[, first_frame[, num_frames[, sub_frames]]]) tuples, or dicts with "clip" and any
    of those keys (num_frames None / missing = to the end of the clip, sub_frames 0 / missing = 100 ms) -> (status, one dict of
    zlhip_loudness's fields per request; peak is a pair)"""
    reqs = (_abi.LoudnessRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        if isinstance(r, dict):
            r = (r["clip"], r.get("first_frame", 0), r.get("num_frames"), r.get("sub_frames", 0))
        r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
        r = r + (0, None, 0)[len(r) - 1:]
        clip, first = int(r[0]), int(r[1])
        reqs[i] = _abi.LoudnessRequest(clip, first, int(length_of(clip) - first if r[2] is None else r[2]), int(r[3]))
    out = (_abi.Loudness * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: (tuple(out[i].peak) if k == "peak" else getattr(out[i], k)) for k in LOUDNESS_FIELDS} for i in range(len(requests))]


LOOP_FIELDS = tuple(name for name, _ in _abi.Loop._fields_ if name != "reserved")
LOOP_ITEM_FIELDS = tuple(name for name, _ in _abi.LoopItem._fields_)
_LOOP_KEYS = ("start_frame", "stop_frame", "start_search", "stop_search", "window", "min_length")


def _loop_call(fn, handle, requests):
    """one zlhip_sound_loop_batch-shaped call over (clip, start_frame, stop_frame[, start_search[, stop_search[, window[, min_length]]]]) tuples,
    or dicts with "clip", "start_frame", "stop_frame" and any of the other keys (0 / missing = the default, a search of -1 = the point
    stays) -> (status, one dict of zlhip_loop's fields per request)"""
    reqs = (_abi.LoopRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        if isinstance(r, dict):
            r = (r["clip"],) + tuple(r.get(k, 0) for k in _LOOP_KEYS)
        r = tuple(r) + (0, 0, 0, 0)[len(r) - 3:]
        reqs[i] = _abi.LoopRequest(*(int(v) for v in r))
    out = (_abi.Loop * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in LOOP_FIELDS} for i in range(len(requests))]


XFADE_FIELDS = tuple(name for name, _ in _abi.Xfade._fields_ if name != "reserved")
_XFADE_KEYS = ("start_frame", "stop_frame", "fade_frames", "curve")


def _xfade_call(fn, handle, requests):
    """one zlhip_sound_loop_crossfade_batch-shaped call over (clip, start_frame, stop_frame[, fade_frames[, curve]]) tuples, or dicts with
    "clip", "start_frame", "stop_frame" and either of the other keys (fade_frames 0 / missing = 20 ms, curve 0 / missing = from the measured
    correlation) -> (status, one dict of zlhip_xfade's fields per request)"""
    reqs = (_abi.XfadeRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        if isinstance(r, dict):
            r = (r["clip"],) + tuple(r.get(k, 0) for k in _XFADE_KEYS)
        r = tuple(r) + (0, 0)[len(r) - 3:]
        reqs[i] = _abi.XfadeRequest(*(int(v) for v in r))
    out = (_abi.Xfade * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in XFADE_FIELDS} for i in range(len(requests))]


EDIT_FIELDS = tuple(name for name, _ in _abi.Edit._fields_ if name != "reserved")
_EDIT_KEYS = tuple(name for name, _ in _abi.EditRequest._fields_[1:])


def _edit_call(fn, handle, requests):
    """one zlhip_sound_edit_batch-shaped call over dicts with "clip" and any of zlhip_edit_request's other fields (missing = 0: the
    whole clip, no flag, no fade, the default threshold) -> (status, one dict of zlhip_edit's fields per request)"""
    reqs = (_abi.EditRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        reqs[i] = _abi.EditRequest(int(r["clip"]), *(int(r.get(k, 0)) for k in _EDIT_KEYS[:-1]), float(r.get("threshold", 0.0)))
    out = (_abi.Edit * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in EDIT_FIELDS} for i in range(len(requests))]


LIMIT_FIELDS = tuple(name for name, _ in _abi.Limit._fields_ if name != "reserved")


def _peak_call(fn, handle, requests):
    """one zlhip_sound_peak_batch-shaped call over dicts with "clip", "first_frame", "num_frames" (0: to the end of `length`, which the
    caller fills in) and "flags" -> (status, one dict of zlhip_peak's fields per request)"""
    reqs = (_abi.PeakRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        reqs[i] = _abi.PeakRequest(int(r["clip"]), int(r.get("first_frame", 0)), int(r.get("num_frames", 0)), int(r.get("flags", 0)))
    out = (_abi.Peak * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [dict(sample_peak=tuple(out[i].sample_peak), true_peak=tuple(out[i].true_peak), oversampling=out[i].oversampling, chunks=out[i].chunks)
                for i in range(len(requests))]


def _limit_call(fn, handle, requests):
    """one zlhip_sound_limit_batch-shaped call over dicts with "clip" and any of zlhip_limit_request's other fields (missing = 0: the
    default) -> (status, one dict of zlhip_limit's fields per request)"""
    reqs = (_abi.LimitRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        reqs[i] = _abi.LimitRequest(int(r["clip"]), int(r.get("flags", 0)), int(r.get("lookahead_frames", 0)), int(r.get("hold_frames", 0)),
                                    float(r.get("ceiling", 0.0)), float(r.get("gain", 0.0)))
    out = (_abi.Limit * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in LIMIT_FIELDS} for i in range(len(requests))]


WARP_FIELDS = tuple(name for name, _ in _abi.Warp._fields_)


def _warp_call(fn, handle, requests):
    """one zlhip_sound_warp_batch-shaped call over (clip, anchors) pairs, anchors a sequence of (src_frame, dst_frame)
    -> (status, one dict of zlhip_warp's fields per request)"""
    reqs = (_abi.WarpRequest * max(1, len(requests)))()
    keep = []
    for i, (clip, anchors) in enumerate(requests):
        a = np.ascontiguousarray(np.asarray(anchors, np.int32).reshape(-1, 2))
        keep.append(a)
        reqs[i] = _abi.WarpRequest(int(clip), int(a.shape[0]), C.cast(a.ctypes.data, C.POINTER(_abi.WarpAnchor)))
    out = (_abi.Warp * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in WARP_FIELDS} for i in range(len(requests))]


KEY_FIELDS = tuple(name for name, _ in _abi.Key._fields_)
_KEY_KEYS = ("first_frame", "num_frames", "hop", "max_frames", "a4_hz", "note_lo", "note_hi", "q", "gate")


def _key_call(fn, handle, requests, length_of):
    """one zlhip_sound_key_batch-shaped call over (clip[, first_frame[, num_frames[, hop[, max_frames[, a4_hz[, note_lo[, note_hi[, q[, gate]]]]]]]]])
    tuples, or dicts with "clip" and any of those keys (num_frames None / missing = to the end of the clip, every other field 0 / missing =
    its default) -> (status, one dict of zlhip_key's fields per request; chroma a tuple of twelve integers)"""
    reqs = (_abi.KeyRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        if isinstance(r, dict):
            r = (r["clip"],) + tuple(r.get(k, None if k == "num_frames" else 0) for k in _KEY_KEYS)
        r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
        r = r + (0, None, 0, 0, 0.0, 0, 0, 0, 0)[len(r) - 1:]
        clip, first = int(r[0]), int(r[1])
        reqs[i] = _abi.KeyRequest(clip, first, int(length_of(clip) - first if r[2] is None else r[2]), int(r[3]), int(r[4]), float(r[5]), int(r[6]), int(r[7]), int(r[8]), int(r[9]))
    out = (_abi.Key * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: (tuple(int(v) for v in out[i].chroma) if k == "chroma" else getattr(out[i], k)) for k in KEY_FIELDS} for i in range(len(requests))]


TEMPO_FIELDS = tuple(name for name, _ in _abi.Tempo._fields_ if name != "reserved")


def _tempo_call(fn, handle, requests, length_of):
    """one zlhip_sound_tempo_batch-shaped call over (clip[, first_frame[, num_frames[, hop[, bpm_min[, bpm_max]]]]]) tuples (num_frames
    None / missing = to the end of the clip, every other field 0 / missing = its default) -> (status, one dict of zlhip_tempo's fields
    per request)"""
    reqs = (_abi.TempoRequest * max(1, len(requests)))()
    for i, r in enumerate(requests):
        r = tuple(r) if isinstance(r, (tuple, list)) else (r,)
        clip = int(r[0])
        first = int(r[1]) if len(r) > 1 else 0
        n = r[2] if len(r) > 2 else None
        reqs[i] = _abi.TempoRequest(clip, first, int(length_of(clip) - first if n is None else n), int(r[3]) if len(r) > 3 else 0,
                                    float(r[4]) if len(r) > 4 else 0.0, float(r[5]) if len(r) > 5 else 0.0)
    out = (_abi.Tempo * max(1, len(requests)))()
    rc = fn(handle, reqs, len(requests), out)
    return rc, [{k: getattr(out[i], k) for k in TEMPO_FIELDS} for i in range(len(requests))]


def _pcm_sources(sources):
    """(frames, fmt, channels, sample_rate) tuples -> (the C source array, the buffers it points into).  frames: a numpy array
    (uint8, int16, int32, float32, float64) or raw bytes (S24: three bytes per sample), interleaved; fmt: a ZLHIP_PCM_* value or None
    to take it from the array's dtype."""
    by_dtype = {"uint8": _abi.PCM_U8, "int16": _abi.PCM_S16, "int32": _abi.PCM_S32, "float32": _abi.PCM_F32, "float64": _abi.PCM_F64}
    arr = (_abi.PcmSource * max(1, len(sources)))()
    keep = []
    for i, (frames, fmt, channels, sample_rate) in enumerate(sources):
        if isinstance(frames, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(frames), np.uint8)
        else:
            buf = np.ascontiguousarray(frames)
            if buf.dtype.name not in by_dtype:
                raise TypeError(f"PCM frames of dtype {buf.dtype}: expected uint8, int16, int32, float32, float64 or bytes")
            if fmt is None:
                fmt = by_dtype[buf.dtype.name]
        if fmt not in _abi.PCM_BYTES:
            raise ValueError(f"PCM format {fmt}")
        if buf.dtype != np.uint8 and by_dtype[buf.dtype.name] != fmt:
            raise ValueError(f"PCM format {fmt} does not match frames of dtype {buf.dtype}")
        frame_bytes = _abi.PCM_BYTES[fmt] * int(channels)
        if int(channels) < 1 or buf.nbytes % frame_bytes:
            raise ValueError(f"{buf.nbytes} bytes are no whole number of frames of {channels} channels of format {fmt}")
        keep.append(buf)
        arr[i] = _abi.PcmSource(buf.ctypes.data, buf.nbytes // frame_bytes, int(channels), int(fmt), 0, float(sample_rate))
    return arr, keep


@dataclass
class BatchResult:
    bus: np.ndarray            # [num_buses, 2, nblocks*nframes] float32
    reports: np.ndarray        # structured array of VoiceReport


class SamplerSynth:
    def __init__(self, num_buses: int = 12, voices_per_bus: int = 8, *, max_frames: int = 1024,
                 max_batch_blocks: int = 64, max_sounds: int = 1024, mode: int = MODE_FAITHFUL,
                 playback_sample_rate: float = 48000.0, sound_arena_bytes: int = 256 << 20,
                 voices_per_task: int = 0, plan_window_blocks: int = 0, device: int = 0, rt_idle_timeout_us: int = 0,
                 sound_arena_max_bytes: int = 0):
        self._lib = _abi.load()
        cfg = Config()
        self._lib.zlhip_config_default(C.byref(cfg))
        cfg.device = device
        cfg.num_buses = num_buses
        cfg.voices_per_bus = voices_per_bus
        cfg.max_frames = max_frames
        cfg.max_batch_blocks = max_batch_blocks
        cfg.max_sounds = max_sounds
        cfg.mode = mode
        cfg.playback_sample_rate = playback_sample_rate
        cfg.sound_arena_bytes = sound_arena_bytes
        cfg.voices_per_task = voices_per_task
        cfg.plan_window_blocks = plan_window_blocks
        cfg.rt_idle_timeout_us = rt_idle_timeout_us
        cfg.sound_arena_max_bytes = sound_arena_max_bytes
        self.cfg = cfg
        self._e = C.c_void_p()
        rc = self._lib.zlhip_engine_create(C.byref(cfg), C.byref(self._e))
        if rc != 0:
            raise ZlHipError(f"zlhip_engine_create: {self._lib.zlhip_strerror(rc).decode()} ({rc})")
        self.num_buses = num_buses
        self.voices_per_bus = voices_per_bus
        self.num_voices = num_buses * voices_per_bus
        self._last = (0, 0)

    # -- lifecycle --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_e", None) and self._e.value:
            self._lib.zlhip_engine_destroy(self._e)
            self._e = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc, what):
        return _abi.check(self._lib, self._e, rc, what)

    @property
    def handle(self):
        return self._e

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._ck(self._lib.zlhip_device_name(self._e, buf, 256), "device_name")
        return buf.value.decode()

    # -- clips ------------------------------------------------------------------------------
    def register_clip(self, left: np.ndarray, right: Optional[np.ndarray], sample_rate: float) -> int:
        """SamplerSynth::registerClip + SamplerSynthSound::loadSoundData: upload planar fp32."""
        left = np.ascontiguousarray(left, dtype=np.float32)
        rp = None
        if right is not None:
            right = np.ascontiguousarray(right, dtype=np.float32)
            assert right.shape == left.shape
            rp = right.ctypes.data
        out = C.c_int32(-1)
        self._ck(self._lib.zlhip_sound_upload(self._e, left.ctypes.data, rp, left.shape[0], float(sample_rate), C.byref(out)), "sound_upload")
        return out.value

    def register_clip_pcm(self, frames, fmt, channels: int, sample_rate: float) -> int:
        """A clip from interleaved little-endian PCM -- the bytes of a WAV data chunk -- decoded on the device (zlhip_sound_upload_pcm)."""
        return self.register_clips_pcm([(frames, fmt, channels, sample_rate)])[0]

    def register_clips_pcm(self, sources: Sequence[tuple]):
        """[(frames, fmt, channels, sample_rate)] -> clip ids: one call, one wait for the device, all or nothing."""
        arr, keep = _pcm_sources(sources)
        ids = (C.c_int32 * max(1, len(sources)))()
        self._ck(self._lib.zlhip_sound_upload_pcm_batch(self._e, arr, len(sources), ids), "sound_upload_pcm_batch")
        del keep
        return [ids[i] for i in range(len(sources))]

    def upload_pcm_timings(self):
        """(copy_ms, decode_ms) of the last PCM upload made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_upload_pcm_timings(self._e, C.byref(a), C.byref(b)), "debug_upload_pcm_timings")
        return a.value, b.value

    def register_clip_device(self, left_ptr: int, right_ptr: Optional[int], length: int, sample_rate: float) -> int:
        out = C.c_int32(-1)
        self._ck(self._lib.zlhip_sound_upload_device(self._e, left_ptr, right_ptr, length, float(sample_rate), C.byref(out)), "sound_upload_device")
        return out.value

    def register_clip_device_on(self, left_ptr: int, right_ptr: Optional[int], length: int, sample_rate: float, producer_stream: Optional[int]) -> int:
        """register_clip_device with the HIP stream the planes were produced on: the engine waits for that stream (an event), not for the device."""
        out = C.c_int32(-1)
        self._ck(self._lib.zlhip_sound_upload_device_on(self._e, left_ptr, right_ptr, length, float(sample_rate), producer_stream, C.byref(out)), "sound_upload_device_on")
        return out.value

    def unregister_clip(self, clip: int):
        self._ck(self._lib.zlhip_sound_release(self._e, clip), "sound_release")

    def default_clip_params(self, duration_seconds: float) -> ClipParams:
        p = ClipParams()
        self._lib.zlhip_clip_params_default(C.byref(p), float(duration_seconds))
        return p

    def set_clip_params(self, clip: int, params: ClipParams):
        self._ck(self._lib.zlhip_clip_set(self._e, clip, C.byref(params)), "clip_set")

    def rerender_clip(self, clip: int, gain_db: float = 0.0, pitch: float = 0.0, speed: float = 1.0):
        """ClipAudioSource::setGain / setPitch / setSpeedRatio: re-render the clip's playback data on the device from its original
        upload (zlhip_sound_rerender); gain 0, pitch 0, speed 1 plays the original again."""
        p = RerenderParams(float(gain_db), float(pitch), float(speed), 0)
        self._ck(self._lib.zlhip_sound_rerender(self._e, clip, C.byref(p)), "sound_rerender")

    def rerender_clips(self, clips: Sequence[int], gain_db=0.0, pitch=0.0, speed=1.0):
        """Several clips in one call (zlhip_sound_rerender_batch: one seek and one synthesis launch); each parameter is a scalar
        for every clip or a sequence with one value per clip."""
        n = len(clips)
        col = lambda v: [float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else [float(v)] * n
        g, p, s = col(gain_db), col(pitch), col(speed)
        ids = (C.c_int32 * n)(*clips)
        params = (RerenderParams * n)(*[RerenderParams(g[i], p[i], s[i], 0) for i in range(n)])
        self._ck(self._lib.zlhip_sound_rerender_batch(self._e, ids, params, n), "sound_rerender_batch")

    def convert_clips(self, clips: Sequence[int], target_rate: Optional[float] = None):
        """Convert the clips to `target_rate` (None: the engine's playback rate) on the device, band-limited, in one call
        (zlhip_sound_convert_rate_batch): from then on they play as unit-step sources.  Opt-in: a converted clip no longer reproduces
        the reference's bits for its file.  All or nothing; a clip already at the rate is skipped."""
        n = len(clips)
        ids = (C.c_int32 * max(1, n))(*clips)
        self._ck(self._lib.zlhip_sound_convert_rate_batch(self._e, ids, n, float(target_rate or 0.0)), "sound_convert_rate_batch")

    def clip_info(self, clip: int) -> dict:
        """What the clip plays now: length, channels, sample_rate, finite (ZL_SOUND_FINITE), rendered (it plays a re-render)"""
        i = _abi.SoundInfo()
        self._ck(self._lib.zlhip_sound_info_get(self._e, clip, C.byref(i)), "sound_info_get")
        return {"length": i.length, "channels": i.channels, "sample_rate": i.sample_rate, "finite": bool(i.finite), "rendered": bool(i.rendered)}

    def clip_extent(self, clip: int) -> np.ndarray:
        """debug: the clip's playback extent as it lies in the arena, the zero frames behind the last frame included (zlhip_debug_sound_extent)"""
        n = C.c_size_t(0)
        self._ck(self._lib.zlhip_debug_sound_extent(self._e, clip, None, 0, C.byref(n)), "debug_sound_extent")
        out = np.empty(n.value, np.float32)
        self._ck(self._lib.zlhip_debug_sound_extent(self._e, clip, out.ctypes.data, out.size, None), "debug_sound_extent")
        return out

    def convert_timings(self) -> float:
        """device ms of the last conversion call made with profiling on (set_profiling)"""
        a = C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_convert_timings(self._e, C.byref(a)), "debug_convert_timings")
        return a.value

    def read_clip(self, clip: int):
        """The clip's current playback data: (left, right) float32, right None for a mono clip (zlhip_sound_read)."""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_sound_read(self._e, clip, None, None, 0, C.byref(n)), "sound_read")
        L = np.empty(n.value, np.float32); R = np.empty(n.value, np.float32)
        ch = self._ck(self._lib.zlhip_sound_read(self._e, clip, L.ctypes.data, R.ctypes.data, n.value, C.byref(n)), "sound_read")
        return L, (R if ch == 2 else None)

    def clip_length(self, clip: int) -> int:
        """frames of the clip's current playback data"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_sound_read(self._e, clip, None, None, 0, C.byref(n)), "sound_read")
        return n.value

    def clip_overview(self, clip: int, columns: int, first_frame: int = 0, num_frames: Optional[int] = None) -> np.ndarray:
        """The waveform overview of the clip's current playback data (zlhip_sound_overview), computed on the device: float32
        [columns, 4] = (minL, maxL, minR, maxR) per pixel column over the frames [first_frame, first_frame + num_frames) (None: to
        the end); a mono clip repeats its channel.  What a WaveFormItem-shaped painter draws from."""
        return self.clip_overviews([(clip, columns, first_frame, num_frames)])[0]

    def clip_overviews(self, requests: Sequence[tuple]):
        """Several overviews in one call (zlhip_sound_overview_batch: two launches whatever the count).  requests: tuples
        (clip, columns[, first_frame[, num_frames]]); returns one float32 [columns, 4] array per request (views of one packed array)."""
        reqs = _overview_requests(requests, self.clip_length)
        total = sum(max(0, reqs[i].columns) for i in range(len(requests)))
        out = np.empty((total, 4), np.float32)
        self._ck(self._lib.zlhip_sound_overview_batch(self._e, reqs, len(requests), out.ctypes.data, out.size), "sound_overview_batch")
        return _overview_split(out, reqs, len(requests))

    def clip_onsets(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, gate: int = 0, threshold: int = 0,
                    min_gap: int = 0, max_onsets: int = 0) -> np.ndarray:
        """The transients of the clip's current playback data over [first_frame, first_frame + num_frames) (None: to the end), found on
        the device (zlhip_sound_onsets): int32 [count, 2] = (frame, strength) in ascending frame order.  A field
        given as 0 takes its default (zlhip_onset_resolve).  Where a sampler slices a loop."""
        return self.clip_onsets_batch([(clip, first_frame, num_frames, hop, gate, threshold, min_gap, max_onsets)])[0]

    def clip_onsets_batch(self, requests: Sequence[tuple]):
        """Several requests in one call (zlhip_sound_onsets_batch: two launches whatever the count).  requests: tuples
        (clip[, first_frame[, num_frames[, hop[, gate[, threshold[, min_gap[, max_onsets]]]]]]]); one int32 [count, 2] array each."""
        rc, res = _onsets_call(self._lib.zlhip_sound_onsets_batch, self._e, requests, self.clip_length)
        self._ck(rc, "sound_onsets_batch")
        return res

    def onset_hops(self, request: int = 0):
        """debug: (E uint64 [hops], N int32 [hops]) of request `request` of the last onsets call"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_onset_hops(self._e, request, None, None, 0, C.byref(n)), "debug_onset_hops")
        E = np.zeros(n.value, np.uint64); N = np.zeros(n.value, np.int32)
        self._ck(self._lib.zlhip_debug_onset_hops(self._e, request, E.ctypes.data, N.ctypes.data, n.value, C.byref(n)), "debug_onset_hops")
        return E, N

    def onset_timings(self):
        """device ms of the energy pass and of the rest of the last onsets call made with profiling on (set_profiling)"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_onset_timings(self._e, C.byref(a), C.byref(b)), "debug_onset_timings")
        return a.value, b.value

    def clip_tempo(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, bpm_min: float = 0.0, bpm_max: float = 0.0) -> dict:
        """The tempo of the clip's current playback data over [first_frame, first_frame + num_frames) (None: to the end), estimated on
        the device (zlhip_sound_tempo): a dict of zlhip_tempo's fields -- bpm, confidence and the integers they
        derive from.  bpm == 0 means "no tempo" (silence, or too short for the range).  A field given as 0 takes its default
        (zlhip_tempo_resolve: 75 to 150 bpm)."""
        return self.clip_tempo_batch([(clip, first_frame, num_frames, hop, bpm_min, bpm_max)])[0]

    def clip_tempo_batch(self, requests: Sequence[tuple]):
        """Several requests in one call (zlhip_sound_tempo_batch: four launches whatever the count).  requests: tuples
        (clip[, first_frame[, num_frames[, hop[, bpm_min[, bpm_max]]]]]); one dict each."""
        rc, res = _tempo_call(self._lib.zlhip_sound_tempo_batch, self._e, requests, self.clip_length)
        self._ck(rc, "sound_tempo_batch")
        return res

    def tempo_acf(self, request: int = 0):
        """debug: (W uint16 [hops], first_lag, A uint64 [lags] from first_lag on) of request `request` of the last tempo call"""
        n, f, l = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.zlhip_debug_tempo_acf(self._e, request, None, None, 0, C.byref(n), C.byref(f), C.byref(l)), "debug_tempo_acf")
        W = np.zeros(n.value, np.uint16); A = np.zeros(l.value, np.uint64)
        self._ck(self._lib.zlhip_debug_tempo_acf(self._e, request, W.ctypes.data, A.ctypes.data, max(n.value, l.value), C.byref(n), C.byref(f), C.byref(l)), "debug_tempo_acf")
        return W, f.value, A

    def tempo_timings(self):
        """device ms of the energy pass, the autocorrelation kernel and the rest of the last tempo call made with profiling on"""
        a, b, c = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_tempo_timings(self._e, C.byref(a), C.byref(b), C.byref(c)), "debug_tempo_timings")
        return a.value, b.value, c.value

    def clip_pitch(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, window: int = 0, max_frames: int = 0, f_min: float = 0.0,
                   f_max: float = 0.0, threshold: int = 0, gate: int = 0) -> dict:
        """The pitch of the clip's current playback data over [first_frame, first_frame + num_frames) (None: to the end), detected on the
        device (zlhip_sound_pitch): a dict of zlhip_pitch's fields -- hz, note, cents, confidence, root_note and the
        integers they derive from.  hz == 0 means "no pitch" (silence, noise, or shorter than one analysis frame).  A field given as 0
        takes its default (zlhip_pitch_resolve: 55 to 1760 Hz, up to 64 frames).  A note above f_max comes back an octave low."""
        return self.clip_pitch_batch([(clip, first_frame, num_frames, window, max_frames, f_min, f_max, threshold, gate)])[0]

    def clip_pitch_batch(self, requests: Sequence):
        """Several requests in one call (zlhip_sound_pitch_batch: three launches whatever the count).  requests: tuples
        (clip[, first_frame[, num_frames[, window[, max_frames[, f_min[, f_max[, threshold[, gate]]]]]]]]) or dicts; one dict each."""
        rc, res = _pitch_call(self._lib.zlhip_sound_pitch_batch, self._e, requests, self.clip_length)
        self._ck(rc, "sound_pitch_batch")
        return res

    def pitch_frames(self, request: int = 0):
        """debug: the frame records (dicts of zlhip_pitch_frame's fields) of request `request` of the last pitch call"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_pitch_frames(self._e, request, None, 0, C.byref(n)), "debug_pitch_frames")
        recs = (_abi.PitchFrame * max(1, n.value))()
        self._ck(self._lib.zlhip_debug_pitch_frames(self._e, request, C.addressof(recs), n.value, C.byref(n)), "debug_pitch_frames")
        return [{k: getattr(recs[i], k) for k in PITCH_FRAME_FIELDS} for i in range(n.value)]

    def pitch_diff(self, request: int = 0, frame: int = 0):
        """debug: d[1 .. t_max + 1] (uint64) of frame `frame` of request `request` of the last pitch call"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_pitch_diff(self._e, request, frame, None, 0, C.byref(n)), "debug_pitch_diff")
        d = np.zeros(n.value, np.uint64)
        self._ck(self._lib.zlhip_debug_pitch_diff(self._e, request, frame, d.ctypes.data, n.value, C.byref(n)), "debug_pitch_diff")
        return d

    def pitch_timings(self):
        """device ms of the difference-function kernel and of the rest of the last pitch call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_pitch_timings(self._e, C.byref(a), C.byref(b)), "debug_pitch_timings")
        return a.value, b.value

    def clip_loudness(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, sub_frames: int = 0) -> dict:
        """The integrated loudness (ITU-R BS.1770-4 / EBU R 128) and the sample peak of the clip's current playback data over
        [first_frame, first_frame + num_frames) (None: to the end), measured on the device (zlhip_sound_loudness):
        a dict of zlhip_loudness's fields -- lufs, mean_square, relative_gate, peak (a pair), sub_blocks, blocks, above_absolute,
        above_relative.  above_absolute == 0 (lufs == -inf) means "no loudness": silence, or nothing above -70 LUFS."""
        return self.clip_loudness_batch([(clip, first_frame, num_frames, sub_frames)])[0]

    def clip_loudness_batch(self, requests: Sequence):
        """Several requests in one call (zlhip_sound_loudness_batch: one launch whatever the count).  requests: tuples
        (clip[, first_frame[, num_frames[, sub_frames]]]) or dicts; one dict each."""
        rc, res = _loudness_call(self._lib.zlhip_sound_loudness_batch, self._e, requests, self.clip_length)
        self._ck(rc, "sound_loudness_batch")
        return res

    def loudness_subs(self, request: int = 0):
        """debug: the sub-block records of request `request` of the last loudness call -> (sum [n, 2] float64, peak [n, 2] float32)"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_loudness_subs(self._e, request, None, 0, C.byref(n)), "debug_loudness_subs")
        recs = np.zeros(max(1, n.value), np.dtype([("sum", np.float64, 2), ("peak", np.float32, 2)]))
        self._ck(self._lib.zlhip_debug_loudness_subs(self._e, request, recs.ctypes.data, n.value, C.byref(n)), "debug_loudness_subs")
        return recs["sum"][:n.value].copy(), recs["peak"][:n.value].copy()

    def loudness_timings(self) -> float:
        """device ms of the kernel of the last loudness call made with profiling on"""
        a = C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_loudness_timings(self._e, C.byref(a)), "debug_loudness_timings")
        return a.value

    def clip_loop(self, clip: int, start_frame: int, stop_frame: int, start_search: int = 0, stop_search: int = 0, window: int = 0, min_length: int = 0) -> dict:
        """The seamless loop points of the clip's current playback data near the nominal loop [start_frame, stop_frame), searched on the
        device (zlhip_sound_loop): a dict of zlhip_loop's fields -- found, start_frame, stop_frame, seam_db,
        nominal_db, improvement_db and the integers they derive from.  found == 0 means "no admissible pair".  A field given as 0 takes
        its default (zlhip_loop_resolve: 10 ms of search around each point, a window of 256 frames); a search of -1 keeps the point."""
        return self.clip_loop_batch([(clip, start_frame, stop_frame, start_search, stop_search, window, min_length)])[0]

    def clip_loop_batch(self, requests: Sequence):
        """Several requests in one call (zlhip_sound_loop_batch: three launches whatever the count).  requests: tuples
        (clip, start_frame, stop_frame[, start_search[, stop_search[, window[, min_length]]]]) or dicts; one dict each."""
        rc, res = _loop_call(self._lib.zlhip_sound_loop_batch, self._e, requests)
        self._ck(rc, "sound_loop_batch")
        return res

    def loop_items(self, request: int = 0):
        """debug: the work items' records (dicts of zlhip_loop_item's fields) of request `request` of the last loop call"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_loop_items(self._e, request, None, 0, C.byref(n)), "debug_loop_items")
        recs = (_abi.LoopItem * max(1, n.value))()
        self._ck(self._lib.zlhip_debug_loop_items(self._e, request, C.addressof(recs), n.value, C.byref(n)), "debug_loop_items")
        return [{k: getattr(recs[i], k) for k in LOOP_ITEM_FIELDS} for i in range(n.value)]

    def loop_costs(self, request: int = 0):
        """debug: every candidate pair's cost, uint32 [starts, ends], of request `request` of the last loop call; a call with more than
        2^20 candidate pairs keeps none (ZlHipError, ZLHIP_ERR_STATE)"""
        ns, ne = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.zlhip_debug_loop_costs(self._e, request, None, 0, C.byref(ns), C.byref(ne)), "debug_loop_costs")
        d = np.zeros((ns.value, ne.value), np.uint32)
        self._ck(self._lib.zlhip_debug_loop_costs(self._e, request, d.ctypes.data, d.size, C.byref(ns), C.byref(ne)), "debug_loop_costs")
        return d

    def loop_timings(self):
        """device ms of the pairs kernel and of the rest of the last loop call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_loop_timings(self._e, C.byref(a), C.byref(b)), "debug_loop_timings")
        return a.value, b.value

    def clip_loop_crossfade(self, clip: int, start_frame: int, stop_frame: int, fade_frames: int = 0, curve: int = 0) -> dict:
        """Bake a crossfade into the clip's data on the device, so that the loop [start_frame, stop_frame) wraps without a jump
        (zlhip_sound_loop_crossfade): the fade_frames frames in front of stop_frame are faded into the ones in
        front of start_frame.  fade_frames 0: 20 ms, cut to the lead-in and the loop; curve: 0 from the measured correlation, 1 linear,
        2 equal power.  A dict of zlhip_xfade's fields -- applied (0: nothing to fade, the clip is untouched), fade_frames, the three
        integer sums, correlation, rho.  The clip keeps its id; the fade cannot be taken back."""
        return self.clip_loop_crossfade_batch([(clip, start_frame, stop_frame, fade_frames, curve)])[0]

    def clip_loop_crossfade_batch(self, requests: Sequence):
        """Several clips in one call (zlhip_sound_loop_crossfade_batch: three launches and two waits whatever the count; all or nothing).
        requests: tuples (clip, start_frame, stop_frame[, fade_frames[, curve]]) or dicts; one dict each."""
        rc, res = _xfade_call(self._lib.zlhip_sound_loop_crossfade_batch, self._e, requests)
        self._ck(rc, "sound_loop_crossfade_batch")
        return res

    def xfade_timings(self):
        """device ms of the measuring launch and of the render and publishing launches of the last crossfade call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_xfade_timings(self._e, C.byref(a), C.byref(b)), "debug_xfade_timings")
        return a.value, b.value

    def clip_edit(self, clip: int, first_frame: int = 0, num_frames: int = 0, flags: int = 0, pre_roll_frames: int = 0, hold_frames: int = 0,
                  fade_in_frames: int = 0, fade_out_frames: int = 0, curve: int = 0, threshold: float = 0.0) -> dict:
        """Edit the clip's data on the device under its own id (zlhip_sound_edit): keep [first_frame, first_frame +
        num_frames) (num_frames 0: to the end), flags 1 trims the silence off both ends of it (threshold 0: 2^-10; pre_roll_frames and
        hold_frames are kept around the loud part), flags 2 reverses it, then the ends are faded in and out (curve 0 linear, 1 square
        root, 2 smoothstep; each fade cut to half the result).  A dict of zlhip_edit's fields -- applied (0: nothing to change, the clip is
        untouched), silent, the kept region first_frame and num_frames, first_loud, last_loud, the fades as cut, length, reversed, curve.
        There is no undo; the clip's parameters are seconds and stay.  A clip that plays a re-render is refused."""
        return self.clip_edit_batch([dict(clip=clip, first_frame=first_frame, num_frames=num_frames, flags=flags, pre_roll_frames=pre_roll_frames, hold_frames=hold_frames,
                                          fade_in_frames=fade_in_frames, fade_out_frames=fade_out_frames, curve=curve, threshold=threshold)])[0]

    def clip_edit_batch(self, requests: Sequence):
        """Several clips in one call (zlhip_sound_edit_batch: a scan and a wait where a request trims, one render launch whatever the
        count; all or nothing).  requests: dicts with "clip" and any of clip_edit's other arguments"""
        rc, res = _edit_call(self._lib.zlhip_sound_edit_batch, self._e, requests)
        self._ck(rc, "sound_edit_batch")
        return res

    def edit_timings(self):
        """device ms of the scanning launch (0 for a call that trims nothing) and of the render and publishing launches of the last edit call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_edit_timings(self._e, C.byref(a), C.byref(b)), "debug_edit_timings")
        return a.value, b.value

    def clip_peak(self, clip: int, first_frame: int = 0, num_frames: int = 0, flags: int = 0) -> dict:
        """The sample peak and the true peak of the clip's current playback data, measured on the device (zlhip_sound_peak; DESIGN.md
        section 21): a dict of zlhip_peak's fields -- sample_peak and true_peak per channel (linear), oversampling, chunks.  num_frames
        0: to the end.  flags 1 (ZLHIP_LIMIT_TRUE_PEAK) adds the inter-sample peaks (4x below 70 kHz, 2x below 140 kHz)."""
        return self.clip_peak_batch([dict(clip=clip, first_frame=first_frame, num_frames=num_frames, flags=flags)])[0]

    def clip_peak_batch(self, requests: Sequence):
        """Several requests in one call (zlhip_sound_peak_batch: one launch whatever the count).  requests: dicts with "clip" and any of
        clip_peak's other arguments"""
        reqs = []
        for r in requests:
            r = dict(r)
            if int(r.get("num_frames", 0)) == 0:
                r["num_frames"] = self.clip_length(int(r["clip"])) - int(r.get("first_frame", 0))
            reqs.append(r)
        rc, res = _peak_call(self._lib.zlhip_sound_peak_batch, self._e, reqs)
        self._ck(rc, "sound_peak_batch")
        return res

    def peak_chunks(self, request: int = 0):
        """debug: the chunk records of request `request` of the last peak call, float32 [chunks][4]: sample peak L R, inter-sample peak L R"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_peak_chunks(self._e, request, None, 0, C.byref(n)), "debug_peak_chunks")
        recs = np.zeros((max(1, n.value), 4), np.float32)
        self._ck(self._lib.zlhip_debug_peak_chunks(self._e, request, C.cast(recs.ctypes.data, C.POINTER(_abi.PeakChunk)), n.value, C.byref(n)), "debug_peak_chunks")
        return recs[:n.value]

    def clip_limit(self, clip: int, ceiling: float = 0.0, lookahead_frames: int = 0, hold_frames: int = 0, gain: float = 0.0, flags: int = 0) -> dict:
        """Bring the clip's peaks under a ceiling on the device, under its own id (zlhip_sound_limit): a look-ahead
        limiter over the clip's original data, baked.  ceiling 0: -1 dBFS (linear, in (0, 1]); lookahead_frames 0: 5 ms; gain is
        multiplied in first (0: 1); flags 1 detects on the true peak.  A frame out of reach of every peak keeps its bits (times gain).  A
        dict of zlhip_limit's fields -- applied (0: already under the ceiling, the clip is untouched), frames_reduced, peak_before,
        min_gain and the resolved request.  There is no undo.  A clip that plays a re-render, or holds a non-finite sample, is refused."""
        return self.clip_limit_batch([dict(clip=clip, ceiling=ceiling, lookahead_frames=lookahead_frames, hold_frames=hold_frames, gain=gain, flags=flags)])[0]

    def clip_limit_batch(self, requests: Sequence):
        """Several clips in one call (zlhip_sound_limit_batch: a detecting launch, a wait, one render launch whatever the count; all or
        nothing).  requests: dicts with "clip" and any of clip_limit's other arguments"""
        rc, res = _limit_call(self._lib.zlhip_sound_limit_batch, self._e, requests)
        self._ck(rc, "sound_limit_batch")
        return res

    def limit_timings(self):
        """device ms of the detecting launch and of the render and publishing launches of the last limit call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_limit_timings(self._e, C.byref(a), C.byref(b)), "debug_limit_timings")
        return a.value, b.value

    def clip_warp(self, clip: int, anchors) -> dict:
        """Warp the clip's data on the device (zlhip_sound_warp): anchors is a sequence of (src_frame, dst_frame)
        from (0, 0) to (length, new length), strictly increasing; every region between two anchors is stretched by its own ratio and
        starts exactly at its anchor.  A dict of zlhip_warp's fields -- applied (0: the identity, the clip is untouched), regions,
        stretched_regions, segments, length, overlap.  The clip keeps its id; the warp cannot be taken back."""
        return self.clip_warp_batch([(clip, anchors)])[0]

    def clip_warp_batch(self, requests: Sequence):
        """Several clips in one call (zlhip_sound_warp_batch: three launches and one wait whatever the count; all or nothing).
        requests: (clip, anchors) pairs; one dict each."""
        rc, res = _warp_call(self._lib.zlhip_sound_warp_batch, self._e, requests)
        self._ck(rc, "sound_warp_batch")
        return res

    def warp_plan(self, sample_rate: float, length: int, onset_frames, src_bpm: float, dst_bpm: float, steps_per_beat: int = 4, strength: float = 1.0,
                  origin_frame: int = 0, preroll_frames: int = -1):
        """From hits to anchors on the host (zlhip_warp_plan): every onset moved by `strength` towards the nearest step of the grid of
        src_bpm counted from origin_frame, then scaled to dst_bpm.  -> (anchors [n][2] int32, candidates dropped)"""
        on = np.ascontiguousarray(np.asarray(onset_frames, np.int32).reshape(-1))
        out = np.zeros((on.size + 2, 2), np.int32)
        n, dropped = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.zlhip_warp_plan(float(sample_rate), int(length), on.ctypes.data, on.size, float(src_bpm), float(dst_bpm), int(steps_per_beat),
                                           float(strength), int(origin_frame), int(preroll_frames), C.cast(out.ctypes.data, C.POINTER(_abi.WarpAnchor)),
                                           out.shape[0], C.byref(n), C.byref(dropped)), "warp_plan")
        return out[:n.value].copy(), dropped.value

    def warp_offsets(self, clip: int) -> np.ndarray:
        """the seek offsets of the clip's last warp, region by region in output order (zlhip_debug_warp_offsets)"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_warp_offsets(self._e, clip, None, 0, C.byref(n)), "debug_warp_offsets")
        out = np.zeros(max(1, n.value), np.int32)
        self._ck(self._lib.zlhip_debug_warp_offsets(self._e, clip, out.ctypes.data, out.size, C.byref(n)), "debug_warp_offsets")
        return out[:n.value]

    def warp_timings(self):
        """device ms of the seek launch and of the synthesis and publishing launches of the last warp call made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_warp_timings(self._e, C.byref(a), C.byref(b)), "debug_warp_timings")
        return a.value, b.value

    def clip_key(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, max_frames: int = 0, a4_hz: float = 0.0,
                 note_lo: int = 0, note_hi: int = 0, q: int = 0, gate: int = 0) -> dict:
        """The musical key of the clip's current playback data over [first_frame, first_frame + num_frames) (None: to the end), detected on
        the device (zlhip_sound_key): a dict of zlhip_key's fields -- tonic (0 = C .. 11 = B), mode (0 major, 1 minor),
        confidence, the runner-up second_*, frames, sounding and the twelve chroma integers.  tonic == -1 means "no key" (silence, or shorter
        than one analysis frame).  A field given as 0 takes its default (zlhip_key_resolve: a4 = 440, notes 36 .. 95, q = 34, hop 8192)."""
        return self.clip_key_batch([(clip, first_frame, num_frames, hop, max_frames, a4_hz, note_lo, note_hi, q, gate)])[0]

    def clip_key_batch(self, requests: Sequence):
        """Several requests in one call (zlhip_sound_key_batch: three launches whatever the count).  requests: tuples
        (clip[, first_frame[, num_frames[, hop[, max_frames[, a4_hz[, note_lo[, note_hi[, q[, gate]]]]]]]]]) or dicts; one dict each."""
        rc, res = _key_call(self._lib.zlhip_sound_key_batch, self._e, requests, self.clip_length)
        self._ck(rc, "sound_key_batch")
        return res

    def key_bins(self, request: int = 0):
        """debug: the per-bin totals (uint64 [bins]) of request `request` of the last key call"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_key_bins(self._e, request, None, 0, C.byref(n)), "debug_key_bins")
        d = np.zeros(n.value, np.uint64)
        self._ck(self._lib.zlhip_debug_key_bins(self._e, request, d.ctypes.data, n.value, C.byref(n)), "debug_key_bins")
        return d

    def key_frame(self, request: int = 0, frame: int = 0):
        """debug: (re, im), int64 [bins] each, of frame `frame` of request `request` of the last key call (a silent frame's are 0)"""
        n, k = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.zlhip_debug_key_frame(self._e, request, frame, None, None, 0, C.byref(n), C.byref(k)), "debug_key_frame")
        re, im = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
        self._ck(self._lib.zlhip_debug_key_frame(self._e, request, frame, re.ctypes.data, im.ctypes.data, n.value, C.byref(n), C.byref(k)), "debug_key_frame")
        return re, im

    def key_frames(self, request: int = 0) -> int:
        """debug: the analysis frames of request `request` of the last key call"""
        n, k = C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.zlhip_debug_key_frame(self._e, request, 0, None, None, 0, C.byref(n), C.byref(k)), "debug_key_frame")
        return k.value

    def key_timings(self):
        """device ms of the gate, the correlate and the fold launch of the last key call made with profiling on"""
        a, b, c = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_key_timings(self._e, C.byref(a), C.byref(b), C.byref(c)), "debug_key_timings")
        return a.value, b.value, c.value

    def overview_timings(self) -> float:
        """device ms of the last overview call made with profiling on (set_profiling)"""
        a = C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_overview_timings(self._e, C.byref(a)), "debug_overview_timings")
        return a.value

    def rerender_offsets(self, clip: int) -> np.ndarray:
        """debug: the seek offsets of the clip's last render, one per stretch segment (empty: the stretch did not run)"""
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_debug_rerender_offsets(self._e, clip, None, 0, C.byref(n)), "debug_rerender_offsets")
        out = np.zeros(max(n.value, 1), np.int32)
        self._ck(self._lib.zlhip_debug_rerender_offsets(self._e, clip, out.ctypes.data, out.size, C.byref(n)), "debug_rerender_offsets")
        return out[:n.value]

    def rerender_timings(self):
        """(seek ms, synthesis ms) of the last re-render call made with profiling on (set_profiling)"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._ck(self._lib.zlhip_debug_rerender_timings(self._e, C.byref(a), C.byref(b)), "debug_rerender_timings")
        return a.value, b.value

    # -- commands ---------------------------------------------------------------------------
    def handle_clip_command(self, cmd: ClipCommand, current_tick: int = 0) -> int:
        return self._ck(self._lib.zlhip_handle_command(self._e, C.byref(cmd), current_tick), "handle_command")

    def handle_clip_commands(self, cmds: Sequence[ClipCommand], current_tick: int = 0, want_voices: bool = False):
        """A block's worth of commands in one call; returns the per-command results (1 taken / 0 dropped) -- with want_voices also
        the voice (bus * voices_per_bus + slot) each command started, -1 if none."""
        n = len(cmds)
        arr = (ClipCommand * n)(*cmds)
        taken = (C.c_int32 * n)()
        if want_voices:
            voices = (C.c_int32 * n)()
            self._ck(self._lib.zlhip_handle_commands_voices(self._e, arr, n, current_tick, taken, voices), "handle_commands")
            return list(taken), list(voices)
        self._ck(self._lib.zlhip_handle_commands(self._e, arr, n, current_tick, taken), "handle_commands")
        return list(taken)

    def set_bus_enabled(self, bus: int, enabled: bool) -> None:
        """SamplerSynth::setChannelEnabled for bus = channel + 2: a disabled bus takes commands but its voices stand still."""
        self._ck(self._lib.zlhip_bus_set_enabled(self._e, bus, 1 if enabled else 0), "bus_set_enabled")

    def start_voice(self, bus: int, slot: int, cmd: ClipCommand, current_tick: int = 0) -> int:
        return self._ck(self._lib.zlhip_start_voice(self._e, bus, slot, C.byref(cmd), current_tick), "start_voice")

    def stop_voice(self, bus: int, slot: int, allow_tail_off: bool = True) -> int:
        """SamplerSynthVoice::stopNote on one voice slot."""
        return self._ck(self._lib.zlhip_stop_voice(self._e, bus, slot, 1 if allow_tail_off else 0), "stop_voice")

    def update_voice(self, bus: int, slot: int, cmd: ClipCommand) -> int:
        """SamplerSynthVoice::setCurrentCommand on a playing voice."""
        return self._ck(self._lib.zlhip_update_voice(self._e, bus, slot, C.byref(cmd)), "update_voice")

    def voice_is_playing(self, bus: int, slot: int) -> bool:
        return self._ck(self._lib.zlhip_voice_is_playing(self._e, bus, slot), "voice_is_playing") == 1

    # -- render -----------------------------------------------------------------------------
    def process(self, nframes: int, clock: Clock):
        """One real-time cycle of every SamplerChannel; returns (left[B,N], right[B,N])."""
        L = np.empty((self.num_buses, nframes), dtype=np.float32)
        R = np.empty((self.num_buses, nframes), dtype=np.float32)
        self._ck(self._lib.zlhip_render(self._e, nframes, C.byref(clock), L.ctypes.data, R.ctypes.data), "render")
        self._last = (1, nframes)
        return L, R

    def process_into(self, nframes: int, clock: Clock, left: np.ndarray, right: np.ndarray, fan_params: Optional[Sequence[PassthroughParams]] = None,
                     fan: Optional[np.ndarray] = None):
        """One real-time cycle into the caller's arrays ([B, nframes] each, fan [B, 6, nframes]).  Page-locked arrays (pinned_array) are
        written by the kernels directly -- no host copy behind the cycle."""
        if fan is not None:
            arr = (PassthroughParams * self.num_buses)(*fan_params)
            self._ck(self._lib.zlhip_render_fanout(self._e, nframes, C.byref(clock), left.ctypes.data, right.ctypes.data, arr, fan.ctypes.data), "render_fanout")
        else:
            self._ck(self._lib.zlhip_render(self._e, nframes, C.byref(clock), left.ctypes.data, right.ctypes.data), "render")
        self._last = (1, nframes)

    def process_fanout(self, nframes: int, clock: Clock, fan_params: Sequence[PassthroughParams]):
        """One real-time cycle with the JackPassthrough client behind every bus (zlhip_render_fanout): returns
        (left[B,N], right[B,N], fan[B,6,N]) -- fan rows = dryL, dryR, fx1L, fx1R, fx2L, fx2R."""
        L = np.empty((self.num_buses, nframes), dtype=np.float32)
        R = np.empty((self.num_buses, nframes), dtype=np.float32)
        fan = np.empty((self.num_buses, 6, nframes), dtype=np.float32)
        arr = (PassthroughParams * self.num_buses)(*fan_params)
        self._ck(self._lib.zlhip_render_fanout(self._e, nframes, C.byref(clock), L.ctypes.data, R.ctypes.data, arr, fan.ctypes.data), "render_fanout")
        self._last = (1, nframes)
        return L, R, fan

    def render_batch(self, nblocks: int, nframes: int, clocks, bus_out_dev: Optional[int] = None, stream: Optional[int] = None,
                     fan_params: Optional[Sequence[PassthroughParams]] = None, fan_out_dev: Optional[int] = None):
        """fan_params + fan_out_dev: also write the JackPassthrough fan-out [num_buses][6][nblocks*nframes] (fused)."""
        if fan_out_dev is not None:
            arr = (PassthroughParams * self.num_buses)(*fan_params)
            self._ck(self._lib.zlhip_render_batch_fanout(self._e, nblocks, nframes, clocks, bus_out_dev, arr, fan_out_dev, stream), "render_batch_fanout")
        else:
            self._ck(self._lib.zlhip_render_batch(self._e, nblocks, nframes, clocks, bus_out_dev, stream), "render_batch")
        self._last = (nblocks, nframes)

    def synchronize(self):
        self._ck(self._lib.zlhip_synchronize(self._e), "synchronize")

    def bounce(self, nblocks: int, nframes: int, clocks, fmt: str = "f32", sub_blocks: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Offline bounce to HOST memory (zlhip_bounce): "f32" -> float32 [num_buses, 2, nblocks*nframes]; "pcm16" -> int16
        [num_buses, nblocks*nframes, 2], the data chunk of one 16-bit stereo WAV per bus.  Without `out` the result lives in
        page-locked memory owned by the returned array."""
        pcm = {"f32": False, "pcm16": True}[fmt]
        shape = (self.num_buses, nblocks * nframes, 2) if pcm else (self.num_buses, 2, nblocks * nframes)
        dtype = np.int16 if pcm else np.float32
        if out is None:
            out = pinned_array(self._lib, shape, dtype)
        if out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"bounce: out must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
        self._ck(self._lib.zlhip_bounce(self._e, nblocks, nframes, C.cast(clocks, C.c_void_p), out.ctypes.data, 1 if pcm else 0, sub_blocks), "bounce")
        # what read_bus / block_peaks / levels_tick see afterwards: the last chunk (the split of zlhip_bounce)
        sub = min(sub_blocks if sub_blocks > 0 else self.cfg.max_batch_blocks, self.cfg.max_batch_blocks, nblocks)
        self._last = (nblocks - sub * ((nblocks - 1) // sub), nframes)
        return out

    def read_bus(self) -> np.ndarray:
        K, N = self._last
        out = np.empty((self.num_buses, 2, K * N), dtype=np.float32)
        self._ck(self._lib.zlhip_read_bus(self._e, out.ctypes.data, out.size), "read_bus")
        return out

    def voice_reports(self):
        arr = (VoiceReport * self.num_voices)()
        self._ck(self._lib.zlhip_voice_reports(self._e, arr, self.num_voices), "voice_reports")
        return arr

    def enable_trace(self, enable: bool = True, force_slow: bool = False, no_periodic: bool = False):
        self._ck(self._lib.zlhip_debug_enable_trace(self._e, (1 if enable else 0) | (2 if force_slow else 0) | (4 if no_periodic else 0)), "enable_trace")

    def read_trace(self) -> np.ndarray:
        K, N = self._last
        out = np.empty((K, self.num_voices, N), dtype=np.int32)
        self._ck(self._lib.zlhip_debug_read_trace(self._e, out.ctypes.data, out.size), "read_trace")
        return out

    # -- levels -----------------------------------------------------------------------------
    def levels_tick(self, block_index: int = -1, with_hold_bus: int = -1):
        arr = (Levels * self.num_buses)()
        self._ck(self._lib.zlhip_levels_tick(self._e, block_index, with_hold_bus, arr), "levels_tick")
        return arr

    def block_peaks(self) -> np.ndarray:
        K, _ = self._last
        out = np.empty((K, self.num_buses, 2), dtype=np.int32)
        self._ck(self._lib.zlhip_block_peaks(self._e, out.ctypes.data, out.size), "block_peaks")
        return out

    def levels_scan_device(self, bus_dev_ptr: int, nblocks: int, nframes: int, stream: Optional[int] = None):
        self._ck(self._lib.zlhip_levels_scan_device(self._e, bus_dev_ptr, nblocks, nframes, stream), "levels_scan_device")
        self._last = (nblocks, nframes)

    # -- multi-GPU exchange (a bus that spans GPUs) -------------------------------------------
    def bus_reduce_sum_scan(self, pieces_dev_ptr: int, npieces: int, piece_stride_floats: int, units: int, nframes: int,
                            sum_out_dev_ptr: int, levels_out_dev_ptr: int, stream: Optional[int] = None):
        """Sum `npieces` received bus pieces in piece (= rank) order and scan the result for AudioLevels, one kernel."""
        self._ck(self._lib.zlhip_bus_reduce_sum_scan(self._e, pieces_dev_ptr, npieces, piece_stride_floats, units, nframes,
                                                     sum_out_dev_ptr, levels_out_dev_ptr, stream), "bus_reduce_sum_scan")

    def levels_import_units(self, units_dev_ptr: int, nblocks: int, nframes: int, stream: Optional[int] = None):
        """Unit levels of the whole bus ([bus][channel][block]) -> the block levels levels_tick / block_peaks read."""
        self._ck(self._lib.zlhip_levels_import_units(self._e, units_dev_ptr, nblocks, nframes, stream), "levels_import_units")
        self._last = (nblocks, nframes)

    # -- passthrough ------------------------------------------------------------------------
    def passthrough(self, params: Sequence[PassthroughParams], in_dev_ptr: int, out_dev_ptr: int, frames: int, stream: Optional[int] = None):
        arr = (PassthroughParams * self.num_buses)(*params)
        self._ck(self._lib.zlhip_passthrough_process(self._e, arr, in_dev_ptr, out_dev_ptr, frames, stream), "passthrough")

    # -- measurement ------------------------------------------------------------------------
    def set_profiling(self, on: bool = True):
        self._ck(self._lib.zlhip_set_profiling(self._e, 1 if on else 0), "set_profiling")

    def last_timings(self) -> Timings:
        t = Timings()
        self._ck(self._lib.zlhip_last_timings(self._e, C.byref(t)), "last_timings")
        return t

    def profile_totals(self, reset: bool = False):
        """(sums of the timings of the profiled calls since the last reset, number of calls); waits for them."""
        t = Timings()
        n = C.c_int32(0)
        self._ck(self._lib.zlhip_profile_totals(self._e, C.byref(t), C.byref(n), 1 if reset else 0), "profile_totals")
        return t, n.value

    def memory_bytes(self):
        """(HBM bytes the engine allocated at creation, the source arena's share of them)."""
        t, a = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.zlhip_memory_bytes(self._e, C.byref(t), C.byref(a)), "memory_bytes")
        return t.value, a.value

    def rt_stats(self):
        """(launches of the resident real-time kernel, cycles it rendered)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.zlhip_rt_stats(self._e, C.byref(a), C.byref(b)), "rt_stats")
        return a.value, b.value

    def rt_last_cycle(self):
        """Where the last real-time cycle spent its time (engines created with ZL_RT_TRACE=1): an _abi.RtCycleTrace."""
        from ._abi import RtCycleTrace
        t = RtCycleTrace()
        self._ck(self._lib.zlhip_rt_last_cycle(self._e, C.byref(t)), "rt_last_cycle")
        return t

    def rt_residency(self):
        """(is the resident real-time kernel on the device right now, the share of the device's resident capacity it takes)"""
        r, sh = C.c_int32(0), C.c_double(0.0)
        self._ck(self._lib.zlhip_rt_residency(self._e, C.byref(r), C.byref(sh)), "rt_residency")
        return bool(r.value), sh.value

    def bus_device_ptr(self) -> int:
        return self._lib.zlhip_bus_device_ptr(self._e)


class SamplerSynthGroup:
    """One synth over several engines in one process (zlhip_group_*, include/zlhip.h): one member engine per entry of `devices`
    (a device may repeat: [0, 0] is two members on one GPU).  `num_buses` / `voices_per_bus` and the keyword arguments describe the
    WHOLE synth, as for SamplerSynth.  partition: "auto" (bus-aligned when num_buses >= members, else span), "bus" or "span"; root:
    the member that holds the summed bus and the meters in span mode.  Buses, slots, voices and midi channels are global."""

    _PARTITIONS = {"auto": _abi.GROUP_AUTO, "bus": _abi.GROUP_BUS_ALIGNED, "bus_aligned": _abi.GROUP_BUS_ALIGNED, "span": _abi.GROUP_SPAN}

    def __init__(self, devices: Sequence[int], num_buses: int = 12, voices_per_bus: int = 8, *, partition: str = "auto", root: int = 0,
                 max_frames: int = 1024, max_batch_blocks: int = 64, max_sounds: int = 1024, mode: int = MODE_FAITHFUL,
                 playback_sample_rate: float = 48000.0, sound_arena_bytes: int = 256 << 20, voices_per_task: int = 0,
                 plan_window_blocks: int = 0, rt_idle_timeout_us: int = 0, sound_arena_max_bytes: int = 0):
        self._lib = _abi.load()
        cfg = Config()
        self._lib.zlhip_config_default(C.byref(cfg))
        cfg.num_buses = num_buses
        cfg.voices_per_bus = voices_per_bus
        cfg.max_frames = max_frames
        cfg.max_batch_blocks = max_batch_blocks
        cfg.max_sounds = max_sounds
        cfg.mode = mode
        cfg.playback_sample_rate = playback_sample_rate
        cfg.sound_arena_bytes = sound_arena_bytes
        cfg.voices_per_task = voices_per_task
        cfg.plan_window_blocks = plan_window_blocks
        cfg.rt_idle_timeout_us = rt_idle_timeout_us
        cfg.sound_arena_max_bytes = sound_arena_max_bytes
        gc = _abi.GroupConfig()
        self._lib.zlhip_group_config_default(C.byref(gc))
        gc.partition = self._PARTITIONS[partition]
        gc.root = root
        self.cfg, self.gcfg = cfg, gc
        self.devices = list(devices)
        self.n = len(self.devices)
        devs = (C.c_int32 * max(1, self.n))(*self.devices)
        self._g = C.c_void_p()
        rc = self._lib.zlhip_group_create(devs, self.n, C.byref(cfg), C.byref(gc), C.byref(self._g))
        if rc != 0:
            raise ZlHipError(f"zlhip_group_create: {self._lib.zlhip_strerror(rc).decode()} ({rc}) {self._lib.zlhip_group_last_error(None).decode()}")
        self.num_buses = num_buses
        self.voices_per_bus = voices_per_bus
        self.num_voices = num_buses * voices_per_bus
        self._last = (0, 0)

    # -- lifecycle --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._lib.zlhip_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc, what):
        return _abi.check_group(self._lib, self._g, rc, what)

    @property
    def handle(self):
        return self._g

    def layout(self):
        """per member: dict(partition, first_bus, num_buses, first_slot, slots) -- partition "bus" or "span"."""
        arrs = [(C.c_int32 * self.n)() for _ in range(5)]
        self._ck(self._lib.zlhip_group_layout(self._g, *arrs), "group_layout")
        names = {_abi.GROUP_BUS_ALIGNED: "bus", _abi.GROUP_SPAN: "span"}
        return [dict(partition=names[arrs[0][r]], first_bus=arrs[1][r], num_buses=arrs[2][r], first_slot=arrs[3][r], slots=arrs[4][r])
                for r in range(self.n)]

    def member(self, r: int) -> int:
        """the borrowed zlhip_engine * of member r (read-only and measurement calls: zlhip_last_timings, zlhip_memory_bytes ...)"""
        return self._lib.zlhip_group_member(self._g, r)

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        _abi.check(self._lib, C.c_void_p(self.member(0)), self._lib.zlhip_device_name(self.member(0), buf, 256), "device_name")
        return buf.value.decode()

    # -- clips (broadcast to every member) ----------------------------------------------------
    def register_clip(self, left: np.ndarray, right: Optional[np.ndarray], sample_rate: float) -> int:
        left = np.ascontiguousarray(left, dtype=np.float32)
        rp = None
        if right is not None:
            right = np.ascontiguousarray(right, dtype=np.float32)
            assert right.shape == left.shape
            rp = right.ctypes.data
        out = C.c_int32(-1)
        self._ck(self._lib.zlhip_group_sound_upload(self._g, left.ctypes.data, rp, left.shape[0], float(sample_rate), C.byref(out)), "group_sound_upload")
        return out.value

    def register_clip_pcm(self, frames, fmt, channels: int, sample_rate: float) -> int:
        """A clip from interleaved little-endian PCM -- the bytes of a WAV data chunk -- decoded on the device (zlhip_sound_upload_pcm)."""
        return self.register_clips_pcm([(frames, fmt, channels, sample_rate)])[0]

    def register_clips_pcm(self, sources: Sequence[tuple]):
        """[(frames, fmt, channels, sample_rate)] -> clip ids: one call, one wait for the device, all or nothing."""
        arr, keep = _pcm_sources(sources)
        ids = (C.c_int32 * max(1, len(sources)))()
        self._ck(self._lib.zlhip_group_sound_upload_pcm_batch(self._g, arr, len(sources), ids), "group_sound_upload_pcm_batch")
        del keep
        return [ids[i] for i in range(len(sources))]

    def upload_pcm_timings(self):
        """(copy_ms, decode_ms) of the last PCM upload made with profiling on"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        _abi.check(self._lib, C.c_void_p(self.member(0)), self._lib.zlhip_debug_upload_pcm_timings(self.member(0), C.byref(a), C.byref(b)), "debug_upload_pcm_timings")
        return a.value, b.value

    def unregister_clip(self, clip: int):
        self._ck(self._lib.zlhip_group_sound_release(self._g, clip), "group_sound_release")

    def default_clip_params(self, duration_seconds: float) -> ClipParams:
        p = ClipParams()
        self._lib.zlhip_clip_params_default(C.byref(p), float(duration_seconds))
        return p

    def set_clip_params(self, clip: int, params: ClipParams):
        self._ck(self._lib.zlhip_group_clip_set(self._g, clip, C.byref(params)), "group_clip_set")

    def rerender_clips(self, clips: Sequence[int], gain_db=0.0, pitch=0.0, speed=1.0):
        """SamplerSynth.rerender_clips on every member (zlhip_group_sound_rerender_batch)"""
        n = len(clips)
        col = lambda v: [float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else [float(v)] * n
        g, p, s = col(gain_db), col(pitch), col(speed)
        ids = (C.c_int32 * n)(*clips)
        params = (RerenderParams * n)(*[RerenderParams(g[i], p[i], s[i], 0) for i in range(n)])
        self._ck(self._lib.zlhip_group_sound_rerender_batch(self._g, ids, params, n), "group_sound_rerender_batch")

    def rerender_clip(self, clip: int, gain_db: float = 0.0, pitch: float = 0.0, speed: float = 1.0):
        self.rerender_clips([clip], gain_db, pitch, speed)

    def convert_clips(self, clips: Sequence[int], target_rate: Optional[float] = None):
        """SamplerSynth.convert_clips on every member (zlhip_group_sound_convert_rate_batch)"""
        n = len(clips)
        ids = (C.c_int32 * max(1, n))(*clips)
        self._ck(self._lib.zlhip_group_sound_convert_rate_batch(self._g, ids, n, float(target_rate or 0.0)), "group_sound_convert_rate_batch")

    def clip_info(self, clip: int) -> dict:
        """SamplerSynth.clip_info: every member holds every clip, member 0 answers"""
        i = _abi.SoundInfo()
        m0 = C.c_void_p(self.member(0))
        _abi.check(self._lib, m0, self._lib.zlhip_sound_info_get(m0, clip, C.byref(i)), "sound_info_get")
        return {"length": i.length, "channels": i.channels, "sample_rate": i.sample_rate, "finite": bool(i.finite), "rendered": bool(i.rendered)}

    def clip_length(self, clip: int) -> int:
        n = C.c_int32(0)
        m0 = C.c_void_p(self.member(0))
        _abi.check(self._lib, m0, self._lib.zlhip_sound_read(m0, clip, None, None, 0, C.byref(n)), "sound_read")
        return n.value

    def clip_overview(self, clip: int, columns: int, first_frame: int = 0, num_frames: Optional[int] = None) -> np.ndarray:
        """SamplerSynth.clip_overview: every member holds every clip, member 0 answers (zlhip_group_sound_overview_batch)"""
        return self.clip_overviews([(clip, columns, first_frame, num_frames)])[0]

    def clip_overviews(self, requests: Sequence[tuple]):
        reqs = _overview_requests(requests, self.clip_length)
        total = sum(max(0, reqs[i].columns) for i in range(len(requests)))
        out = np.empty((total, 4), np.float32)
        self._ck(self._lib.zlhip_group_sound_overview_batch(self._g, reqs, len(requests), out.ctypes.data, out.size), "group_sound_overview_batch")
        return _overview_split(out, reqs, len(requests))

    def clip_onsets(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, gate: int = 0, threshold: int = 0,
                    min_gap: int = 0, max_onsets: int = 0) -> np.ndarray:
        """SamplerSynth.clip_onsets: every member holds every clip, member 0 answers (zlhip_group_sound_onsets_batch)"""
        return self.clip_onsets_batch([(clip, first_frame, num_frames, hop, gate, threshold, min_gap, max_onsets)])[0]

    def clip_onsets_batch(self, requests: Sequence[tuple]):
        rc, res = _onsets_call(self._lib.zlhip_group_sound_onsets_batch, self._g, requests, self.clip_length)
        self._ck(rc, "group_sound_onsets_batch")
        return res

    def clip_tempo(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, bpm_min: float = 0.0, bpm_max: float = 0.0) -> dict:
        """SamplerSynth.clip_tempo: every member holds every clip, member 0 answers (zlhip_group_sound_tempo_batch)"""
        return self.clip_tempo_batch([(clip, first_frame, num_frames, hop, bpm_min, bpm_max)])[0]

    def clip_tempo_batch(self, requests: Sequence[tuple]):
        rc, res = _tempo_call(self._lib.zlhip_group_sound_tempo_batch, self._g, requests, self.clip_length)
        self._ck(rc, "group_sound_tempo_batch")
        return res

    def clip_pitch(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, window: int = 0, max_frames: int = 0, f_min: float = 0.0,
                   f_max: float = 0.0, threshold: int = 0, gate: int = 0) -> dict:
        """SamplerSynth.clip_pitch: every member holds every clip, member 0 answers (zlhip_group_sound_pitch_batch)"""
        return self.clip_pitch_batch([(clip, first_frame, num_frames, window, max_frames, f_min, f_max, threshold, gate)])[0]

    def clip_pitch_batch(self, requests: Sequence):
        rc, res = _pitch_call(self._lib.zlhip_group_sound_pitch_batch, self._g, requests, self.clip_length)
        self._ck(rc, "group_sound_pitch_batch")
        return res

    def clip_loop(self, clip: int, start_frame: int, stop_frame: int, start_search: int = 0, stop_search: int = 0, window: int = 0, min_length: int = 0) -> dict:
        """SamplerSynth.clip_loop: every member holds every clip, member 0 answers (zlhip_group_sound_loop_batch)"""
        return self.clip_loop_batch([(clip, start_frame, stop_frame, start_search, stop_search, window, min_length)])[0]

    def clip_loop_batch(self, requests: Sequence):
        rc, res = _loop_call(self._lib.zlhip_group_sound_loop_batch, self._g, requests)
        self._ck(rc, "group_sound_loop_batch")
        return res

    def clip_loop_crossfade(self, clip: int, start_frame: int, stop_frame: int, fade_frames: int = 0, curve: int = 0) -> dict:
        """SamplerSynth.clip_loop_crossfade on every member; member 0's results (zlhip_group_sound_loop_crossfade_batch)"""
        return self.clip_loop_crossfade_batch([(clip, start_frame, stop_frame, fade_frames, curve)])[0]

    def clip_loop_crossfade_batch(self, requests: Sequence):
        rc, res = _xfade_call(self._lib.zlhip_group_sound_loop_crossfade_batch, self._g, requests)
        self._ck(rc, "group_sound_loop_crossfade_batch")
        return res

    def clip_edit_batch(self, requests: Sequence):
        """SamplerSynth.clip_edit_batch on every member; member 0's results (zlhip_group_sound_edit_batch)"""
        rc, res = _edit_call(self._lib.zlhip_group_sound_edit_batch, self._g, requests)
        self._ck(rc, "group_sound_edit_batch")
        return res

    def clip_peak_batch(self, requests: Sequence):
        """SamplerSynth.clip_peak_batch; member 0 answers (zlhip_group_sound_peak_batch)"""
        reqs = []
        for r in requests:
            r = dict(r)
            if int(r.get("num_frames", 0)) == 0:
                r["num_frames"] = self.clip_length(int(r["clip"])) - int(r.get("first_frame", 0))
            reqs.append(r)
        rc, res = _peak_call(self._lib.zlhip_group_sound_peak_batch, self._g, reqs)
        self._ck(rc, "group_sound_peak_batch")
        return res

    def clip_limit_batch(self, requests: Sequence):
        """SamplerSynth.clip_limit_batch on every member; member 0's results (zlhip_group_sound_limit_batch)"""
        rc, res = _limit_call(self._lib.zlhip_group_sound_limit_batch, self._g, requests)
        self._ck(rc, "group_sound_limit_batch")
        return res

    def clip_warp(self, clip: int, anchors) -> dict:
        """SamplerSynth.clip_warp on every member; member 0's results (zlhip_group_sound_warp_batch)"""
        return self.clip_warp_batch([(clip, anchors)])[0]

    def clip_warp_batch(self, requests: Sequence):
        rc, res = _warp_call(self._lib.zlhip_group_sound_warp_batch, self._g, requests)
        self._ck(rc, "group_sound_warp_batch")
        return res

    def clip_key(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, hop: int = 0, max_frames: int = 0, a4_hz: float = 0.0,
                 note_lo: int = 0, note_hi: int = 0, q: int = 0, gate: int = 0) -> dict:
        """SamplerSynth.clip_key: every member holds every clip, member 0 answers (zlhip_group_sound_key_batch)"""
        return self.clip_key_batch([(clip, first_frame, num_frames, hop, max_frames, a4_hz, note_lo, note_hi, q, gate)])[0]

    def clip_key_batch(self, requests: Sequence):
        rc, res = _key_call(self._lib.zlhip_group_sound_key_batch, self._g, requests, self.clip_length)
        self._ck(rc, "group_sound_key_batch")
        return res

    def clip_loudness(self, clip: int, first_frame: int = 0, num_frames: Optional[int] = None, sub_frames: int = 0) -> dict:
        """SamplerSynth.clip_loudness: every member holds every clip, member 0 answers (zlhip_group_sound_loudness_batch)"""
        return self.clip_loudness_batch([(clip, first_frame, num_frames, sub_frames)])[0]

    def clip_loudness_batch(self, requests: Sequence):
        rc, res = _loudness_call(self._lib.zlhip_group_sound_loudness_batch, self._g, requests, self.clip_length)
        self._ck(rc, "group_sound_loudness_batch")
        return res

    # -- commands (global buses, slots and midi channels) --------------------------------------
    def handle_clip_commands(self, cmds: Sequence[ClipCommand], current_tick: int = 0, want_voices: bool = False):
        n = len(cmds)
        arr = (ClipCommand * max(1, n))(*cmds)
        taken = (C.c_int32 * max(1, n))()
        voices = (C.c_int32 * max(1, n))()
        self._ck(self._lib.zlhip_group_handle_commands(self._g, arr, n, current_tick, taken, voices), "group_handle_commands")
        return (list(taken)[:n], list(voices)[:n]) if want_voices else list(taken)[:n]

    def handle_clip_command(self, cmd: ClipCommand, current_tick: int = 0) -> int:
        return self.handle_clip_commands([cmd], current_tick)[0]

    def set_bus_enabled(self, bus: int, enabled: bool) -> None:
        self._ck(self._lib.zlhip_group_bus_set_enabled(self._g, bus, 1 if enabled else 0), "group_bus_set_enabled")

    def start_voice(self, bus: int, slot: int, cmd: ClipCommand, current_tick: int = 0) -> int:
        return self._ck(self._lib.zlhip_group_start_voice(self._g, bus, slot, C.byref(cmd), current_tick), "group_start_voice")

    def stop_voice(self, bus: int, slot: int, allow_tail_off: bool = True) -> int:
        return self._ck(self._lib.zlhip_group_stop_voice(self._g, bus, slot, 1 if allow_tail_off else 0), "group_stop_voice")

    def update_voice(self, bus: int, slot: int, cmd: ClipCommand) -> int:
        return self._ck(self._lib.zlhip_group_update_voice(self._g, bus, slot, C.byref(cmd)), "group_update_voice")

    def voice_is_playing(self, bus: int, slot: int) -> bool:
        return self._ck(self._lib.zlhip_group_voice_is_playing(self._g, bus, slot), "group_voice_is_playing") == 1

    # -- render -----------------------------------------------------------------------------
    def render_batch(self, nblocks: int, nframes: int, clocks, bus_out_dev: Optional[int] = None):
        """Asynchronous.  bus_out_dev (span only): a device buffer [num_buses][2][nblocks*nframes] on the root's device."""
        self._ck(self._lib.zlhip_group_render_batch(self._g, nblocks, nframes, clocks, bus_out_dev), "group_render_batch")
        self._last = (nblocks, nframes)

    def synchronize(self):
        self._ck(self._lib.zlhip_group_synchronize(self._g), "group_synchronize")

    def read_bus(self) -> np.ndarray:
        K, N = self._last
        out = np.empty((self.num_buses, 2, K * N), dtype=np.float32)
        self._ck(self._lib.zlhip_group_read_bus(self._g, out.ctypes.data, out.size), "group_read_bus")
        return out

    def voice_reports(self):
        arr = (VoiceReport * self.num_voices)()
        self._ck(self._lib.zlhip_group_voice_reports(self._g, arr, self.num_voices), "group_voice_reports")
        return arr

    # -- levels -----------------------------------------------------------------------------
    def levels_tick(self, block_index: int = -1, with_hold_bus: int = -1):
        arr = (Levels * self.num_buses)()
        self._ck(self._lib.zlhip_group_levels_tick(self._g, block_index, with_hold_bus, arr), "group_levels_tick")
        return arr

    def block_peaks(self) -> np.ndarray:
        K, _ = self._last
        out = np.empty((K, self.num_buses, 2), dtype=np.int32)
        self._ck(self._lib.zlhip_group_block_peaks(self._g, out.ctypes.data, out.size), "group_block_peaks")
        return out
