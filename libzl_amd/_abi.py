"""ctypes mirror of include/zlhip.h and the loader of libzl_amd/lib/libzlhip.so.

The loader fails loudly: there is no CPU render path and no fallback library.  If libzlhip.so is
missing or no HIP device is usable, the error says so.
"""
from __future__ import annotations

import ctypes as C
import os

ZLHIP_OK = 0
ZLHIP_ERR_INVALID = -1
ZLHIP_ERR_NO_DEVICE = -2
ZLHIP_ERR_HIP = -3
ZLHIP_ERR_CAPACITY = -4
ZLHIP_ERR_STATE = -5

MODE_FAITHFUL = 0
MODE_FIX_GAIN = 1
MODE_FIX_DELAY = 2
MODE_HERMITE = 4

MAX_SLICES = 128
BEAT_SUBDIVISIONS = 96


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("num_buses", C.c_int32),
        ("voices_per_bus", C.c_int32), ("max_frames", C.c_int32), ("max_batch_blocks", C.c_int32),
        ("max_sounds", C.c_int32), ("mode", C.c_uint32), ("playback_sample_rate", C.c_double),
        ("sound_arena_bytes", C.c_uint64), ("voices_per_task", C.c_int32), ("plan_window_blocks", C.c_int32),
        ("rt_idle_timeout_us", C.c_int32), ("sound_arena_max_bytes", C.c_uint64),
    ]


class Clock(C.Structure):
    _fields_ = [
        ("current_usecs", C.c_uint64), ("next_usecs", C.c_uint64), ("jack_playhead", C.c_uint64),
        ("jack_playhead_usecs", C.c_uint64), ("jack_subbeat_length_usecs", C.c_uint64),
    ]


class ClipParams(C.Structure):
    _fields_ = [
        ("start_position_seconds", C.c_float), ("length_seconds", C.c_float), ("length_in_beats", C.c_float),
        ("volume_absolute", C.c_float), ("pan", C.c_float), ("duration_seconds", C.c_float),
        ("adsr_attack", C.c_float), ("adsr_decay", C.c_float), ("adsr_sustain", C.c_float), ("adsr_release", C.c_float),
        ("root_note", C.c_int32), ("num_slice_positions", C.c_int32),
        ("slice_positions", C.c_double * MAX_SLICES),
    ]


class ClipCommand(C.Structure):
    _fields_ = [
        ("clip", C.c_int32), ("midi_note", C.c_int32), ("midi_channel", C.c_int32),
        ("start_playback", C.c_int32), ("stop_playback", C.c_int32),
        ("change_slice", C.c_int32), ("slice", C.c_int32),
        ("change_looping", C.c_int32), ("looping", C.c_int32),
        ("change_pitch", C.c_int32), ("pitch_change", C.c_float),
        ("change_speed", C.c_int32), ("speed_ratio", C.c_float),
        ("change_gain_db", C.c_int32), ("gain_db", C.c_float),
        ("change_volume", C.c_int32), ("volume", C.c_float),
    ]


class VoiceReport(C.Structure):
    _fields_ = [
        ("playing", C.c_int32), ("valid", C.c_int32), ("gain", C.c_float), ("progress", C.c_float),
        ("clip", C.c_int32), ("reserved", C.c_int32), ("source_sample_position", C.c_double),
    ]


class Levels(C.Structure):
    _fields_ = [
        ("peak_a", C.c_int32), ("peak_b", C.c_int32),
        ("peak_a_hold_signal", C.c_float), ("peak_b_hold_signal", C.c_float),
        ("peak_db_a", C.c_float), ("peak_db_b", C.c_float), ("combined_db", C.c_float),
        ("hold_db_a", C.c_float), ("hold_db_b", C.c_float), ("rms_a", C.c_float), ("rms_b", C.c_float),
    ]


class PassthroughParams(C.Structure):
    _fields_ = [
        ("dry_amount", C.c_float), ("wet_fx1_amount", C.c_float), ("wet_fx2_amount", C.c_float),
        ("pan_amount", C.c_float), ("muted", C.c_int32),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("plan_ms", C.c_float), ("render_ms", C.c_float), ("finalize_ms", C.c_float), ("total_ms", C.c_float),
        ("source_bytes", C.c_uint64), ("slow_blocks", C.c_uint64), ("active_voice_frames", C.c_uint64),
        ("render_launches", C.c_int32), ("reserved", C.c_int32),
    ]


class RerenderParams(C.Structure):
    _fields_ = [("gain_db", C.c_float), ("pitch_semitones", C.c_float), ("speed_ratio", C.c_float), ("reserved", C.c_int32)]


OVERVIEW_MAX_COLUMNS = 4096


class OverviewRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("columns", C.c_int32)]


ONSET_MAX_ONSETS = 1024


class OnsetRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("hop_frames", C.c_int32), ("gate", C.c_int32),
                ("threshold", C.c_int32), ("min_gap_hops", C.c_int32), ("max_onsets", C.c_int32)]


class Onset(C.Structure):
    _fields_ = [("frame", C.c_int32), ("strength", C.c_int32)]


class TempoRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("hop_frames", C.c_int32), ("bpm_min", C.c_float),
                ("bpm_max", C.c_float)]


class PitchRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("window", C.c_int32), ("max_frames", C.c_int32),
                ("f_min", C.c_float), ("f_max", C.c_float), ("threshold", C.c_int32), ("gate", C.c_int32)]


class Pitch(C.Structure):
    _fields_ = [("hz", C.c_float), ("note", C.c_float), ("cents", C.c_float), ("confidence", C.c_float), ("root_note", C.c_int32),
                ("frames", C.c_int32), ("voiced", C.c_int32), ("consistent", C.c_int32), ("frame", C.c_int32), ("lag", C.c_int32),
                ("shift", C.c_int32), ("clarity", C.c_int32), ("d_lo", C.c_uint64), ("d_mid", C.c_uint64), ("d_hi", C.c_uint64),
                ("cum", C.c_uint64)]


class PitchFrame(C.Structure):
    _fields_ = [("lag", C.c_int32), ("clarity", C.c_int32), ("shift", C.c_int32), ("flag", C.c_int32), ("d_lo", C.c_uint64),
                ("d_mid", C.c_uint64), ("d_hi", C.c_uint64), ("cum", C.c_uint64)]


class LoudnessRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("sub_frames", C.c_int32)]


class Loudness(C.Structure):
    _fields_ = [("lufs", C.c_double), ("mean_square", C.c_double), ("relative_gate", C.c_double), ("peak", C.c_float * 2),
                ("sub_blocks", C.c_int32), ("blocks", C.c_int32), ("above_absolute", C.c_int32), ("above_relative", C.c_int32)]


class LoudnessSub(C.Structure):
    _fields_ = [("sum", C.c_double * 2), ("peak", C.c_float * 2)]


class LoopRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("start_frame", C.c_int32), ("stop_frame", C.c_int32), ("start_search", C.c_int32), ("stop_search", C.c_int32),
                ("window", C.c_int32), ("min_length", C.c_int32)]


class Loop(C.Structure):
    _fields_ = [("found", C.c_int32), ("start_frame", C.c_int32), ("stop_frame", C.c_int32), ("shift", C.c_int32), ("starts", C.c_int32),
                ("ends", C.c_int32), ("nominal_valid", C.c_int32), ("reserved", C.c_int32), ("pairs", C.c_uint64), ("cost", C.c_uint32),
                ("den", C.c_uint32), ("nominal_cost", C.c_uint32), ("nominal_den", C.c_uint32), ("seam_db", C.c_double), ("nominal_db", C.c_double),
                ("improvement_db", C.c_double)]


class LoopItem(C.Structure):
    _fields_ = [("start", C.c_int32), ("stop", C.c_int32), ("cost", C.c_uint32), ("den", C.c_uint32), ("pairs", C.c_uint64)]


class XfadeRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("start_frame", C.c_int32), ("stop_frame", C.c_int32), ("fade_frames", C.c_int32), ("curve", C.c_int32)]


class Xfade(C.Structure):
    _fields_ = [("applied", C.c_int32), ("fade_frames", C.c_int32), ("start_frame", C.c_int32), ("stop_frame", C.c_int32), ("curve", C.c_int32),
                ("reserved", C.c_int32), ("sab", C.c_int64), ("saa", C.c_int64), ("sbb", C.c_int64), ("correlation", C.c_double), ("rho", C.c_double)]


XFADE_AUTO, XFADE_LINEAR, XFADE_EQUAL_POWER = 0, 1, 2


class EditRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("flags", C.c_int32), ("pre_roll_frames", C.c_int32),
                ("hold_frames", C.c_int32), ("fade_in_frames", C.c_int32), ("fade_out_frames", C.c_int32), ("curve", C.c_int32), ("threshold", C.c_float)]


class Edit(C.Structure):
    _fields_ = [("applied", C.c_int32), ("silent", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("first_loud", C.c_int32),
                ("last_loud", C.c_int32), ("fade_in_frames", C.c_int32), ("fade_out_frames", C.c_int32), ("length", C.c_int32), ("reversed", C.c_int32),
                ("curve", C.c_int32), ("reserved", C.c_int32)]


EDIT_TRIM, EDIT_REVERSE = 1, 2
EDIT_LINEAR, EDIT_SQRT, EDIT_SMOOTH = 0, 1, 2
# the sizes the library asserts for the edit's two records (zl_clip_calls.cpp)
STRUCT_SIZES = {"zlhip_edit_request": (EditRequest, 40), "zlhip_edit": (Edit, 48)}


class PeakRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("flags", C.c_int32)]


class Peak(C.Structure):
    _fields_ = [("sample_peak", C.c_float * 2), ("true_peak", C.c_float * 2), ("oversampling", C.c_int32), ("chunks", C.c_int32)]


class PeakChunk(C.Structure):
    _fields_ = [("sample_peak", C.c_float * 2), ("inter_peak", C.c_float * 2)]


class LimitRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("flags", C.c_int32), ("lookahead_frames", C.c_int32), ("hold_frames", C.c_int32), ("ceiling", C.c_float), ("gain", C.c_float)]


class Limit(C.Structure):
    _fields_ = [("applied", C.c_int32), ("lookahead_frames", C.c_int32), ("hold_frames", C.c_int32), ("oversampling", C.c_int32), ("frames_reduced", C.c_int32),
                ("peak_before", C.c_float), ("min_gain", C.c_float), ("ceiling", C.c_float), ("gain", C.c_float), ("reserved", C.c_int32)]


LIMIT_TRUE_PEAK = 1


class WarpAnchor(C.Structure):
    _fields_ = [("src_frame", C.c_int32), ("dst_frame", C.c_int32)]


class WarpRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("count", C.c_int32), ("anchors", C.POINTER(WarpAnchor))]


class Warp(C.Structure):
    _fields_ = [("applied", C.c_int32), ("regions", C.c_int32), ("stretched_regions", C.c_int32), ("segments", C.c_int32), ("length", C.c_int32),
                ("overlap", C.c_int32)]


WARP_MAX_ANCHORS = 4096


class KeyRequest(C.Structure):
    _fields_ = [("id", C.c_int32), ("first_frame", C.c_int32), ("num_frames", C.c_int32), ("hop", C.c_int32), ("max_frames", C.c_int32),
                ("a4_hz", C.c_float), ("note_lo", C.c_int32), ("note_hi", C.c_int32), ("q", C.c_int32), ("gate", C.c_int32)]


class Key(C.Structure):
    _fields_ = [("tonic", C.c_int32), ("mode", C.c_int32), ("second_tonic", C.c_int32), ("second_mode", C.c_int32), ("frames", C.c_int32),
                ("sounding", C.c_int32), ("confidence", C.c_double), ("second_confidence", C.c_double), ("chroma", C.c_uint64 * 12)]


class KeyBin(C.Structure):
    _fields_ = [("note", C.c_int32), ("n", C.c_int32), ("step", C.c_uint32), ("wstep", C.c_uint32)]


class Tempo(C.Structure):
    _fields_ = [("bpm", C.c_float), ("confidence", C.c_float), ("lag_coarse", C.c_int32), ("lag_fine", C.c_int32), ("doublings", C.c_int32),
                ("shift", C.c_int32), ("hops", C.c_int32), ("reserved", C.c_int32), ("acf_lo", C.c_uint64), ("acf_mid", C.c_uint64),
                ("acf_hi", C.c_uint64), ("acf_zero", C.c_uint64), ("sum", C.c_uint64)]


PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = 1, 2, 3, 4, 5, 6
PCM_MAX_CHANNELS = 64
PCM_BYTES = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4, PCM_F64: 8}


class PcmSource(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("length", C.c_int32), ("channels", C.c_int32), ("format", C.c_int32), ("reserved", C.c_int32),
                ("sample_rate", C.c_double)]


class SoundInfo(C.Structure):
    _fields_ = [("length", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_double), ("finite", C.c_int32), ("rendered", C.c_int32)]


class RtCycleTrace(C.Structure):
    _fields_ = [
        ("cycle", C.c_uint64), ("resident", C.c_int32), ("reserved", C.c_int32),
        ("total_us", C.c_double), ("before_post_us", C.c_double), ("wait_us", C.c_double), ("after_us", C.c_double),
        ("max_poll_gap_us", C.c_double), ("device_us", C.c_double), ("involuntary_switches", C.c_int64),
    ]


GROUP_MAX_MEMBERS = 8
GROUP_AUTO, GROUP_BUS_ALIGNED, GROUP_SPAN = 0, 1, 2


class GroupConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("partition", C.c_int32), ("root", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/zlhip.h declares: name -> (restype, argtypes)
_F = C.POINTER(C.c_float)
_E = C.c_void_p
SIGNATURES = {
    "zlhip_abi_version": (C.c_int, []),
    "zlhip_config_default": (None, [C.POINTER(Config)]),
    "zlhip_engine_create": (C.c_int, [C.POINTER(Config), C.POINTER(_E)]),
    "zlhip_engine_destroy": (None, [_E]),
    "zlhip_last_error": (C.c_char_p, [_E]),
    "zlhip_strerror": (C.c_char_p, [C.c_int]),
    "zlhip_sound_upload": (C.c_int, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_int32)]),
    "zlhip_sound_upload_device": (C.c_int, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_int32)]),
    "zlhip_sound_upload_device_on": (C.c_int, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.POINTER(C.c_int32)]),
    "zlhip_sound_release": (C.c_int, [_E, C.c_int32]),
    "zlhip_clip_params_default": (None, [C.POINTER(ClipParams), C.c_float]),
    "zlhip_clip_set": (C.c_int, [_E, C.c_int32, C.POINTER(ClipParams)]),
    "zlhip_sound_rerender": (C.c_int, [_E, C.c_int32, C.POINTER(RerenderParams)]),
    "zlhip_sound_rerender_batch": (C.c_int, [_E, C.POINTER(C.c_int32), C.POINTER(RerenderParams), C.c_int32]),
    "zlhip_sound_read": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_sound_overview": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "zlhip_sound_overview_batch": (C.c_int, [_E, C.POINTER(OverviewRequest), C.c_int32, C.c_void_p, C.c_size_t]),
    "zlhip_debug_overview_timings": (C.c_int, [_E, C.POINTER(C.c_float)]),
    "zlhip_onset_resolve": (C.c_int, [C.c_double, C.POINTER(OnsetRequest)]),
    "zlhip_sound_onsets": (C.c_int, [_E, C.POINTER(OnsetRequest), C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_sound_onsets_batch": (C.c_int, [_E, C.POINTER(OnsetRequest), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "zlhip_debug_onset_hops": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_onset_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_tempo_resolve": (C.c_int, [C.c_double, C.POINTER(TempoRequest)]),
    "zlhip_sound_tempo": (C.c_int, [_E, C.POINTER(TempoRequest), C.POINTER(Tempo)]),
    "zlhip_sound_tempo_batch": (C.c_int, [_E, C.POINTER(TempoRequest), C.c_int32, C.POINTER(Tempo)]),
    "zlhip_debug_tempo_acf": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_debug_tempo_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_pitch_resolve": (C.c_int, [C.c_double, C.POINTER(PitchRequest)]),
    "zlhip_sound_pitch": (C.c_int, [_E, C.POINTER(PitchRequest), C.POINTER(Pitch)]),
    "zlhip_sound_pitch_batch": (C.c_int, [_E, C.POINTER(PitchRequest), C.c_int32, C.POINTER(Pitch)]),
    "zlhip_debug_pitch_frames": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_pitch_diff": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_pitch_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_loudness_resolve": (C.c_int, [C.c_double, C.POINTER(LoudnessRequest)]),
    "zlhip_loudness_design": (C.c_int, [C.c_double, C.POINTER(C.c_double)]),
    "zlhip_sound_loudness": (C.c_int, [_E, C.POINTER(LoudnessRequest), C.POINTER(Loudness)]),
    "zlhip_sound_loudness_batch": (C.c_int, [_E, C.POINTER(LoudnessRequest), C.c_int32, C.POINTER(Loudness)]),
    "zlhip_debug_loudness_subs": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_loudness_timings": (C.c_int, [_E, C.POINTER(C.c_float)]),
    "zlhip_loop_resolve": (C.c_int, [C.c_double, C.POINTER(LoopRequest)]),
    "zlhip_loop_seconds": (C.c_int, [C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_sound_loop": (C.c_int, [_E, C.POINTER(LoopRequest), C.POINTER(Loop)]),
    "zlhip_sound_loop_batch": (C.c_int, [_E, C.POINTER(LoopRequest), C.c_int32, C.POINTER(Loop)]),
    "zlhip_debug_loop_items": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_loop_costs": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_debug_loop_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_xfade_resolve": (C.c_int, [C.c_double, C.c_int32, C.POINTER(XfadeRequest)]),
    "zlhip_xfade_design": (C.c_int, [C.c_int32, C.c_double, C.c_void_p]),
    "zlhip_sound_loop_crossfade": (C.c_int, [_E, C.POINTER(XfadeRequest), C.POINTER(Xfade)]),
    "zlhip_sound_loop_crossfade_batch": (C.c_int, [_E, C.POINTER(XfadeRequest), C.c_int32, C.POINTER(Xfade)]),
    "zlhip_debug_xfade_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_edit_resolve": (C.c_int, [C.c_int32, C.POINTER(EditRequest)]),
    "zlhip_edit_design": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "zlhip_sound_edit": (C.c_int, [_E, C.POINTER(EditRequest), C.POINTER(Edit)]),
    "zlhip_sound_edit_batch": (C.c_int, [_E, C.POINTER(EditRequest), C.c_int32, C.POINTER(Edit)]),
    "zlhip_debug_edit_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_peak_resolve": (C.c_int, [C.c_double, C.c_int32, C.POINTER(PeakRequest)]),
    "zlhip_sound_peak": (C.c_int, [_E, C.POINTER(PeakRequest), C.POINTER(Peak)]),
    "zlhip_sound_peak_batch": (C.c_int, [_E, C.POINTER(PeakRequest), C.c_int32, C.POINTER(Peak)]),
    "zlhip_debug_peak_chunks": (C.c_int, [_E, C.c_int32, C.POINTER(PeakChunk), C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_limit_resolve": (C.c_int, [C.c_double, C.POINTER(LimitRequest)]),
    "zlhip_limit_design": (C.c_int, [C.c_int32, C.c_void_p]),
    "zlhip_sound_limit": (C.c_int, [_E, C.POINTER(LimitRequest), C.POINTER(Limit)]),
    "zlhip_sound_limit_batch": (C.c_int, [_E, C.POINTER(LimitRequest), C.c_int32, C.POINTER(Limit)]),
    "zlhip_debug_limit_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_warp_resolve": (C.c_int, [C.c_double, C.c_int32, C.POINTER(WarpAnchor), C.c_int32, C.POINTER(Warp)]),
    "zlhip_warp_plan": (C.c_int, [C.c_double, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                  C.POINTER(WarpAnchor), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_warp_map": (C.c_int64, [C.POINTER(WarpAnchor), C.c_int32, C.c_int64]),
    "zlhip_sound_warp": (C.c_int, [_E, C.POINTER(WarpRequest), C.POINTER(Warp)]),
    "zlhip_sound_warp_batch": (C.c_int, [_E, C.POINTER(WarpRequest), C.c_int32, C.POINTER(Warp)]),
    "zlhip_debug_warp_offsets": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_warp_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_key_resolve": (C.c_int, [C.c_double, C.POINTER(KeyRequest)]),
    "zlhip_key_design": (C.c_int, [C.c_double, C.POINTER(KeyRequest), C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]),
    "zlhip_key_match_shift": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "zlhip_sound_key": (C.c_int, [_E, C.POINTER(KeyRequest), C.POINTER(Key)]),
    "zlhip_sound_key_batch": (C.c_int, [_E, C.POINTER(KeyRequest), C.c_int32, C.POINTER(Key)]),
    "zlhip_debug_key_bins": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_key_frame": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_debug_key_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_sound_upload_pcm": (C.c_int, [_E, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_int32)]),
    "zlhip_sound_upload_pcm_batch": (C.c_int, [_E, C.POINTER(PcmSource), C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_upload_pcm_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_debug_rerender_offsets": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_debug_rerender_timings": (C.c_int, [_E, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "zlhip_sound_convert_rate": (C.c_int, [_E, C.c_int32, C.c_double]),
    "zlhip_sound_convert_rate_batch": (C.c_int, [_E, C.POINTER(C.c_int32), C.c_int32, C.c_double]),
    "zlhip_resample_design": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_size_t]),
    "zlhip_sound_info_get": (C.c_int, [_E, C.c_int32, C.POINTER(SoundInfo)]),
    "zlhip_debug_convert_timings": (C.c_int, [_E, C.POINTER(C.c_float)]),
    "zlhip_debug_sound_extent": (C.c_int, [_E, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "zlhip_clip_command_clear": (None, [C.POINTER(ClipCommand)]),
    "zlhip_handle_command": (C.c_int, [_E, C.POINTER(ClipCommand), C.c_uint64]),
    "zlhip_handle_commands": (C.c_int, [_E, C.POINTER(ClipCommand), C.c_int32, C.c_uint64, C.POINTER(C.c_int32)]),
    "zlhip_handle_commands_voices": (C.c_int, [_E, C.POINTER(ClipCommand), C.c_int32, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_bus_set_enabled": (C.c_int, [_E, C.c_int32, C.c_int]),
    "zlhip_start_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(ClipCommand), C.c_uint64]),
    "zlhip_stop_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_int]),
    "zlhip_update_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(ClipCommand)]),
    "zlhip_voice_is_playing": (C.c_int, [_E, C.c_int32, C.c_int32]),
    "zlhip_render": (C.c_int, [_E, C.c_int32, C.POINTER(Clock), C.c_void_p, C.c_void_p]),
    "zlhip_render_fanout": (C.c_int, [_E, C.c_int32, C.POINTER(Clock), C.c_void_p, C.c_void_p, C.POINTER(PassthroughParams), C.c_void_p]),
    "zlhip_render_batch": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(Clock), C.c_void_p, C.c_void_p]),
    "zlhip_render_batch_fanout": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(Clock), C.c_void_p, C.POINTER(PassthroughParams), C.c_void_p, C.c_void_p]),
    "zlhip_synchronize": (C.c_int, [_E]),
    "zlhip_read_bus": (C.c_int, [_E, C.c_void_p, C.c_size_t]),
    "zlhip_voice_reports": (C.c_int, [_E, C.POINTER(VoiceReport), C.c_int32]),
    "zlhip_debug_enable_trace": (C.c_int, [_E, C.c_int]),
    "zlhip_debug_read_trace": (C.c_int, [_E, C.c_void_p, C.c_size_t]),
    "zlhip_debug_live_resources": (C.c_int, [C.POINTER(C.c_int32)]),
    "zlhip_levels_tick": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(Levels)]),
    "zlhip_block_peaks": (C.c_int, [_E, C.c_void_p, C.c_size_t]),
    "zlhip_levels_scan_device": (C.c_int, [_E, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "zlhip_memory_bytes": (C.c_int, [_E, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zlhip_bounce": (C.c_int, [_E, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "zlhip_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "zlhip_host_free": (None, [C.c_void_p]),
    "zlhip_bus_reduce_sum_scan": (C.c_int, [_E, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "zlhip_levels_import_units": (C.c_int, [_E, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "zlhip_passthrough_params_default": (None, [C.POINTER(PassthroughParams)]),
    "zlhip_passthrough_process": (C.c_int, [_E, C.POINTER(PassthroughParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "zlhip_set_profiling": (C.c_int, [_E, C.c_int]),
    "zlhip_last_timings": (C.c_int, [_E, C.POINTER(Timings)]),
    "zlhip_profile_totals": (C.c_int, [_E, C.POINTER(Timings), C.POINTER(C.c_int32), C.c_int]),
    "zlhip_bus_device_ptr": (C.c_void_p, [_E]),
    "zlhip_device_name": (C.c_int, [_E, C.c_char_p, C.c_size_t]),
    "zlhip_rt_stats": (C.c_int, [_E, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "zlhip_rt_residency": (C.c_int, [_E, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "zlhip_rt_last_cycle": (C.c_int, [_E, C.POINTER(RtCycleTrace)]),
    # engine group (one synth over several engines / devices in one process)
    "zlhip_group_config_default": (None, [C.POINTER(GroupConfig)]),
    "zlhip_group_create": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(Config), C.POINTER(GroupConfig), C.POINTER(_E)]),
    "zlhip_group_destroy": (None, [_E]),
    "zlhip_group_last_error": (C.c_char_p, [_E]),
    "zlhip_group_layout": (C.c_int, [_E, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_group_member": (C.c_void_p, [_E, C.c_int32]),
    "zlhip_group_sound_upload": (C.c_int, [_E, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_int32)]),
    "zlhip_group_sound_upload_pcm_batch": (C.c_int, [_E, C.POINTER(PcmSource), C.c_int32, C.POINTER(C.c_int32)]),
    "zlhip_group_sound_release": (C.c_int, [_E, C.c_int32]),
    "zlhip_group_clip_set": (C.c_int, [_E, C.c_int32, C.POINTER(ClipParams)]),
    "zlhip_group_sound_rerender_batch": (C.c_int, [_E, C.POINTER(C.c_int32), C.POINTER(RerenderParams), C.c_int32]),
    "zlhip_group_sound_convert_rate_batch": (C.c_int, [_E, C.POINTER(C.c_int32), C.c_int32, C.c_double]),
    "zlhip_group_sound_overview": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "zlhip_group_sound_overview_batch": (C.c_int, [_E, C.POINTER(OverviewRequest), C.c_int32, C.c_void_p, C.c_size_t]),
    "zlhip_group_sound_onsets_batch": (C.c_int, [_E, C.POINTER(OnsetRequest), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "zlhip_group_sound_tempo_batch": (C.c_int, [_E, C.POINTER(TempoRequest), C.c_int32, C.POINTER(Tempo)]),
    "zlhip_group_sound_pitch_batch": (C.c_int, [_E, C.POINTER(PitchRequest), C.c_int32, C.POINTER(Pitch)]),
    "zlhip_group_sound_loop_batch": (C.c_int, [_E, C.POINTER(LoopRequest), C.c_int32, C.POINTER(Loop)]),
    "zlhip_group_sound_loop_crossfade_batch": (C.c_int, [_E, C.POINTER(XfadeRequest), C.c_int32, C.POINTER(Xfade)]),
    "zlhip_group_sound_edit_batch": (C.c_int, [_E, C.POINTER(EditRequest), C.c_int32, C.POINTER(Edit)]),
    "zlhip_group_sound_peak_batch": (C.c_int, [_E, C.POINTER(PeakRequest), C.c_int32, C.POINTER(Peak)]),
    "zlhip_group_sound_limit_batch": (C.c_int, [_E, C.POINTER(LimitRequest), C.c_int32, C.POINTER(Limit)]),
    "zlhip_group_sound_warp_batch": (C.c_int, [_E, C.POINTER(WarpRequest), C.c_int32, C.POINTER(Warp)]),
    "zlhip_group_sound_key_batch": (C.c_int, [_E, C.POINTER(KeyRequest), C.c_int32, C.POINTER(Key)]),
    "zlhip_group_sound_loudness_batch": (C.c_int, [_E, C.POINTER(LoudnessRequest), C.c_int32, C.POINTER(Loudness)]),
    "zlhip_group_handle_commands": (C.c_int, [_E, C.POINTER(ClipCommand), C.c_int32, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "zlhip_group_start_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(ClipCommand), C.c_uint64]),
    "zlhip_group_stop_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.c_int]),
    "zlhip_group_update_voice": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(ClipCommand)]),
    "zlhip_group_voice_is_playing": (C.c_int, [_E, C.c_int32, C.c_int32]),
    "zlhip_group_bus_set_enabled": (C.c_int, [_E, C.c_int32, C.c_int]),
    "zlhip_group_render_batch": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(Clock), C.c_void_p]),
    "zlhip_group_synchronize": (C.c_int, [_E]),
    "zlhip_group_read_bus": (C.c_int, [_E, C.c_void_p, C.c_size_t]),
    "zlhip_group_voice_reports": (C.c_int, [_E, C.POINTER(VoiceReport), C.c_int32]),
    "zlhip_group_levels_tick": (C.c_int, [_E, C.c_int32, C.c_int32, C.POINTER(Levels)]),
    "zlhip_group_block_peaks": (C.c_int, [_E, C.c_void_p, C.c_size_t]),
}

# ZLHIP_LIBRARY selects another build of the same library (A/B measurements of kernel variants); never a fallback
LIB_PATH = os.environ.get("ZLHIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libzlhip.so")
_lib = None


def bind(lib, signatures=SIGNATURES):
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libzlhip.so (built in-tree by libzl_amd/build.py).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m libzl_amd.build` "
                "(hipcc --offload-arch=gfx950).  libzl_amd has no CPU fallback.")
        _lib = bind(C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL))
    return _lib


class UnitLevels(C.Structure):
    _fields_ = [("peak", C.c_int32), ("sumsq", C.c_float)]


class ZlHipError(RuntimeError):
    pass


def check_group(lib, group, rc, what):
    if rc < 0:
        raise ZlHipError(f"{what}: {lib.zlhip_strerror(rc).decode()} ({rc}) {lib.zlhip_group_last_error(group).decode()}")
    return rc


def check(lib, engine, rc, what):
    if rc < 0:
        detail = lib.zlhip_last_error(engine).decode() if engine else ""
        raise ZlHipError(f"{what}: {lib.zlhip_strerror(rc).decode()} ({rc}) {detail}")
    return rc
