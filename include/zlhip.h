/*
 * zlhip.h -- C-ABI of the MI355X sampler engine that replaces libzl's audio hot path.
 *
 * Drop-in seam (reference, paths under /root/reference/lib):
 *   SamplerChannel::process            SamplerSynth.cpp:116-148   -> zlhip_render / zlhip_render_batch
 *   SamplerChannel::handleCommand      SamplerSynth.cpp:187-230   -> zlhip_handle_command
 *   SamplerSynth::registerClip / SamplerSynthSound::loadSoundData
 *                                      SamplerSynth.cpp:285-295, SamplerSynthSound.cpp:28-59 -> zlhip_sound_upload
 *   ClipAudioSource getters read per block by the voice
 *                                      SamplerSynthVoice.cpp:189-196, ClipAudioSource.cpp:261-277,338-346,362,619,692
 *                                                                 -> zlhip_clip_set
 *   SamplerSynthVoice::process         SamplerSynthVoice.cpp:174-270 -> HIP kernels behind zlhip_render*
 *   positions-model report             SamplerSynthVoice.cpp:265-267 -> zlhip_voice_reports
 *   AudioLevels::timerCallback         AudioLevels.cpp:347-412    -> zlhip_levels_tick
 *   JackPassthroughPrivate::process    JackPassthrough.cpp:45-115 -> zlhip_passthrough_*
 *
 * Plain C: opaque handle, POD structs, raw pointers and sizes, int status codes.  No torch / Qt /
 * JUCE types.  All functions are thread-compatible (one caller at a time per engine), mirroring
 * the reference where each SamplerChannel is driven by one JACK thread.
 * The library has NO CPU render path: if no HIP device is usable, zlhip_engine_create fails with
 * ZLHIP_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef ZLHIP_H
#define ZLHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: zlhip_config grew (rt_idle_timeout_us; struct_size tells the library which fields the caller knows); ZLHIP_MODE_HERMITE is
 *    the tap-weight form fixed in round 2 (it differs from the Horner form of ABI 1 in the last bits);
 *    new entry points: zlhip_bounce, zlhip_host_alloc/free, zlhip_bus_reduce_sum_scan, zlhip_levels_import_units,
 *    zlhip_sound_upload_device_on; zlhip_clip_set no longer waits for the device (the edit lands at the next render call).
 * 3: new entry points only (a caller built against 2 keeps working): zlhip_render_fanout (the JackPassthrough fan-out on the
 *    real-time cycle), zlhip_rt_residency, zlhip_rt_last_cycle; the resident real-time kernel takes any period (blocks longer than 256 frames too).
 *    Later additions, still 3 (new entry points only): the engine group (zlhip_group_*), zlhip_sound_overview / _batch (waveform overviews),
 *    zlhip_sound_upload_pcm / _batch (clips from raw PCM, decoded on the device), zlhip_sound_convert_rate / _batch (clips converted to
 *    another sample rate on the device, band-limited), zlhip_resample_design, zlhip_sound_info_get, zlhip_debug_sound_extent, zlhip_sound_onsets / _batch (a clip's transients, found on
 *    the device), zlhip_onset_resolve, zlhip_sound_tempo / _batch (a clip's tempo, estimated on the device), zlhip_tempo_resolve,
 *    zlhip_sound_pitch / _batch (a clip's pitch, detected on the device), zlhip_pitch_resolve, zlhip_sound_loudness / _batch (a clip's
 *    loudness, measured on the device), zlhip_loudness_resolve, zlhip_loudness_design, zlhip_sound_loop / _batch (a clip's seamless
 *    loop points, found on the device), zlhip_loop_resolve, zlhip_loop_seconds, zlhip_sound_key / _batch (a clip's musical
 *    key, detected on the device), zlhip_key_resolve, zlhip_key_design, zlhip_debug_live_resources, zlhip_sound_loop_crossfade / _batch (a loop crossfade
 *    baked into a clip's data on the device), zlhip_xfade_resolve, zlhip_xfade_design, zlhip_sound_edit / _batch (a clip's data cropped,
 *    trimmed of silence, reversed and faded on the device), zlhip_edit_resolve, zlhip_edit_design, zlhip_debug_edit_timings,
 *    zlhip_group_sound_edit_batch, zlhip_sound_peak / _batch (a clip's sample and true peak, measured on the device), zlhip_peak_resolve,
 *    zlhip_debug_peak_chunks, zlhip_sound_limit / _batch (a clip's peaks brought under a ceiling on the device), zlhip_limit_resolve,
 *    zlhip_limit_design, zlhip_debug_limit_timings, zlhip_group_sound_peak_batch, zlhip_group_sound_limit_batch. */
#define ZLHIP_ABI_VERSION 3

/* status codes */
#define ZLHIP_OK                 0
#define ZLHIP_ERR_INVALID       -1   /* bad argument */
#define ZLHIP_ERR_NO_DEVICE     -2   /* no usable HIP device / kernels not loadable */
#define ZLHIP_ERR_HIP           -3   /* a HIP runtime call failed (see zlhip_last_error) */
#define ZLHIP_ERR_CAPACITY      -4   /* arena / table / batch capacity exceeded */
#define ZLHIP_ERR_STATE         -5   /* call not valid in the current state */

/* render modes: 0 reproduces the reference bit for bit (quirks Q1/Q2 of SURVEY.md section 0) */
#define ZLHIP_MODE_FAITHFUL      0u
#define ZLHIP_MODE_FIX_GAIN      1u  /* gain/envelope/volume scale the whole interpolated sample */
#define ZLHIP_MODE_FIX_DELAY     2u  /* frame f is written to out[f] instead of out[f+1] */
#define ZLHIP_MODE_HERMITE       4u  /* build-defined extension: 4-tap Catmull-Rom interpolation */

#define ZLHIP_MAX_SLICES         128
#define ZLHIP_BEAT_SUBDIVISIONS  96  /* SyncTimer.cpp:95 */

typedef struct zlhip_engine zlhip_engine;

typedef struct zlhip_config {
    uint32_t struct_size;            /* sizeof(zlhip_config), for ABI growth */
    int32_t  device;                 /* HIP device ordinal */
    int32_t  num_buses;              /* SamplerChannels (reference: 12, SamplerSynth.cpp:258) */
    int32_t  voices_per_bus;         /* voices per channel (reference: 8, SamplerSynth.cpp:23) */
    int32_t  max_frames;             /* largest nframes per block, 1 .. 4096 (any JACK period: 16, 32, 441, 480 ... -- a block runs on whole 64-lane waves) */
    int32_t  max_batch_blocks;       /* largest nblocks per zlhip_render_batch call */
    int32_t  max_sounds;             /* clip / sound table size */
    uint32_t mode;                   /* ZLHIP_MODE_* */
    double   playback_sample_rate;   /* jack_get_sample_rate, SamplerSynth.cpp:271-272 */
    uint64_t sound_arena_bytes;      /* HBM reserved for decoded sources */
    int32_t  voices_per_task;        /* voices summed sequentially by one wavefront (mix group); 0 = the whole bus,
                                        i.e. the reference's order.  Smaller groups = two-level order, more parallelism.
                                        (With 0, single real-time blocks of buses of >= 32 voices are rendered one voice
                                        per workgroup and added in voice order: the same order, bit for bit.) */
    int32_t  plan_window_blocks;     /* blocks planned per window (planning of window i+1 overlaps rendering of window i);
                                        0 = automatic: 512 Ki frames at 1024 voices (2048 blocks of 256), proportionally
                                        more frames for fewer voices (up to 16 Mi), never more than max_batch_blocks */
    int32_t  rt_idle_timeout_us;     /* (ABI 2) how long the resident real-time kernel behind zlhip_render stays on the device
                                        without a cycle before it leaves (it is started again by the next cycle); 0 = 200 000.
                                        A host that makes device-synchronising HIP calls of its own (hipFree, hipDeviceSynchronize)
                                        waits at most this long behind an idle engine; calls made through this library do not wait. */
    uint64_t sound_arena_max_bytes;  /* (ABI 2) sound_arena_bytes is what the engine reserves at creation; when a source no longer fits it
                                        allocates further segments of at least that size, up to this total (0 = no limit but the
                                        device's memory; = sound_arena_bytes: a fixed arena, uploads beyond it fail with
                                        ZLHIP_ERR_CAPACITY until clips are released) */
} zlhip_config;

/* clock inputs of one block: JACK cycle times + SyncTimer playhead getters
 * (SamplerSynth.cpp:128, SyncTimer.cpp:990-1009) */
typedef struct zlhip_clock {
    uint64_t current_usecs;
    uint64_t next_usecs;
    uint64_t jack_playhead;
    uint64_t jack_playhead_usecs;
    uint64_t jack_subbeat_length_usecs;
} zlhip_clock;

/* snapshot of the ClipAudioSource fields the voice reads (ClipAudioSource.cpp:63-82) */
typedef struct zlhip_clip_params {
    float   start_position_seconds;
    float   length_seconds;
    float   length_in_beats;
    float   volume_absolute;         /* tracktion fader position in [0,1], taken as an input */
    float   pan;
    float   duration_seconds;        /* getDuration() */
    float   adsr_attack, adsr_decay, adsr_sustain, adsr_release;
    int32_t root_note;
    int32_t num_slice_positions;
    double  slice_positions[ZLHIP_MAX_SLICES];
} zlhip_clip_params;

/* ClipCommand (ClipCommand.h:11-32); `clip` is the id returned by zlhip_sound_upload */
typedef struct zlhip_clip_command {
    int32_t clip;
    int32_t midi_note;
    int32_t midi_channel;
    int32_t start_playback, stop_playback;
    int32_t change_slice, slice;
    int32_t change_looping, looping;
    int32_t change_pitch;   float pitch_change;
    int32_t change_speed;   float speed_ratio;
    int32_t change_gain_db; float gain_db;
    int32_t change_volume;  float volume;
} zlhip_clip_command;

/* what SamplerSynthVoice.cpp:265-267 hands to ClipAudioSourcePositionsModel, per voice slot */
typedef struct zlhip_voice_report {
    int32_t playing;                 /* voice->isPlaying after the render */
    int32_t valid;                   /* 1 if (gain, progress) were reported for the last rendered block */
    float   gain;                    /* peakGain * 0.5f */
    float   progress;                /* sourceSamplePosition / sourceSampleLength */
    int32_t clip;                    /* clip id the voice plays, -1 if none */
    int32_t reserved;
    double  source_sample_position;  /* d->sourceSamplePosition after the render (parity checks) */
} zlhip_voice_report;

/* AudioLevels per-channel meter state + outputs (AudioLevels.cpp:359-398) */
typedef struct zlhip_levels {
    int32_t peak_a, peak_b;                          /* integer peaks after decay + scan */
    float   peak_a_hold_signal, peak_b_hold_signal;  /* 0.9x hold (playback channel) */
    float   peak_db_a, peak_db_b, combined_db, hold_db_a, hold_db_b;
    float   rms_a, rms_b;                            /* build-defined extension: RMS of the scanned block */
} zlhip_levels;

/* JackPassthrough parameters (JackPassthrough.cpp:27-31) */
typedef struct zlhip_passthrough_params {
    float   dry_amount, wet_fx1_amount, wet_fx2_amount, pan_amount;
    int32_t muted;
} zlhip_passthrough_params;

/* profiling counters of the last zlhip_render_batch (HIP events on the engine's stream) */
typedef struct zlhip_timings {
    float plan_ms;        /* planning (K0+K1+K1c) not hidden behind rendering: start of the call on its stream to first K2 */
    float render_ms;      /* gather-interp-mix kernel (K2), the dominant one: sum over the call's launches */
    float finalize_ms;    /* total - render - plan: K3 (bus reduce + levels), reports, gaps between launches */
    float total_ms;       /* first launch to last completion */
    uint64_t source_bytes;   /* algorithmic source bytes of the batch: sum (ceil(N*ratio)+taps-1)*ch*4 */
    uint64_t slow_blocks;    /* voice-blocks that needed the per-frame control path */
    uint64_t active_voice_frames; /* voice-samples rendered */
    int32_t  render_launches;  /* K2 launches of the call (one per plan window); render_ms is their sum */
    int32_t  reserved;
} zlhip_timings;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int  zlhip_abi_version(void);
void zlhip_config_default(zlhip_config *cfg);
int  zlhip_engine_create(const zlhip_config *cfg, zlhip_engine **out);
void zlhip_engine_destroy(zlhip_engine *e);
const char *zlhip_last_error(const zlhip_engine *e);          /* borrowed, valid until the next call */
const char *zlhip_strerror(int status);

/* ---- sounds and clip parameters ----------------------------------------------------------- */
/* Upload a decoded source (planar fp32, right == NULL for mono) from host memory; returns its id
 * in *out_id.  The id doubles as the clip id (one SamplerSynthSound per ClipAudioSource). */
int zlhip_sound_upload(zlhip_engine *e, const float *left, const float *right, int32_t length,
                       double sample_rate, int32_t *out_id);
/* Same, but left/right are DEVICE pointers on the engine's device (no PCIe transfer).  The call waits for the device
 * (hipDeviceSynchronize) before it reads them: whatever stream produced the planes, they are complete. */
int zlhip_sound_upload_device(zlhip_engine *e, const float *left_dev, const float *right_dev, int32_t length,
                              double sample_rate, int32_t *out_id);
/* Same, with the stream the planes were produced on (hipStream_t; NULL = the null stream): the engine waits for that stream only
 * (an event), not for the device. */
int zlhip_sound_upload_device_on(zlhip_engine *e, const float *left_dev, const float *right_dev, int32_t length,
                                 double sample_rate, void *producer_stream, int32_t *out_id);
int zlhip_sound_release(zlhip_engine *e, int32_t id);          /* SamplerSynth::unregisterClip */
void zlhip_clip_params_default(zlhip_clip_params *p, float duration_seconds);   /* ClipAudioSource ctor defaults */
/* The parameters a voice reads per block (SamplerSynthVoice.cpp:189-196).  Host-only and wait-free: the edit is recorded and the
 * device applies it at the start of the next render call / real-time cycle, the block boundary at which the reference's voices
 * would read it; commands handled after the call see the new values (startNote, SamplerSynthVoice.cpp:115-121).  The resident
 * real-time kernel keeps running. */
int zlhip_clip_set(zlhip_engine *e, int32_t id, const zlhip_clip_params *p);

/* Clip re-render: ClipAudioSource::setGain / setPitch / setSpeedRatio re-render the clip's playback file from its source
 * (ClipAudioSource.cpp:279-311,404-413) and the sound reloads it (SamplerSynthSound.cpp:28-68).  The render is build-defined
 * (a SoundTouch-shaped WSOLA stretch by speed / 2^(pitch/12), a linear resampler by 2^(pitch/12), a gain)
 * and runs on the device: one seek launch and one synthesis launch per call, for every clip of the call.
 *   Ranges: speed_ratio in [0.25, 4], pitch_semitones in [-24, 24], finite gain_db; anything else is ZLHIP_ERR_INVALID.
 *   Every render starts from the ORIGINAL upload; gain 0, pitch 0, speed 1 goes back to it (no render, no copy).
 *   The playback data has max(1, floor(length / speed_ratio)) frames at the source's sample rate.  Clip parameters keep their
 *   meaning: start / length / slices are seconds of the playback data; duration_seconds stays the source's.
 *   The sound table switches at a block boundary (the resident real-time kernel leaves, queued batches finish first); the clip id
 *   keeps its slot, and a voice playing the clip reads the new data from its next block at its unchanged position.
 *   An arena that cannot hold the call returns ZLHIP_ERR_CAPACITY and leaves every clip as it was.
 * zlhip_sound_rerender_batch: ids must be distinct; all or nothing. */
typedef struct zlhip_rerender_params {
    float   gain_db;
    float   pitch_semitones;
    float   speed_ratio;
    int32_t reserved;                /* 0 */
} zlhip_rerender_params;
int zlhip_sound_rerender(zlhip_engine *e, int32_t id, const zlhip_rerender_params *params);
int zlhip_sound_rerender_batch(zlhip_engine *e, const int32_t *ids, const zlhip_rerender_params *params, int32_t count);
/* The sound's current playback data as planar fp32 (left / right: host [capacity]; right may be NULL, and is left alone for a mono
 * sound).  *length receives its frames; left == NULL asks for the length only.  Returns the number of channels (1 or 2), < 0 on
 * error (ZLHIP_ERR_CAPACITY: capacity < length). */
int zlhip_sound_read(zlhip_engine *e, int32_t id, float *left, float *right, int32_t capacity, int32_t *length);
/* Waveform overviews: the data behind the reference's WaveFormItem (lib/WaveFormItem.cpp:130-139 paints a juce::AudioThumbnail of the
 * clip between `start` and `end`) -- per pixel column the minimum and maximum of every channel, computed on the device from the
 * sound's CURRENT playback data (what a voice reads: after zlhip_sound_rerender the rendered extent).  The painting stays the host's.
 *   Column c of a request covers the frames [lo, hi): lo = first_frame + floor(c * num_frames / columns),
 *   hi = first_frame + floor((c + 1) * num_frames / columns) (int64); hi == lo (more columns than frames) makes it [lo, lo + 1).
 *   Order: samples are compared as integers -- the 32 bits of a negative value with all bits flipped, of a non-negative one with the
 *   sign bit flipped -- so -0 < +0, denormals come back with their own bits, a NaN with the sign bit clear lies above +inf and one
 *   with it set below -inf; the result does not depend on any order of evaluation.
 *   out: per column four floats (minL, maxL, minR, maxR); a mono sound repeats its channel in the R pair.  The requests of a batch
 *   are packed one behind the other, in request order, without gaps.
 *   Limits: 1 <= columns <= ZLHIP_OVERVIEW_MAX_COLUMNS, num_frames >= 1, first_frame >= 0, first_frame + num_frames <= the sound's
 *   length (zlhip_sound_read reports it), at most 262144 columns in one call: anything else is ZLHIP_ERR_INVALID; out_floats below
 *   4 per column is ZLHIP_ERR_CAPACITY.  On any error out is not written.
 *   A call is two kernel launches whatever its size, and moves 16 bytes per column to the host.  It runs on the engine's stream
 *   behind what is queued there, like zlhip_sound_read, and the resident real-time kernel keeps running -- except in the first call
 *   (and one that needs larger buffers than any before), which allocates the call's buffers. */
#define ZLHIP_OVERVIEW_MAX_COLUMNS 4096
typedef struct zlhip_overview_request { int32_t id, first_frame, num_frames, columns; } zlhip_overview_request;
int zlhip_sound_overview(zlhip_engine *e, int32_t id, int32_t first_frame, int32_t num_frames, int32_t columns, float *out /* [columns][4] */);
int zlhip_sound_overview_batch(zlhip_engine *e, const zlhip_overview_request *reqs, int32_t count, float *out, size_t out_floats);
/* measurement: device time of the last overview call made with profiling on (zlhip_set_profiling; HIP events on the engine's stream
 * around the call's launches) */
int zlhip_debug_overview_timings(zlhip_engine *e, float *device_ms);
/* Transients: the frames at which a sampler slices a loop (a build-defined extension, the reference has no
 * transient detection) -- found on the device in the sound's CURRENT playback data.  Everything behind the 16-bit quantisation
 * q = clamp(rint(4096 v), +-32767) (NaN -> 0) is integer arithmetic, so the result does not depend on any order of evaluation:
 *   E[h]: the sum of q^2 over the channels and the frames of hop h (hop_frames frames from first_frame on, the last hop cut at the
 *   request's end), E[-1] = 0; F = hop_frames * channels * gate^2; L(x) = 64 p + floor((x - 2^p) * 64 / 2^p), p = floor(log2 x);
 *   N[h] = max(0, L(E[h] + F) - L(E[h-1] + F)).  Hop h is a candidate if N[h] >= threshold, N[h] > N[j] for the min_gap_hops hops
 *   before it and N[h] >= N[j] for the min_gap_hops hops behind it.  More than max_onsets candidates: those with the largest N stay,
 *   equal N goes to the earlier hop.  A kept hop's onset is the start of the first sub-block of hop_frames / 16 frames, from one hop
 *   before h to the end of h, whose energy e has 4 e > E[h-1] + F; else the hop's first frame.
 *   out: the onsets (frame counted from the sound's first frame, strength = N[h]) in ascending frame order; *count / counts[i]: how
 *   many.  The requests of a batch are packed one behind the other, in request order, without gaps.
 *   A field given as 0 takes its default (zlhip_onset_resolve with the sound's sample rate): hop_frames = 16 * clamp(rint(rate / 3000),
 *   4, 256), gate = 8, threshold = 128, min_gap_hops = max(1, ceil(0.05 * rate / hop_frames)), max_onsets = 128.
 *   Limits: hop_frames a multiple of 16 in [64, 4096], gate in [1, 32767], threshold in [1, 4096], min_gap_hops in [1, 1024],
 *   max_onsets in [1, ZLHIP_ONSET_MAX_ONSETS], num_frames >= 1, first_frame >= 0, first_frame + num_frames <= the sound's length, at
 *   most 65536 hops per request and 4194304 per call, nreq >= 0: anything else is ZLHIP_ERR_INVALID; capacity below the sum of the
 *   resolved max_onsets is ZLHIP_ERR_CAPACITY.  On any error out and counts are not written; one bad request fails the call.
 *   A call is two kernel launches whatever its size, waits once and moves 8 bytes per onset and 4 per request to the host.  It runs
 *   on the engine's stream behind what is queued there and the resident real-time kernel keeps running, like zlhip_sound_overview. */
#define ZLHIP_ONSET_MAX_ONSETS 1024
typedef struct zlhip_onset_request { int32_t id, first_frame, num_frames, hop_frames, gate, threshold, min_gap_hops, max_onsets; } zlhip_onset_request;
typedef struct zlhip_onset { int32_t frame, strength; } zlhip_onset;
/* host only: fills the fields given as 0 and checks every limit that does not need the sound; a refused request is left as it was */
int zlhip_onset_resolve(double sample_rate, zlhip_onset_request *r);
int zlhip_sound_onsets(zlhip_engine *e, const zlhip_onset_request *r, zlhip_onset *out, int32_t capacity, int32_t *count);
int zlhip_sound_onsets_batch(zlhip_engine *e, const zlhip_onset_request *reqs, int32_t nreq, zlhip_onset *out, size_t capacity, int32_t *counts);
/* E and N of request `request` of the last call (energy / strength: [capacity], may be NULL to ask for *hops only) */
int zlhip_debug_onset_hops(zlhip_engine *e, int32_t request, uint64_t *energy, int32_t *strength, int32_t capacity, int32_t *hops);
/* measurement: device time of the energy pass and of the rest of the last call made with profiling on */
int zlhip_debug_onset_timings(zlhip_engine *e, float *energy_ms, float *rest_ms);
/* Tempo: how fast a loop is (a build-defined extension, the reference has no tempo estimate) -- estimated on the
 * device in the sound's CURRENT playback data.  The samples are read once, by the transients' energy pass; everything behind it is
 * integer arithmetic, so the result does not depend on any order of evaluation:
 *   E[h] as for zlhip_sound_onsets; R[h] = floor(sqrt(E[h])), R[-1] = 0; s = max(0, bitlength(max R) - 16);
 *   W[h] = max(0, R[h] - R[h-1]) >> s; sum = the sum of W.  l_min = max(1, ceil(60 rate / (hop_frames bpm_max))),
 *   l_max = floor(60 rate / (hop_frames bpm_min)), cap = (hops - 1) / 2, l_max = min(l_max, cap).
 *   A[l] = the sum over h >= l of W[h] W[h-l], for l = 0 and l in [max(1, l_min - 1), min(8 l_max + 8, cap + 1)].
 *   Lag a beats lag b iff A[a] (hops - b) > A[b] (hops - a); equal goes to the smaller lag.  lag_coarse = the best lag in
 *   [l_min, l_max]; then, with m = lag_coarse and doublings = 0: while doublings < 3 and 2m + 1 <= cap, m = the best of
 *   {2m-1, 2m, 2m+1} and doublings += 1; lag_fine = m, acf_lo / mid / hi = A[m-1], A[m], A[m+1], acf_zero = A[0].
 *   The host derives, in double: y_d = A[m+d] / (hops - m - d); den = (y- - 2 y0) + y+; delta = (y- - y+) / (2 den) if den < 0 else 0,
 *   clamped to +-0.5; period = (m + delta) / 2^doublings; bpm = 60 rate / (hop_frames period); mu = sum / hops;
 *   confidence = (y0 - mu^2) / (A[0] / hops - mu^2), 0 where that denominator is not positive.
 *   No tempo -- l_min > l_max (the frames are too few for the range) or A[0] == 0 (silence) -- is not an error: every field is 0
 *   except hops, shift, sum and acf_zero.
 *   A field given as 0 takes its default (zlhip_tempo_resolve with the sound's sample rate): hop_frames as for the transients,
 *   bpm_min = 75, bpm_max = 150 (one octave makes the answer unambiguous).
 *   Limits: hop_frames a multiple of 16 in [64, 4096]; bpm_min and bpm_max finite, 20 <= bpm_min < bpm_max <= 400; l_max <= 1024
 *   before the cut to cap; num_frames >= 1, first_frame >= 0, first_frame + num_frames <= the sound's length; at most 65536 hops per
 *   request and 4194304 per call; nreq >= 0: anything else is ZLHIP_ERR_INVALID.  On any error out is not written; one bad request
 *   fails the call.
 *   A call is four kernel launches whatever its size, behind one copy of the request records; it waits once and 72 bytes per request
 *   come back.  It runs on the engine's stream behind what is queued there and the resident real-time kernel keeps running. */
typedef struct zlhip_tempo_request { int32_t id, first_frame, num_frames, hop_frames; float bpm_min, bpm_max; } zlhip_tempo_request;
typedef struct zlhip_tempo { float bpm, confidence; int32_t lag_coarse, lag_fine, doublings, shift, hops, reserved;
                             uint64_t acf_lo, acf_mid, acf_hi, acf_zero, sum; } zlhip_tempo;
/* host only: fills the fields given as 0 and checks every limit that does not need the sound; a refused request is left as it was */
int zlhip_tempo_resolve(double sample_rate, zlhip_tempo_request *r);
int zlhip_sound_tempo(zlhip_engine *e, const zlhip_tempo_request *r, zlhip_tempo *out);
int zlhip_sound_tempo_batch(zlhip_engine *e, const zlhip_tempo_request *reqs, int32_t nreq, zlhip_tempo *out);
/* W and A of request `request` of the last call: flux [hops], acf [lags] = A[first_lag ...] (either may be NULL; both NULL asks for
 * *hops, *first_lag and *lags only; capacity: the elements each array given holds).  A[0] is the record's acf_zero. */
int zlhip_debug_tempo_acf(zlhip_engine *e, int32_t request, uint16_t *flux, uint64_t *acf, int32_t capacity, int32_t *hops, int32_t *first_lag, int32_t *lags);
/* measurement: device time of the energy pass, of the autocorrelation kernel and of the rest of the last call made with profiling on */
int zlhip_debug_tempo_timings(zlhip_engine *e, float *energy_ms, float *acf_ms, float *rest_ms);
/* Pitch: what note a clip is (a build-defined extension, the reference has no pitch detection) -- detected on
 * the device in the sound's CURRENT playback data: YIN's difference function, cumulative-mean normalisation and absolute threshold,
 * in integers behind the 16-bit quantisation, so the result does not depend on any order of evaluation:
 *   t_min = max(2, ceil(rate / f_max)), t_max = floor(rate / f_min); W = window; a frame needs L = W + t_max + 1 samples.
 *   num_frames < L: no frames.  Otherwise hop = W, K = (num_frames - L) / hop + 1; K > max_frames: K = max_frames and
 *   hop = (num_frames - L) / (max_frames - 1) (max_frames 1: K = 1); frame k starts at first_frame + k hop.
 *   m[f] = the sum over the channels of clamp(rint(4096 v), +-32767) (NaN -> 0); e = the sum of m^2 over the frame's first W samples;
 *   e < W channels gate^2: the frame is silent.  sh = max(0, bitlength(max |m| over the L samples) - 12), x = m >> sh (arithmetic).
 *   d[t] = the sum over j < W of (x[j] - x[j + t])^2 for t in [1, t_max + 1]; C[t] = d[1] + ... + d[t].
 *   t0 = the smallest t in [t_min, t_max] with d[t] t 1024 < threshold C[t] (uint64); none: the frame is unvoiced.
 *   The frame's lag = the first t >= t0 with t = t_max or d[t + 1] >= d[t]; clarity = L(C[lag] + 1) - L(d[lag] lag + 1), L the
 *   transients' level (a log2 in 1/64 octaves).  A frame's record (zlhip_pitch_frame): lag, clarity, shift, flag (0 voiced, 1 silent,
 *   2 unvoiced), d_lo / d_mid / d_hi = d[lag - 1], d[lag], d[lag + 1], cum = C[lag]; silent and unvoiced frames: 0 except shift, flag.
 *   The vote: voiced = the voiced frames, t_med = their lower median lag, a frame is consistent if |lag - t_med| <= t_med >> 5,
 *   the representative (`frame`) is the consistent frame with the largest clarity, equal values go to the earlier frame; lag, shift,
 *   clarity, d_lo, d_mid, d_hi, cum are its record's.
 *   The host derives, in double: den = (d_lo - 2 d_mid) + d_hi; delta = (d_lo - d_hi) / (2 den) if den > 0 else 0, clamped to
 *   +-0.5; hz = rate / (lag + delta); note = 69 + 12 log2(hz / 440); root_note = clamp(rint(note), 0, 127);
 *   cents = 100 (note - root_note); confidence = consistent / frames.
 *   No pitch -- no frames (num_frames < L) or no voiced frame (silence, noise, a drum hit) -- is not an error: every field is 0
 *   except frames.  A note above f_max comes back an octave (or more) low: choose f_max above the material.
 *   A field given as 0 takes its default (zlhip_pitch_resolve with the sound's sample rate): f_min = 55, f_max = 1760,
 *   threshold = 154 (0.15), gate = 8, max_frames = 64, window = min(4096, roundup(2 t_max, 64)).
 *   Limits: window a multiple of 64 in [256, 4096]; t_max + 1 <= min(2048, window); f_min and f_max finite,
 *   20 <= f_min < f_max < rate / 2; threshold in [1, 1024]; gate in [1, 32767]; max_frames in [1, 256]; num_frames >= 1,
 *   first_frame >= 0, first_frame + num_frames <= the sound's length; at most 65536 analysis frames per call; nreq >= 0: anything
 *   else is ZLHIP_ERR_INVALID.  On any error out is not written; one bad request fails the call.
 *   A call is three kernel launches whatever its size, behind one copy of the request records; it waits once and 80 bytes per request
 *   come back.  It runs on the engine's stream behind what is queued there and the resident real-time kernel keeps running. */
typedef struct zlhip_pitch_request { int32_t id, first_frame, num_frames, window, max_frames; float f_min, f_max; int32_t threshold, gate; } zlhip_pitch_request;
typedef struct zlhip_pitch { float hz, note, cents, confidence; int32_t root_note, frames, voiced, consistent, frame, lag, shift, clarity;
                             uint64_t d_lo, d_mid, d_hi, cum; } zlhip_pitch;
typedef struct zlhip_pitch_frame { int32_t lag, clarity, shift, flag; uint64_t d_lo, d_mid, d_hi, cum; } zlhip_pitch_frame;
/* host only: fills the fields given as 0 and checks every limit that does not need the sound; a refused request is left as it was */
int zlhip_pitch_resolve(double sample_rate, zlhip_pitch_request *r);
int zlhip_sound_pitch(zlhip_engine *e, const zlhip_pitch_request *r, zlhip_pitch *out);
int zlhip_sound_pitch_batch(zlhip_engine *e, const zlhip_pitch_request *reqs, int32_t nreq, zlhip_pitch *out);
/* the frame records of request `request` of the last call (records: [capacity], may be NULL to ask for *frames only) */
int zlhip_debug_pitch_frames(zlhip_engine *e, int32_t request, zlhip_pitch_frame *records, int32_t capacity, int32_t *frames);
/* d[1 .. t_max + 1] of frame `frame` of request `request` of the last call (d: [capacity], may be NULL to ask for *lags = t_max + 1 only) */
int zlhip_debug_pitch_diff(zlhip_engine *e, int32_t request, int32_t frame, uint64_t *d, int32_t capacity, int32_t *lags);
/* measurement: device time of the difference-function kernel and of the rest of the last call made with profiling on */
int zlhip_debug_pitch_timings(zlhip_engine *e, float *diff_ms, float *rest_ms);
/* Loudness: how loud a clip is (a build-defined extension, the reference has no loudness measurement) -- the
 * integrated loudness of ITU-R BS.1770-4 / EBU R 128 and the sample peak of the sound's CURRENT playback data, measured on the device:
 *   K-weighting: two biquads per channel (a high shelf, the RLB high-pass), designed for the sound's rate in double
 *   (zlhip_loudness_design: coeffs[0..4] = the shelf's b0 b1 b2 a1 a2, coeffs[5..9] = the high-pass's 1 -2 1 a1 a2; at 48 kHz BS.1770's
 *   tables), run in double as transposed direct form II, o = b0 v + s1; s1 = (b1 v - a1 o) + s2; s2 = b2 v - a2 o, one IEEE operation
 *   per operator.  A non-finite sample is 0; subnormals are kept.
 *   sub = sub_frames (given as 0: floor(rate 0.1 + 0.5), 100 ms); S = num_frames / sub whole sub-blocks.  Sub-block k is filtered from
 *   zero state at the start of sub-block k - 1 (sub-block 0: at first_frame) and its own outputs are squared and summed per channel in
 *   sample order: a zlhip_loudness_sub per sub-block, sum[2] and peak[2] (max |v| over its finite samples; the last one also scans
 *   the remainder behind the S whole sub-blocks for the peak); a mono sound leaves sum[1] = peak[1] = 0.  Against one serial pass the
 *   warm-up changes a sub-block's sum by less than 1e-10 relative.
 *   u[k] = sum[0] + sum[1]; the blocks j = 0 .. S - 4: z_j = (((u[j] + u[j+1]) + u[j+2]) + u[j+3]) / (4 sub), 400 ms with 75 % overlap.
 *   S < 4 (a one-shot shorter than 400 ms): the sub-blocks are ceil(num_frames / sub), the last one partial, and there is one block
 *   over the whole region, z_0 = (u[0] + u[1] + ...) / num_frames.
 *   The blocks with z_j > 1.1724653045822981e-07 (-70 LUFS) pass the absolute gate, above_absolute of them; relative_gate = their
 *   mean / 10; the blocks above both gates, above_relative of them, give mean_square = their mean and
 *   lufs = -0.691 + 10 log10(mean_square).  No block above -70 LUFS -- silence -- is not an error: lufs = -inf, mean_square =
 *   relative_gate = 0, above_absolute = above_relative = 0.  peak[c] is the largest sample peak of channel c; sub_blocks and blocks
 *   count what was summed.
 *   Limits: num_frames >= 1, first_frame >= 0, first_frame + num_frames <= the sound's length; sub_frames 0 or in [16, 131072]; at
 *   most 65536 sub-blocks per request and 1048576 per call; nreq >= 0: anything else is ZLHIP_ERR_INVALID.  On any error out is not
 *   written; one bad request fails the call.
 *   A call is one kernel launch whatever its size, behind one copy of the request records; it waits once and 24 bytes per sub-block
 *   come back.  It runs on the engine's stream behind what is queued there and the resident real-time kernel keeps running.
 *   (The true peak: zlhip_sound_peak, below.)
 *   Not provided: loudness range, momentary / short-term meters (the
 *   sub-block sums are there through zlhip_debug_loudness_subs), channel weights beyond stereo. */
typedef struct zlhip_loudness_request { int32_t id, first_frame, num_frames, sub_frames; } zlhip_loudness_request;
typedef struct zlhip_loudness { double lufs, mean_square, relative_gate; float peak[2]; int32_t sub_blocks, blocks, above_absolute, above_relative; } zlhip_loudness;
typedef struct zlhip_loudness_sub { double sum[2]; float peak[2]; } zlhip_loudness_sub;
/* host only: fills sub_frames given as 0 and checks every limit that does not need the sound; a refused request is left as it was */
int zlhip_loudness_resolve(double sample_rate, zlhip_loudness_request *r);
/* host only: the ten K-weighting coefficients for a sample rate (coeffs: [10]) */
int zlhip_loudness_design(double sample_rate, double *coeffs);
int zlhip_sound_loudness(zlhip_engine *e, const zlhip_loudness_request *r, zlhip_loudness *out);
int zlhip_sound_loudness_batch(zlhip_engine *e, const zlhip_loudness_request *reqs, int32_t nreq, zlhip_loudness *out);
/* the sub-block records of request `request` of the last call (records: [capacity], may be NULL to ask for *count only) */
int zlhip_debug_loudness_subs(zlhip_engine *e, int32_t request, zlhip_loudness_sub *records, int32_t capacity, int32_t *count);
/* measurement: device time of the kernel of the last call made with profiling on */
int zlhip_debug_loudness_timings(zlhip_engine *e, float *kernel_ms);
/* Loop points: where a clip's sustain loop wraps without a click (a build-defined extension, the reference has
 * no loop finder) -- searched on the device in the sound's CURRENT playback data of `length` frames, near the nominal loop
 * [start_frame s0, stop_frame e0), in integers behind the 16-bit quantisation, so the result does not depend on any order of evaluation:
 *   W = window, H = W / 2.  Starts s in [max(s0 - Rs, H), min(s0 + Rs, length - H)], ends e in [max(e0 - Re, H), min(e0 + Re,
 *   length - H)] (Rs = start_search, Re = stop_search; -1: "this point stays", the nominal point alone): the window [p - H, p + H) of
 *   a candidate lies inside the data.  A pair is admissible if e - s >= min_length.  A loop over the whole file has its points inside
 *   H of the data's ends, so its candidates begin H frames in: the service is meant for sustain loops inside a sound, not for beat
 *   loops that trust the file's edges.
 *   m[f] = the sum over the channels of clamp(rint(4096 v), +-32767) (NaN -> 0); one shift per request,
 *   sh = max(0, bitlength(max |m| over the two strips [smin - H, smax + H) and [emin - H, emax + H)) - 10), x = m >> sh (arithmetic).
 *   cost(s, e) = the sum over j in [-H, H) of (x[s + j] - x[e + j])^2 (uint32); E(p) = the sum of x[p + j]^2 over the window;
 *   den(s, e) = E(s) + E(e) + 1.  Pair a is better than pair b under the first rule that differs: cost_a den_b < cost_b den_a
 *   (uint64); the smaller |s - s0| + |e - e0|; the smaller s; the smaller e.
 *   zlhip_loop: found, start_frame, stop_frame (the best admissible pair), shift, starts, ends (the candidates), pairs (the
 *   admissible pairs), cost, den, nominal_valid (1 when (s0, e0) is itself an admissible candidate pair), nominal_cost, nominal_den.
 *   The host derives, in double: seam_db = -120 where cost == 0, else max(-120, 10 log10(cost / den)); nominal_db the same way;
 *   improvement_db = nominal_db - seam_db, or 0 without a nominal.
 *   An empty range or no admissible pair is not an error: found = 0 and every other field is 0.
 *   A field given as 0 takes its default (zlhip_loop_resolve with the sound's sample rate): start_search and stop_search
 *   min(2047, rint(0.010 rate)), window 256, min_length = window.
 *   Limits: start_search and stop_search in [-1, 2047]; window a multiple of 16 in [16, 1024]; min_length >= 1;
 *   0 <= start_frame < stop_frame <= the sound's length; at most 65536 work items (tiles of 64 starts x 64 ends) and 4194304 strip
 *   frames (ns - 1 + W and ne - 1 + W per request, each rounded up to 8) per call; nreq >= 0: anything else is ZLHIP_ERR_INVALID.
 *   On any error out is not written; one bad request fails the call.
 *   A call is three kernel launches whatever its size, behind one copy of the request records; it waits once and 80 bytes per request
 *   come back.  It runs on the engine's stream behind what is queued there and the resident real-time kernel keeps running.
 *   Not provided: loop points for beat loops at the file's edges.  (A crossfade baked into the data: zlhip_sound_loop_crossfade, below.) */
typedef struct zlhip_loop_request { int32_t id, start_frame, stop_frame, start_search, stop_search, window, min_length; } zlhip_loop_request;
typedef struct zlhip_loop { int32_t found, start_frame, stop_frame, shift, starts, ends, nominal_valid, reserved; uint64_t pairs;
                            uint32_t cost, den, nominal_cost, nominal_den; double seam_db, nominal_db, improvement_db; } zlhip_loop;
/* a work item's record: its best admissible pair (none: start = stop = -1, cost = den = 0) and how many admissible pairs it holds */
typedef struct zlhip_loop_item { int32_t start, stop; uint32_t cost, den; uint64_t pairs; } zlhip_loop_item;
/* host only: fills the fields given as 0 and checks every limit that does not need the sound; a refused request is left as it was */
int zlhip_loop_resolve(double sample_rate, zlhip_loop_request *r);
int zlhip_sound_loop(zlhip_engine *e, const zlhip_loop_request *r, zlhip_loop *out);
int zlhip_sound_loop_batch(zlhip_engine *e, const zlhip_loop_request *reqs, int32_t nreq, zlhip_loop *out);
/* host only: the float seconds from which a voice derives exactly these frames -- start = (int)(start_seconds * rate),
 * stop = (int)((float)(start_seconds + length_seconds) * rate).  ZLHIP_ERR_INVALID where no such floats are found within 8 single
 * steps around the frames' middles (from about 2^23 frames on some pairs are not representable) */
int zlhip_loop_seconds(double sample_rate, int64_t start_frame, int64_t stop_frame, float *start_seconds, float *length_seconds);
/* the item records of request `request` of the last call, start tile by start tile (items: [capacity], may be NULL to ask for *count only) */
int zlhip_debug_loop_items(zlhip_engine *e, int32_t request, zlhip_loop_item *items, int32_t capacity, int32_t *count);
/* every candidate pair's cost, [starts][ends], of request `request` of the last call (costs: [capacity], may be NULL to ask for the
 * counts only).  Kept only where the call had at most 1048576 candidate pairs: ZLHIP_ERR_STATE otherwise */
int zlhip_debug_loop_costs(zlhip_engine *e, int32_t request, uint32_t *costs, int32_t capacity, int32_t *starts, int32_t *ends);
/* measurement: device time of the pairs kernel and of the rest of the last call made with profiling on */
int zlhip_debug_loop_timings(zlhip_engine *e, float *pairs_ms, float *rest_ms);
/* Loop crossfade: the X frames in front of a loop's stop faded into the X frames in front of its start, baked into the clip's data on
 * the device (a build-defined extension, the reference has no loop crossfade).  The loop finder only chooses among
 * points that exist; a decaying pad or a loop placed by ear still jumps from x[stop - 1] to x[start] on every lap.
 *   A request is (id, start_frame s, stop_frame e, fade_frames X, curve) over the slot's ORIGINAL data of `length` frames,
 *   0 <= s < e <= length, e exclusive.  fade_frames 0 means min(rint(0.020 rate), s, e - s, 65536); where that is 0 (a loop from frame 0
 *   has no lead-in) the request answers applied = 0 and every other field 0, which is no error: the clip is left alone.  An explicit
 *   fade_frames lies in [1, min(s, e - s, 65536)], curve is ZLHIP_XFADE_AUTO, _LINEAR or _EQUAL_POWER: anything else is
 *   ZLHIP_ERR_INVALID, as are ids not in use or repeated and count < 0 -- all decided before the first HIP call.
 *   Correlation: m[f] = the sum over the channels of q(v) (section 8's 16-bit quantisation); sab = the sum over i in [0, X) of
 *   m[e - X + i] m[s - X + i], saa and sbb likewise, exact in int64; correlation = sab / sqrt(saa sbb) (0 where saa or sbb is 0), in
 *   double on the host.  Always measured and reported.
 *   Weights: rho = min(1, max(0, correlation)) for AUTO, 1 for LINEAR, 0 for EQUAL_POWER (the result's rho is the one used); for
 *   i in [0, X): t = (i + 1) / X, u = 1 - t, d = sqrt(((u u) + (t t)) + ((2 rho) (t u))), a[i] = (float)(u / d), b[i] = (float)(t / d), in
 *   double on the host: a^2 + b^2 + 2 rho a b = 1, the power of material of that correlation stays constant through the fade.
 *   Output: y[e - X + i] = (a[i] x[e - X + i]) + (b[i] x[s - X + i]) per channel in fp32, two rounded multiplies and a rounded add;
 *   every other frame is copied bit for bit into a new arena extent.  The loop's last frame becomes the frame in front of the loop's
 *   start, so the wrap e - 1 -> s is the original's own step s - 1 -> s.  ZL_SOUND_FINITE stays set iff the original had it and every
 *   written fade sample is finite.
 *   A clip that currently plays a re-render is ZLHIP_ERR_STATE; an arena that cannot hold the whole call is ZLHIP_ERR_CAPACITY.  All
 *   or nothing: on any error every clip is as it was and out is not written; one bad request fails the call.
 *   Synchronisation is zlhip_sound_convert_rate's: the resident kernel leaves, queued batches finish, the table entries switch at a
 *   block boundary.  A call is one measuring launch, a wait, one render launch and one publishing launch, a second wait -- whatever
 *   the number of requests; a call whose every request answers applied = 0 launches and copies nothing.
 *   Consequences.  A baked fade cannot be taken back: reload the clip.  The new extent becomes the clip's ORIGINAL: a later re-render
 *   starts from the crossfaded data -- a gain keeps the seam, a pitch or speed render moves the frames and the loop must be placed
 *   again.  A voice playing the clip reads the new data from its next block at its unchanged position.  The fade serves the
 *   free-running loop branch; a clip whose lengthInBeats is whole restarts by the clock and does not pass the seam.
 *   Not provided: a guard copy of x[s ...] behind the stop for the interpolation taps of pitched laps (it would change data a
 *   non-looping command plays); undo; fades for beat-locked restarts; fading under a re-render. */
enum { ZLHIP_XFADE_AUTO = 0, ZLHIP_XFADE_LINEAR = 1, ZLHIP_XFADE_EQUAL_POWER = 2 };
typedef struct zlhip_xfade_request { int32_t id, start_frame, stop_frame, fade_frames, curve; } zlhip_xfade_request;
typedef struct zlhip_xfade { int32_t applied, fade_frames, start_frame, stop_frame, curve, reserved; int64_t sab, saa, sbb;
                             double correlation, rho; } zlhip_xfade;
/* host only: checks the request against a sound of `length` frames at `sample_rate` and fills fade_frames where it was given as 0
 * (it stays 0 where there is nothing to fade); a refused request is left as it was */
int zlhip_xfade_resolve(double sample_rate, int32_t length, zlhip_xfade_request *r);
/* host only: the X weight pairs (a[i], b[i]) of a correlation, ab: [2 X]; X outside [1, 65536] or rho outside [0, 1] is
 * ZLHIP_ERR_INVALID.  The engine builds its tables with this code */
int zlhip_xfade_design(int32_t fade_frames, double rho, float *ab);
int zlhip_sound_loop_crossfade(zlhip_engine *e, const zlhip_xfade_request *r, zlhip_xfade *out);
int zlhip_sound_loop_crossfade_batch(zlhip_engine *e, const zlhip_xfade_request *reqs, int32_t count, zlhip_xfade *out);
/* measurement: device time of the measuring launch and of the render and publishing launches of the last call made with profiling on */
int zlhip_debug_xfade_timings(zlhip_engine *e, float *measure_ms, float *render_ms);
/* Clip edit: a clip's data cropped to a region, trimmed of the silence at its ends, reversed, its ends faded -- on the device, under the
 * clip's own id (a build-defined extension, the reference has no such edit).  The route without it is
 * zlhip_sound_read, a host loop and zlhip_sound_upload, which gives the clip a new id: every voice and command that names it loses it.
 *   A request acts on the slot's ORIGINAL data of `length` frames.  first_frame a, num_frames: the region to keep is [a, b);
 *   num_frames 0 means "to the end" (a < length), else 0 <= a, num_frames >= 1, a + num_frames <= length.  flags: ZLHIP_EDIT_TRIM |
 *   ZLHIP_EDIT_REVERSE, no other bit.  threshold (fp32; used with TRIM only): 0 means 2^-10 (about -60 dBFS), else finite and above 0.
 *   pre_roll_frames, hold_frames (TRIM only), fade_in_frames, fade_out_frames: >= 0.  curve: ZLHIP_EDIT_LINEAR, _SQRT or _SMOOTH.
 *   Anything else is ZLHIP_ERR_INVALID, as are ids not in use or repeated and count < 0 -- all decided before the first HIP call.
 *   Trim: exact, no quantisation.  Frame f is loud iff for some channel !(fabsf(x[f][c]) < threshold) in fp32: NaN and +-inf are loud,
 *   |x| == threshold is loud.  F and Z are the smallest and the largest loud frame of [a, b).  No loud frame: silent = 1, applied = 0,
 *   the clip is untouched, no error.  Else a' = max(a, F - pre_roll_frames), b' = min(b, Z + 1 + hold_frames) (int64).  Without TRIM
 *   a' = a, b' = b.  n = b' - a'.
 *   Fades: cut so that they never overlap, Xi = min(fade_in_frames, n / 2), Xo = min(fade_out_frames, n / 2); the weights are made on
 *   the host in double, for i in [0, X) with t = i / X: LINEAR w = t, SQRT w = sqrt(t) (two clips faded against each other keep constant
 *   power), SMOOTH w = (t t) (3 - (2 t)), then rounded to fp32; w[0] = 0.
 *   Output: n frames, the original's channels and rate.  Output frame i is source frame b' - 1 - i with REVERSE, a' + i without; a
 *   frame i < Xi is multiplied by w_in[i], a frame i >= n - Xo by w_out[n - 1 - i], one rounded fp32 multiply per sample (the fades act
 *   on the data after the reversal); every other sample is copied bit for bit into a new arena extent.
 *   Identity: a' = 0, n = length, no REVERSE, Xi = Xo = 0 answers applied = 0, takes no extent and is copied by no launch; a TRIM that
 *   finds nothing to cut is such a request.
 *   ZL_SOUND_FINITE stays set iff the original had it and every written faded sample is finite.  A clip without the flag never gains
 *   it, even when its non-finite samples were cropped away: copied samples are not looked at.
 *   The result: applied, silent; first_frame, num_frames: the kept region [a', b') in source frames (the asked region where silent);
 *   first_loud, last_loud: F and Z (-1 without TRIM or where silent); fade_in_frames, fade_out_frames as cut (0 where not applied);
 *   length: the clip's length now; reversed; curve.
 *   A clip that currently plays a re-render is ZLHIP_ERR_STATE; an arena that cannot hold the whole call is ZLHIP_ERR_CAPACITY, decided
 *   behind the scan, which changes nothing.  All or nothing: on any error every clip is as it was and out is not written.
 *   Synchronisation is zlhip_sound_convert_rate's.  A call with a TRIM request is a scanning launch, a wait, one render launch and one
 *   publishing launch, a second wait; a call without one skips the scan and its wait -- whatever the number of requests; a call whose
 *   every request answers applied = 0 copies and renders nothing.
 *   Consequences.  There is no undo: reload the clip.  The new extent becomes the clip's ORIGINAL: a later re-render starts from the
 *   edited data.  Clip parameters are seconds and keep their values: the caller moves start and length (libzl_hotpath_clip_trim_silence,
 *   _crop and _reverse do).  A voice that plays the clip during the call keeps its frame position, which is safe and musically wrong:
 *   edit before playing.
 *   Not provided: undo; extracting a region into a NEW clip, or slices into clips; a baked gain alone (zlhip_sound_limit bakes one under a
 *   ceiling; the clip's gain re-render stays the reversible route); DC removal; editing under a re-render; fades at a region inside the data. */
enum { ZLHIP_EDIT_TRIM = 1, ZLHIP_EDIT_REVERSE = 2 };
enum { ZLHIP_EDIT_LINEAR = 0, ZLHIP_EDIT_SQRT = 1, ZLHIP_EDIT_SMOOTH = 2 };
typedef struct zlhip_edit_request { int32_t id, first_frame, num_frames, flags, pre_roll_frames, hold_frames, fade_in_frames, fade_out_frames, curve;
                                    float threshold; } zlhip_edit_request;
typedef struct zlhip_edit { int32_t applied, silent, first_frame, num_frames, first_loud, last_loud, fade_in_frames, fade_out_frames, length,
                            reversed, curve, reserved; } zlhip_edit;
/* host only: checks the request against a sound of `length` frames and fills num_frames and threshold where they were given as 0; a
 * refused request is left as it was */
int zlhip_edit_resolve(int32_t length, zlhip_edit_request *r);
/* host only: the X weights of a fade, rising from w[0] = 0, w: [X]; X < 1 or an unknown curve is ZLHIP_ERR_INVALID.  The engine builds
 * its tables with this code */
int zlhip_edit_design(int32_t fade_frames, int32_t curve, float *w);
int zlhip_sound_edit(zlhip_engine *e, const zlhip_edit_request *r, zlhip_edit *out);
int zlhip_sound_edit_batch(zlhip_engine *e, const zlhip_edit_request *reqs, int32_t count, zlhip_edit *out);
/* measurement: device time of the scanning launch (0 for a call without TRIM) and of the render and publishing launches of the last
 * call made with profiling on */
int zlhip_debug_edit_timings(zlhip_engine *e, float *scan_ms, float *render_ms);
/* Peaks: a clip's sample peak and true peak measured on the device, and a look-ahead limiter that brings the few peaks of a clip under a
 * ceiling and leaves everything else as it was, bit for bit, under the clip's own id (a build-defined extension,
 * the reference has neither).  All arithmetic is fp32, one IEEE operation per operator, nothing fused.
 *   Detector.  v = x gain (one rounded multiply).  Sample peak of a frame and channel: |v|.  Inter-sample peak ips[f][c], with
 *   ZLHIP_LIMIT_TRUE_PEAK: the oversampling factor F is 4 for a rate below 70000, 2 below 140000, else 1 (BS.1770-4 Annex 2); the filter
 *   is zlhip_resample_design(rate, F rate)'s table unchanged (L = F, M = 1, 64 taps), rows p = 1 .. F - 1: y = sum over t of
 *   h[p][t] v[f - 31 + t] in increasing t, a rounded multiply and a rounded add per tap, v = +0 outside the request's region;
 *   ips[f][c] = max over p of |y|, ips[-1] = 0, and 0 with F = 1.  A rate the design refuses, with the flag, is ZLHIP_ERR_INVALID.  The frame
 *   detector is p[f] = max over the channels of max(|v[f]|, ips[f - 1], ips[f]); without the flag max over the channels of |v[f]|.
 *   Maxima compare bits: every order gives the same answer.
 *   zlhip_sound_peak: request { id, first_frame, num_frames, flags } over the sound's CURRENT playback data (num_frames >= 1, the region
 *   inside the data); gain 1, a non-finite sample is +0.  The device writes one record { sample_peak[2], inter_peak[2] } per chunk of 1024
 *   frames of the region (zlhip_debug_peak_chunks), maxima over the chunk's own frames, a mono sound leaves index 1 zero; the host takes
 *   the maxima: true_peak = max(sample_peak, inter_peak); oversampling = F (1 without the flag), chunks.  One launch, one wait; the
 *   resident real-time kernel keeps running.
 *   zlhip_sound_limit: request { id, flags, lookahead_frames L, hold_frames H, ceiling c, gain } over the slot's ORIGINAL data, the whole
 *   clip, n frames.  zlhip_limit_resolve fills the defaults: ceiling 0 means (float)0.8912509381337456 (-1 dBFS), else finite in (0, 1];
 *   gain 0 means 1, else finite and above 0; lookahead_frames 0 means floor(rate 0.005 + 0.5) clipped to [1, 512], else in [1, 512];
 *   hold_frames in [0, 512]; a flag other than TRUE_PEAK, or anything else, is ZLHIP_ERR_INVALID.
 *     1. g[f] = p[f] > c ? c / p[f] : 1; r[f] = 1 - g[f].  (The limiter works on the reduction: nothing above the ceiling means r = 0,
 *        R = 0 and G = 1 exactly.)
 *     2. mr[i] = max r[j] over j in [max(i - H, 0), min(i + L, n - 1)], i in [-L, n - 1].
 *     3. R[f] = sum over k = 0 .. L of w[k] mr[f - k], from +0 in increasing k, a rounded multiply and a rounded add per tap;
 *        w[k] = (double)((k + 1)(L + 1 - k)) / (double)((L + 1)(L + 2)(L + 3) / 6), rounded to fp32 (zlhip_limit_design).
 *     4. G[f] = max(1 - R[f], 0).
 *     5. y = v G[f]; out = y > c ? c : (y < -c ? -c : y).  No output sample exceeds c; the clamp moves a sample by at most
 *        |v| (L + 4) 2^-23.  A frame more than L frames before and more than L + H frames behind every hot frame is v, bit for bit.
 *   The output is not delayed and keeps length, channels and rate; attack and release are both the L-frame ramp.
 *   gain == 1 and the detector's maximum <= c: applied = 0, no extent, no render.  gain != 1 and nothing hot: applied = 1, every sample
 *   is x gain.  The clip must have ZL_SOUND_FINITE (else ZLHIP_ERR_STATE) and keeps it iff every written sample is finite.
 *   The result: applied, lookahead_frames, hold_frames, oversampling, frames_reduced (frames with G < 1), peak_before (the detector's
 *   maximum), min_gain (the smallest G), ceiling, gain.
 *   A clip that plays a re-render is ZLHIP_ERR_STATE; ids not in use or repeated are ZLHIP_ERR_INVALID; an arena that cannot hold the
 *   applied clips is ZLHIP_ERR_CAPACITY, decided behind the detecting pass, which changes nothing.  All or nothing; on any error out is
 *   not written.  Synchronisation is zlhip_sound_edit's: a detecting launch, a wait, one render and one publishing launch, a second wait.
 *   Not provided: a separate release time (a recursive release is serial); a guarantee on the TRUE peak of the output (gain modulation can
 *   recreate small inter-sample overs: measure with zlhip_sound_peak afterwards); undo; limiting a region; limiting under a re-render. */
enum { ZLHIP_LIMIT_TRUE_PEAK = 1 };
typedef struct zlhip_peak_request { int32_t id, first_frame, num_frames, flags; } zlhip_peak_request;
typedef struct zlhip_peak { float sample_peak[2], true_peak[2]; int32_t oversampling, chunks; } zlhip_peak;
typedef struct zlhip_peak_chunk { float sample_peak[2], inter_peak[2]; } zlhip_peak_chunk;
typedef struct zlhip_limit_request { int32_t id, flags, lookahead_frames, hold_frames; float ceiling, gain; } zlhip_limit_request;
typedef struct zlhip_limit { int32_t applied, lookahead_frames, hold_frames, oversampling, frames_reduced; float peak_before, min_gain, ceiling, gain;
                             int32_t reserved; } zlhip_limit;
/* host only: checks the request against a sound of `length` frames at `sample_rate` */
int zlhip_peak_resolve(double sample_rate, int32_t length, const zlhip_peak_request *r);
int zlhip_sound_peak(zlhip_engine *e, const zlhip_peak_request *r, zlhip_peak *out);
int zlhip_sound_peak_batch(zlhip_engine *e, const zlhip_peak_request *reqs, int32_t nreq, zlhip_peak *out);
/* the chunk records of request `request` of the last call (records: [capacity], may be NULL to ask for *count only) */
int zlhip_debug_peak_chunks(zlhip_engine *e, int32_t request, zlhip_peak_chunk *records, int32_t capacity, int32_t *count);
/* host only: fills the fields given as 0 and checks every limit; a refused request is left as it was */
int zlhip_limit_resolve(double sample_rate, zlhip_limit_request *r);
/* host only: the L + 1 weights of the window, w: [L + 1]; L outside [1, 512] is ZLHIP_ERR_INVALID.  The engine builds its tables with this code */
int zlhip_limit_design(int32_t lookahead_frames, float *w);
int zlhip_sound_limit(zlhip_engine *e, const zlhip_limit_request *r, zlhip_limit *out);
int zlhip_sound_limit_batch(zlhip_engine *e, const zlhip_limit_request *reqs, int32_t count, zlhip_limit *out);
/* measurement: device time of the detecting launch and of the render and publishing launches of the last limit call made with profiling on */
int zlhip_debug_limit_timings(zlhip_engine *e, float *detect_ms, float *render_ms);
/* Warp: a clip fitted to the session grid on the device, a time stretch cut at the clip's hits (a build-defined
 * extension, the reference has no warp).  A uniform stretch leaves a hit that is early or late early or late; here every region between
 * two anchors gets its own ratio, starts exactly at its anchor with no seek (the attack is copied 1:1) and is searched by its own
 * workgroup.
 *   A request is (id, count, anchors[count]), each anchor (src_frame a, dst_frame d), over the slot's ORIGINAL data of `length` frames:
 *   2 <= count <= ZLHIP_WARP_MAX_ANCHORS, anchors[0] = (0, 0), anchors[count - 1].src_frame = length, a and d strictly increasing,
 *   N = d_last with N + 8 <= INT32_MAX.  Region i plays [a_i, a_i+1) in [d_i, d_i+1): A and D frames, A <= 4 D and D <= 4 A.  A region
 *   with A != D is stretched with section 8's overlap O of the rate and section 8's sequence S and seek window W of tau = A / D:
 *   L = S - O, nseg = ceil(D / L), room = A - L - (W - 1) >= 0, S > O, W >= 1, W + O <= 4608.  A region with A = D is copied.  Anything
 *   else is ZLHIP_ERR_INVALID, as are ids not in use or repeated and count < 0 -- all decided before the first HIP call.  A request
 *   whose every region has A = D is the identity: applied = 0, no error, the clip is left alone.
 *   Segments and output: libzl_amd/csrc/zl_warp.h.  b_0 = a; b_k = a + min(floor(k tau L), room) + off_k with section 8's seek and tie
 *   rule, so no frame a region plays comes from the next one (a hit is never heard twice); the first O frames of every segment but the
 *   clip's first are faded from the continuation of the segment in front of it (zl_st_xfade), across region joins too.
 *   The result: applied, regions, stretched_regions, segments (one seek offset each, zlhip_debug_warp_offsets), length (= N), overlap.
 *   ZL_SOUND_FINITE stays set iff the original had it and every written sample is finite.
 *   A clip that currently plays a re-render is ZLHIP_ERR_STATE; an arena that cannot hold the whole call is ZLHIP_ERR_CAPACITY.  All
 *   or nothing: on any error every clip is as it was and out is not written.  Synchronisation is zlhip_sound_convert_rate's.  A call is
 *   one copy of each of its tables, a seek launch, a synthesis launch, a publishing launch and one wait, whatever the number of requests; a
 *   call whose every request is the identity launches and copies nothing.
 *   Consequences.  The new extent becomes the clip's ORIGINAL: warp first, then tune and level (a later re-render starts from the
 *   warped data).  Clip parameters are seconds of the playback data and keep their meaning; zlhip_warp_map carries a frame across.
 *   Not provided: undo (reload the clip); a variable seek window or anything cleverer than the clamp at a stretched slice's end (far
 *   below tau = 1 the last segments of a slice repeat its tail); band-limiting; warping under a re-render; moving the clip's own start,
 *   length and slices; beat-phase or downbeat detection (origin is the caller's); any change to section 8's kernels. */
#define ZLHIP_WARP_MAX_ANCHORS 4096
typedef struct zlhip_warp_anchor { int32_t src_frame, dst_frame; } zlhip_warp_anchor;
typedef struct zlhip_warp_request { int32_t id, count; const zlhip_warp_anchor *anchors; } zlhip_warp_request;
typedef struct zlhip_warp { int32_t applied, regions, stretched_regions, segments, length, overlap; } zlhip_warp;
/* host only: checks the anchors against a sound of `length` frames at `sample_rate` and fills the summary (applied = 0: the identity) */
int zlhip_warp_resolve(double sample_rate, int32_t length, const zlhip_warp_anchor *anchors, int32_t count, zlhip_warp *summary);
/* host only: from hits to anchors, pure arithmetic in double (zl_warp.h, zl_wp_plan).  scale = src_bpm / dst_bpm,
 * g = rate 60 / (src_bpm steps_per_beat); every onset t (ascending, inside the clip): q = rint((t - origin) / g), target = origin + q g,
 * moved = t + strength (target - t), the anchor (t - P, rint(moved scale) - P) with P = preroll_frames (-1: the rate's overlap O), so
 * that the attack lands on the grid and the join's fade lies in front of it; anchors with src <= 0 are skipped.  Start (0, 0), end
 * (length, max(1, rint(length scale))).  A candidate is kept iff the region from the last kept anchor to it and the region from it to
 * the end are acceptable by zlhip_warp_resolve's rules with the tighter ratio A <= 2 D, D <= 2 A: the result always resolves.
 * *dropped counts the candidates not kept.  strength in [0, 1], steps_per_beat in [1, 64], both bpm > 0 and finite,
 * 0 <= origin_frame < length, an acceptable region start -> end: else ZLHIP_ERR_INVALID; capacity too small: ZLHIP_ERR_CAPACITY */
int zlhip_warp_plan(double sample_rate, int32_t length, const int32_t *onset_frames, int32_t n, double src_bpm, double dst_bpm, int32_t steps_per_beat,
                    double strength, int32_t origin_frame, int32_t preroll_frames, zlhip_warp_anchor *anchors_out, int32_t capacity, int32_t *count, int32_t *dropped);
/* host only: the piecewise-linear image of a source frame under the anchors (floor, 64-bit integers); frames in front of the clip map
 * to 0, frames behind it to d_last; -1 for anchors == NULL or count < 2 */
int64_t zlhip_warp_map(const zlhip_warp_anchor *anchors, int32_t count, int64_t src_frame);
int zlhip_sound_warp(zlhip_engine *e, const zlhip_warp_request *request, zlhip_warp *out);
int zlhip_sound_warp_batch(zlhip_engine *e, const zlhip_warp_request *reqs, int32_t count, zlhip_warp *out);
/* the seek offsets of the clip's last warp, region by region in output order (a copy region has one, 0); out may be NULL to ask for the count */
int zlhip_debug_warp_offsets(zlhip_engine *e, int32_t id, int32_t *out, int32_t capacity, int32_t *count);
/* measurement: device time of the seek launch and of the synthesis and publishing launches of the last call made with profiling on */
int zlhip_debug_warp_timings(zlhip_engine *e, float *seek_ms, float *synth_ms);
/* Key: what key a loop is in (a build-defined extension, the reference has no key detection) -- detected on the
 * device in the sound's CURRENT playback data.  Pitch detection answers "no pitch" on a chord loop by design; this is the answer for
 * those.  Behind section 8's 16-bit quantisation everything the device does is integer arithmetic (libzl_amd/csrc/zl_key.h):
 *   a bank of correlators, one bin per semitone from note_lo to note_hi (MIDI): f = a4_hz 2^((note - 69) / 12), a Hann window of
 *   N = q rate / f samples (even, at most 32768), phases j step mod 2^32 with step = rint(f / rate 2^32) into ONE cosine table of 4096
 *   int16 entries (zlhip_key_design gives the bins and the table).  L = the largest N.  Frames of L samples every `hop` frames, at most
 *   max_frames of them spread over the region; num_frames < L gives none.  A frame whose energy lies under L channels gate^2 is silent.
 *   Per frame and bin re = the sum of v c, im = the sum of v s (int64), e = ((re / N) >> 8)^2 + ((im / N) >> 8)^2, which counts where
 *   e L reaches the frame's energy (-33 dB of a tone of the frame's power; below it is leakage and rounding); the per-bin totals
 *   over the sounding frames fold into the twelve chroma words; tonic (0 = C .. 11 = B), mode (0 major, 1 minor) and confidence are
 *   the best of Pearson's r with the 24 rotations of the Krumhansl-Kessler profiles, second_* the runner-up (a relative or parallel key
 *   close behind is information, not an error).
 *   No key -- no frames, no sounding frame or a constant chroma -- is not an error: tonic = -1 and every other field 0 except frames.
 *   A field given as 0 takes its default (zlhip_key_resolve with the sound's sample rate): a4_hz = 440, note_lo = 36, note_hi = 95,
 *   q = 34, hop = 8192, max_frames = 256, gate = 8.  Limits: a4_hz in [220, 880], 1 <= note_lo <= note_hi <= 127, at most 96 bins,
 *   the top bin below rate / 2 and at least 32 samples long, q <= 256, hop <= 2^24, max_frames <= 256, gate <= 32767; at most 65536
 *   frames in one call.  Anything else is ZLHIP_ERR_INVALID and nothing has been launched.
 *   A call is three launches, whatever the number of requests, and 136 bytes per request to the host. */
typedef struct zlhip_key_request { int32_t id, first_frame, num_frames, hop, max_frames; float a4_hz; int32_t note_lo, note_hi, q, gate; } zlhip_key_request;
typedef struct zlhip_key { int32_t tonic, mode, second_tonic, second_mode, frames, sounding; double confidence, second_confidence;
                           uint64_t chroma[12]; } zlhip_key;
typedef struct zlhip_key_bin { int32_t note, n; uint32_t step, wstep; } zlhip_key_bin;
#define ZLHIP_KEY_TABLE 4096
/* fills the defaults into r and checks the limits that need no sound */
int zlhip_key_resolve(double sample_rate, zlhip_key_request *r);
/* the table of a request at a rate: *nbins bins into bins [capacity] and the cosine table into table [4096] (each may be NULL) */
int zlhip_key_design(double sample_rate, const zlhip_key_request *r, zlhip_key_bin *bins, int32_t capacity, int32_t *nbins, int16_t *table);
/* how many semitones, -6 .. +5, move a clip in (clip_tonic, clip_mode) into (tonic, mode): ((tonic - from + 6) mod 12) - 6, where from
 * is clip_tonic, or the clip's relative key where the modes differ (major: clip_tonic + 9, minor: clip_tonic + 3).  Tonics 0 .. 11,
 * modes 0 / 1; anything else gives 0 */
int zlhip_key_match_shift(int32_t clip_tonic, int32_t clip_mode, int32_t tonic, int32_t mode);
int zlhip_sound_key(zlhip_engine *e, const zlhip_key_request *r, zlhip_key *out);
int zlhip_sound_key_batch(zlhip_engine *e, const zlhip_key_request *reqs, int32_t nreq, zlhip_key *out);
/* the per-bin totals of request `request` of the last call (totals: [capacity], may be NULL to ask for the count only) */
int zlhip_debug_key_bins(zlhip_engine *e, int32_t request, uint64_t *totals, int32_t capacity, int32_t *bins);
/* re and im of every bin of frame `frame` of request `request` of the last call (a silent frame's are 0); *frames: the request's frames */
int zlhip_debug_key_frame(zlhip_engine *e, int32_t request, int32_t frame, int64_t *re, int64_t *im, int32_t capacity, int32_t *bins, int32_t *frames);
/* measurement: device time of the three launches of the last call made with profiling on */
int zlhip_debug_key_timings(zlhip_engine *e, float *gate_ms, float *correlate_ms, float *fold_ms);
/* Clips from raw PCM.  `frames` is host memory, pageable or page-locked: `length` frames of `channels`
 *   interleaved little-endian samples, exactly the bytes of a WAV `data` chunk.  They are copied raw into a device staging buffer and
 *   decoded there into the arena's layout; one decode launch serves each staging pass and the call waits for the device once.
 *   The first min(2, channels) channels are kept; the sound is mono only when channels == 1.
 *   Integer formats widen to left-justified int32 (U8: (b - 128) << 24, S16: << 16, S24: three bytes << 8), convert to float with
 *   round-to-nearest-even and multiply by 2^-31.  F32 is moved as 32 bits (a signalling NaN, -0 and denormals keep their bits).
 *   F64 is (float)d, round-to-nearest-even: denormal results stay denormal, overflow gives +-inf, a NaN a NaN of the same sign.
 *   All or nothing: every argument of every source is checked before the first HIP call -- frames NULL, a format outside 1..6,
 *   channels outside 1..ZLHIP_PCM_MAX_CHANNELS, length < 1, sample_rate <= 0, reserved != 0, count < 0 are ZLHIP_ERR_INVALID -- and
 *   too few free sound slots or an arena that cannot hold the whole call (it may grow under sound_arena_max_bytes) are
 *   ZLHIP_ERR_CAPACITY, decided before any copy; either way no slot is taken, no extent kept and every out_ids[i] is -1.
 *   count == 0 is ZLHIP_OK.  On success the ids are the first free slots in request order, as `count` consecutive zlhip_sound_upload
 *   calls would have given, every clip with its default clip parameters.  Synchronisation is zlhip_sound_upload's: the resident
 *   kernel leaves, queued batches finish first, the call is synchronous.
 *   The staging buffer (ZL_PCM_STAGE_BYTES, read per call; default 64 MiB, at least 4096, a multiple of 16) is allocated by the
 *   first PCM call, only grows, and is counted in zlhip_memory_bytes. */
enum { ZLHIP_PCM_U8 = 1, ZLHIP_PCM_S16 = 2, ZLHIP_PCM_S24 = 3, ZLHIP_PCM_S32 = 4, ZLHIP_PCM_F32 = 5, ZLHIP_PCM_F64 = 6 };
#define ZLHIP_PCM_MAX_CHANNELS 64
typedef struct zlhip_pcm_source { const void *frames; int32_t length, channels, format, reserved; double sample_rate; } zlhip_pcm_source;
int zlhip_sound_upload_pcm(zlhip_engine *e, const void *frames, int32_t format, int32_t channels, int32_t length, double sample_rate, int32_t *out_id);
int zlhip_sound_upload_pcm_batch(zlhip_engine *e, const zlhip_pcm_source *srcs, int32_t count, int32_t *out_ids);
/* measurement: device time of the copies into the stage and of the decode launches of the last PCM upload call made with profiling on
 * (zlhip_set_profiling; HIP events on the engine's stream) */
int zlhip_debug_upload_pcm_timings(zlhip_engine *e, float *copy_ms, float *decode_ms);
/* debug: the seek offsets off_k of the sound's last render, one per stretch segment (*count = 0: the stretch did not run) */
int zlhip_debug_rerender_offsets(zlhip_engine *e, int32_t id, int32_t *out, int32_t capacity, int32_t *count);
/* measurement: device time of the seek launch and of the synthesis launch of the last re-render call made with profiling on
 * (zlhip_set_profiling; HIP events on the engine's stream) */
int zlhip_debug_rerender_timings(zlhip_engine *e, float *seek_ms, float *synth_ms);
/* Sample-rate conversion: a clip whose rate differs from the engine's plays through the pitched voice path
 *   (an fp64 position per frame, two taps, no anti-alias filter); converted to the engine's rate it is a unit-step source and takes
 *   the on-grid path.  The conversion is build-defined -- the reference resamples while it plays (SamplerSynthVoice.cpp:104), so a
 *   converted clip no longer reproduces the reference's bits for that file -- and therefore opt-in: nothing converts unless asked.
 *   Definition: rates are integer-valued, in [1000, 768000]; g = gcd(fs, ft), L = ft / g, M = fs / g.  A Kaiser-windowed sinc
 *   (beta 10, cutoff 0.95 of the lower Nyquist, 32 / min(1, L/M) input frames a side), one row per phase, rows of unit sum, fp32;
 *   the clip gets N = ceil(length * L / M) frames, each the sum of its taps in fp32 -- a rounded multiply, then a rounded add, in tap
 *   order, samples outside the clip +0.  Mono stays mono.  ZL_SOUND_FINITE is decided on the device from the output.
 *   Limits: L <= 2048, M <= 8 L, L * (taps rounded up to 4) <= 262144, N + 8 <= INT32_MAX: anything else is ZLHIP_ERR_INVALID,
 *   as are ids not in use or repeated and count < 0 -- all decided before the first HIP call.  target_rate == 0 means the engine's
 *   playback_sample_rate.  A clip that currently plays a re-render is ZLHIP_ERR_STATE (re-render it with gain 0, pitch 0, speed 1
 *   first); an arena that cannot hold the whole call is ZLHIP_ERR_CAPACITY.  All or nothing: on any error every clip is as it was.
 *   A clip already at the target rate is skipped (no launch, no copy), whatever that rate is.
 *   The converted extent becomes the clip's ORIGINAL: later re-renders start from it, the old original goes back to the arena.
 *   Synchronisation is zlhip_sound_rerender's: the resident kernel leaves, queued batches finish, the table entry switches at a block
 *   boundary; one launch converts every clip of the call, one publishes, and the call waits once.
 *   Side effects: the sound's sample rate changes, so a note started later steps at the new rate.  Clip parameters are seconds and
 *   keep their meaning; duration_seconds stays.  A voice that plays the clip DURING the call keeps its frame position and step: that is
 *   safe (as after a re-render that shortens the clip) but musically wrong -- convert before playing.
 *   The filter tables live on the device, one per (L, M) ever asked for, until the engine is destroyed; zlhip_memory_bytes counts them.
 *   A table is made by the first call that asks for its ratio; a call that fails frees the tables it added. */
int zlhip_sound_convert_rate(zlhip_engine *e, int32_t id, double target_rate);
int zlhip_sound_convert_rate_batch(zlhip_engine *e, const int32_t *ids, int32_t count, double target_rate);
/* The filter of a ratio, on the host (no engine, no device): *L, *M, *taps and *row_floats (taps rounded up to a multiple of 4) and,
 * where table != NULL, the L rows of row_floats floats (zeros in the pad).  table == NULL asks for the sizes only; table_floats below
 * L * row_floats is ZLHIP_ERR_CAPACITY, a ratio beyond the limits ZLHIP_ERR_INVALID.  The engine builds its device tables with this code. */
int zlhip_resample_design(double source_rate, double target_rate, int32_t *L, int32_t *M, int32_t *taps, int32_t *row_floats,
                          float *table, size_t table_floats);
/* What a sound slot plays now: frames, channels, rate; finite = ZL_SOUND_FINITE is set; rendered = it plays a re-render. */
typedef struct zlhip_sound_info { int32_t length, channels; double sample_rate; int32_t finite, rendered; } zlhip_sound_info;
int zlhip_sound_info_get(zlhip_engine *e, int32_t id, zlhip_sound_info *out);
/* debug: the sound's playback extent as it lies in the arena -- interleaved (or mono), the 8 zero frames behind the last frame and the
 * floats up to the 16-byte boundary included.  *floats receives the extent's size; out == NULL asks for the size only; capacity below it
 * is ZLHIP_ERR_CAPACITY.  Synchronisation is zlhip_sound_read's. */
int zlhip_debug_sound_extent(zlhip_engine *e, int32_t id, float *out, size_t capacity, size_t *floats);
/* measurement: device time of the last conversion call made with profiling on (HIP events around the call's two launches) */
int zlhip_debug_convert_timings(zlhip_engine *e, float *device_ms);

/* ---- commands ------------------------------------------------------------------------------ */
void zlhip_clip_command_clear(zlhip_clip_command *c);           /* ClipCommand.h:74-91 */
/* SamplerChannel::handleCommand for the bus whose midi channel matches (bus b has midi channel
 * b - 2, SamplerSynth.cpp:270).  Returns 1 if a voice took / merged the command, 0 if it was
 * dropped (no free voice, as in the reference), < 0 on error. */
int zlhip_handle_command(zlhip_engine *e, const zlhip_clip_command *cmd, uint64_t current_tick);
/* A block's worth of commands in one call (SyncTimer dispatches every command that is due in a cycle,
 * SyncTimer.cpp:553-558): handled in array order like the channel's command ring; they reach the device as ONE
 * voice-table update (K0) before the next rendered block.  taken[i] (optional) receives what zlhip_handle_command
 * would have returned for command i; the return value is their sum, < 0 on error. */
int zlhip_handle_commands(zlhip_engine *e, const zlhip_clip_command *cmds, int32_t count, uint64_t current_tick, int32_t *taken);
/* The same, and voices[i] (optional) receives the voice -- bus * voices_per_bus + slot, the index of zlhip_voice_reports -- that
 * command i STARTED (startNote, SamplerSynthVoice.cpp:110-144), -1 if it started none.  For a host that keeps per-voice state of its own
 * in the order the reference creates it (the libzl layer's playback-positions rows: created in command order at dispatch, :129). */
int zlhip_handle_commands_voices(zlhip_engine *e, const zlhip_clip_command *cmds, int32_t count, uint64_t current_tick, int32_t *taken, int32_t *voices);
/* SamplerSynth::setChannelEnabled(channel, enabled) for bus = channel + 2 (SamplerSynth.cpp:343-351; SamplerChannel::process :116-123): a
 * disabled bus still takes its commands, but its voices are not processed -- they keep position, envelope and clock state and go on
 * from there when the bus is enabled again -- and report no progress.  The bus renders silence meanwhile (the reference leaves its JACK
 * port buffers untouched).  Host-only, takes effect with the next rendered block. */
int zlhip_bus_set_enabled(zlhip_engine *e, int32_t bus, int enabled);
/* Same, addressed to an explicit voice slot of a bus (bypasses first-free allocation; used to
 * build large synthetic scenes deterministically). */
int zlhip_start_voice(zlhip_engine *e, int32_t bus, int32_t slot, const zlhip_clip_command *cmd, uint64_t current_tick);
/* The voice-level calls behind the JUCE SynthesiserVoice surface of SamplerSynthVoice (include/zlhip_voice_adapter.h):
 * stopNote(velocity, allowTailOff) (SamplerSynthVoice.cpp:146-169), setCurrentCommand on a playing voice (:58-93) and
 * the isPlaying flag (SamplerSynthVoice.h:31).  They apply before the next rendered block.  Return 1 / 0 (the voice
 * was playing / was not), < 0 on error. */
int zlhip_stop_voice(zlhip_engine *e, int32_t bus, int32_t slot, int allow_tail_off);
int zlhip_update_voice(zlhip_engine *e, int32_t bus, int32_t slot, const zlhip_clip_command *cmd);
int zlhip_voice_is_playing(zlhip_engine *e, int32_t bus, int32_t slot);

/* ---- render -------------------------------------------------------------------------------- */
/* One real-time block: renders nframes for every bus and delivers the mix to host memory.
 * out_left/out_right: [num_buses][nframes] each (host).  Synchronous.
 * Page-locked buffers (zlhip_host_alloc, or the caller's own hipHostMalloc / hipHostRegister -- e.g. of its JACK port area) are written by
 * the kernels DIRECTLY: no copy on the host behind the cycle (1.6 us for 12 buses x 256 frames; 5 us more with the fan-out's 72 KB).
 * Any other memory is served through the engine's staging rows and a copy.  (ZL_RT_DIRECT_OUT=0: always staged.) */
int zlhip_render(zlhip_engine *e, int32_t nframes, const zlhip_clock *clock, float *out_left, float *out_right);
/* The same cycle, and the JackPassthrough client behind every bus with it (JackPassthroughPrivate::process, JackPassthrough.cpp:45-115;
 * the client is the next node after a SamplerSynth channel in the reference's JACK graph): the three output pairs of every bus are
 * computed from the registers that hold the finished mix and written to host memory next to it -- by the resident real-time kernel
 * where zlhip_render uses it, else by the launched kernels.
 *   fan_params  host [num_buses]: this cycle's dry / wetFx1 / wetFx2 / pan amounts and mute flags.  Taken per cycle: a changed value
 *               costs no HIP call and does not disturb the resident kernel (it re-reads the table when it differs from the last cycle's)
 *   fan_out     host [num_buses][6][nframes] = dryL, dryR, fx1L, fx1R, fx2L, fx2R of every bus (the order of zlhip_passthrough_process)
 * Bit-identical to zlhip_render followed by the passthrough of its output.  fan_params == fan_out == NULL: zlhip_render. */
int zlhip_render_fanout(zlhip_engine *e, int32_t nframes, const zlhip_clock *clock, float *out_left, float *out_right,
                        const zlhip_passthrough_params *fan_params, float *fan_out);
/* Throughput mode: nblocks consecutive blocks in one pass.  clocks: host [nblocks].
 * bus_out_dev: DEVICE buffer laid out [num_buses][2][nblocks*nframes] fp32, or NULL to use the
 * engine's internal buffer (readable with zlhip_read_bus).  stream: hipStream_t or NULL for the
 * engine's own stream.  Asynchronous; zlhip_synchronize waits. */
int zlhip_render_batch(zlhip_engine *e, int32_t nblocks, int32_t nframes, const zlhip_clock *clocks,
                       float *bus_out_dev, void *stream);
int zlhip_synchronize(zlhip_engine *e);
/* copy the internal bus buffer of the last batch to host: out [num_buses][2][nblocks*nframes] */
int zlhip_read_bus(zlhip_engine *e, float *out, size_t out_floats);
/* per-voice reports of the last rendered block: out [num_buses*voices_per_bus] */
int zlhip_voice_reports(zlhip_engine *e, zlhip_voice_report *out, int32_t count);
/* debug: per-frame (int)sourceSamplePosition of every voice for the blocks of the NEXT batches,
 * kept on device and read back with zlhip_debug_read_trace: out [nblocks][voices][nframes] int32 */
int zlhip_debug_enable_trace(zlhip_engine *e, int enable);   /* bit 0: trace; bits 1, 2: planner test hooks */
int zlhip_debug_read_trace(zlhip_engine *e, int32_t *out, size_t out_ints);
/* debug: the HIP resources the process's engines hold at this moment -- counts[0..3] = device buffers, page-locked host buffers,
 * events, streams.  Process-wide, no engine: whatever an engine took while it lived, its destruction gives back (a host asserting
 * a clean shutdown reads the same four numbers before its first engine and after its last).  Not counted: the arena's later
 * segments, memory from zlhip_host_alloc, an engine group's own events. */
int zlhip_debug_live_resources(int32_t counts[4]);

/* ---- levels -------------------------------------------------------------------------------- */
/* One AudioLevels timer tick for every bus over block `block_index` of the last batch
 * (-1 = the last block; the reference only ever sees the most recent block, AudioLevels.cpp:361-384).
 * out: [num_buses].  with_hold_bus: index of the bus that keeps the 0.9x hold (reference:
 * channel index 1, AudioLevels.cpp:391-398), -1 for none. */
int zlhip_levels_tick(zlhip_engine *e, int32_t block_index, int32_t with_hold_bus, zlhip_levels *out);
/* raw per-block integer peaks of the last batch: out [nblocks][num_buses][2] */
int zlhip_block_peaks(zlhip_engine *e, int32_t *out, size_t out_ints);
/* levels of an arbitrary DEVICE bus buffer [num_buses][2][nblocks*nframes] (e.g. the result of a
 * multi-GPU reduce): recomputes the per-block peaks the next zlhip_levels_tick will use */
int zlhip_levels_scan_device(zlhip_engine *e, const float *bus_dev, int32_t nblocks, int32_t nframes, void *stream);

/* ---- multi-GPU exchange (a bus that spans GPUs) ----------------------------------------------------
 * The only coupling between voices is the per-bus sum of SamplerChannel::process (SamplerSynth.cpp:134-140).  When the
 * voices of a bus live on several GPUs, every rank renders a partial bus [num_buses][2][nblocks*nframes] and the ranks
 * exchange it piecewise (all-to-all over the xGMI mesh: rank r receives piece r of every rank's partial bus; the transport is
 * the host's, e.g. RCCL).  A piece is a run of whole UNITS, unit u = (bus * 2 + channel) * nblocks + block = nframes
 * consecutive floats of the bus buffer.
 *
 * zlhip_bus_reduce_sum_scan: one kernel, run by every rank on the pieces it received.  Sums them in piece (= rank) order,
 * ((0 + p0) + p1) + ... per sample -- deterministic, the same bits for any number of ranks, and equal to the single-GPU
 * result with voices_per_task = voices per rank -- writes the reduced piece and, in the same pass, the AudioLevels scan of
 * every unit (integer peak, AudioLevels.cpp:361-383; sum of squares of the RMS extension).
 *   pieces_dev      DEVICE [npieces] pieces of units * nframes floats, piece_stride_floats apart (the all-to-all receive buffer)
 *   sum_out_dev     DEVICE [units * nframes]
 *   levels_out_dev  DEVICE [units]
 * zlhip_levels_import_units: on the rank that meters (the root, after gathering the unit levels of all pieces in unit order
 * [num_buses * 2 * nblocks]): makes them the block levels the next zlhip_levels_tick / zlhip_block_peaks read. */
typedef struct zlhip_unit_levels { int32_t peak; float sumsq; } zlhip_unit_levels;
int zlhip_bus_reduce_sum_scan(zlhip_engine *e, const float *pieces_dev, int32_t npieces, int64_t piece_stride_floats, int64_t units,
                              int32_t nframes, float *sum_out_dev, zlhip_unit_levels *levels_out_dev, void *stream);
int zlhip_levels_import_units(zlhip_engine *e, const zlhip_unit_levels *units_dev, int32_t nblocks, int32_t nframes, void *stream);

/* ---- engine group: one synth over several GPUs in one process (ABI 3, additive) --------------------------------------------
 * A group is n engines ("members", n in 1..ZLHIP_GROUP_MAX_MEMBERS), one per listed device, driven as ONE synth with the buses and
 * voices of one zlhip_config.  Devices may repeat: [0, 0] is a valid group on one GPU.  zlhip_group_create enables peer access for
 * every ordered pair of distinct devices (tolerating "already enabled"); a pair that cannot reach each other fails creation.
 * Every argument check happens before the first HIP call; without a device the call returns ZLHIP_ERR_NO_DEVICE and *out stays NULL
 * (zlhip_group_last_error(NULL) then tells why the last creation on this thread failed).
 *
 * Two partitions (the two of the Python ranks, libzl_amd/sharding.py):
 *   ZLHIP_GROUP_BUS_ALIGNED (needs num_buses >= n): member r owns the global buses g with (g * n) / num_buses == r -- contiguous,
 *     as its local buses 0.. with the global voices_per_bus and voices_per_task.  Buses never interact, so the output is bit-identical
 *     to one engine with the whole config; nothing crosses devices.  bus_out_dev of zlhip_group_render_batch must be NULL.
 *   ZLHIP_GROUP_SPAN (needs voices_per_bus % n == 0 and voices_per_task 0 or voices_per_bus / n): every member has all buses with
 *     voices_per_bus / n voices; member r holds the global slots [r * VPB / n, (r + 1) * VPB / n) of every bus and renders them into
 *     a partial bus.  The bus is summed per sample IN RANK ORDER, ((0 + p0) + p1) + ... -- bit-identical to one engine with
 *     voices_per_task = VPB / n (the reference's voice order inside a member, the mix-group order across members).  The sum is one
 *     kernel per member over 1/n of the (block, bus) pairs, which reads every member's partial (the others' over xGMI) and writes the
 *     root's bus and the root's meters; the root's stream waits for it, and every member's next render waits for every sum of the call
 *     before.  The group's levels and peaks are the root's.
 *   ZLHIP_GROUP_AUTO: bus-aligned when num_buses >= n, else span.
 * Numbers at this surface are GLOBAL: buses, slots, voices (bus * voices_per_bus + slot) and midi channels (bus g has channel g - 2).
 * Commands of a spanning bus follow SamplerChannel::handleCommand over the bus's voices in global slot order: a stop or an update goes
 * to every member, a start to the first member with a free voice in its slice (a stop + start: the members before it apply the stop,
 * the one that takes it applies both, the ones after it the stop); taken / voices are what one engine would report.
 * Sounds and clips are broadcast: every member holds every clip (any bus may play any clip), so the group's source HBM is n x one
 * engine's; ids agree across members.
 * zlhip_group_member: the borrowed engine of member r, for read-only and measurement calls (zlhip_last_timings, zlhip_memory_bytes,
 * zlhip_device_name ...).  Commands, sounds and renders go through the group: a member driven directly leaves the group undefined. */
#define ZLHIP_GROUP_MAX_MEMBERS 8
enum { ZLHIP_GROUP_AUTO = 0, ZLHIP_GROUP_BUS_ALIGNED = 1, ZLHIP_GROUP_SPAN = 2 };
typedef struct zlhip_group zlhip_group;
typedef struct zlhip_group_config {
    uint32_t struct_size;            /* sizeof(zlhip_group_config) */
    int32_t  partition;              /* ZLHIP_GROUP_* */
    int32_t  root;                   /* span: the member that holds the summed bus and the meters (default 0) */
    int32_t  reserved;               /* 0 */
} zlhip_group_config;
void zlhip_group_config_default(zlhip_group_config *gc);
/* cfg describes the WHOLE synth (global num_buses, voices_per_bus ...); cfg->device is ignored */
int  zlhip_group_create(const int32_t *devices, int32_t n, const zlhip_config *cfg, const zlhip_group_config *gc, zlhip_group **out);
void zlhip_group_destroy(zlhip_group *g);
const char *zlhip_group_last_error(const zlhip_group *g);
/* per member [n] each: its partition, first global bus and number of buses, first global slot and number of slots of each bus */
int  zlhip_group_layout(zlhip_group *g, int32_t *partition, int32_t *first_bus, int32_t *num_buses, int32_t *first_slot, int32_t *slots);
zlhip_engine *zlhip_group_member(zlhip_group *g, int32_t r);
int  zlhip_group_sound_upload(zlhip_group *g, const float *left, const float *right, int32_t length, double sample_rate, int32_t *out_id);
/* zlhip_sound_upload_pcm_batch on every member (broadcast): the ids agree; a failure on one member undoes the others */
int  zlhip_group_sound_upload_pcm_batch(zlhip_group *g, const zlhip_pcm_source *srcs, int32_t count, int32_t *out_ids);
int  zlhip_group_sound_release(zlhip_group *g, int32_t id);
int  zlhip_group_clip_set(zlhip_group *g, int32_t id, const zlhip_clip_params *p);
int  zlhip_group_sound_rerender_batch(zlhip_group *g, const int32_t *ids, const zlhip_rerender_params *params, int32_t count);
/* zlhip_sound_convert_rate_batch on every member, in member order.  The members hold the same clips in arenas that are alike, so a call
 * that is invalid, refused or does not fit fails on member 0 and changes nothing.  A failure on a later member (a HIP error) converts
 * nothing back: the members before it hold the converted clips, it and the ones behind it the old ones; the error names the member. */
int  zlhip_group_sound_convert_rate_batch(zlhip_group *g, const int32_t *ids, int32_t count, double target_rate);
/* zlhip_sound_overview / _batch: every member holds every sound, member 0 answers */
int  zlhip_group_sound_overview(zlhip_group *g, int32_t id, int32_t first_frame, int32_t num_frames, int32_t columns, float *out);
int  zlhip_group_sound_overview_batch(zlhip_group *g, const zlhip_overview_request *reqs, int32_t count, float *out, size_t out_floats);
/* zlhip_sound_onsets_batch: member 0 answers */
int  zlhip_group_sound_onsets_batch(zlhip_group *g, const zlhip_onset_request *reqs, int32_t nreq, zlhip_onset *out, size_t capacity, int32_t *counts);
/* zlhip_sound_tempo_batch: member 0 answers */
int  zlhip_group_sound_tempo_batch(zlhip_group *g, const zlhip_tempo_request *reqs, int32_t nreq, zlhip_tempo *out);
/* zlhip_sound_pitch_batch: member 0 answers */
int  zlhip_group_sound_pitch_batch(zlhip_group *g, const zlhip_pitch_request *reqs, int32_t nreq, zlhip_pitch *out);
/* zlhip_sound_loudness_batch: member 0 answers */
int  zlhip_group_sound_loudness_batch(zlhip_group *g, const zlhip_loudness_request *reqs, int32_t nreq, zlhip_loudness *out);
/* zlhip_sound_loop_batch: member 0 answers */
int  zlhip_group_sound_loop_batch(zlhip_group *g, const zlhip_loop_request *reqs, int32_t nreq, zlhip_loop *out);
/* zlhip_sound_loop_crossfade_batch on every member, in member order, with zlhip_group_sound_convert_rate_batch's semantics: a call
 * that is invalid, refused or does not fit fails on member 0 and changes nothing.  out receives member 0's results (the members hold
 * the same data: every member measures the same integers) */
int  zlhip_group_sound_loop_crossfade_batch(zlhip_group *g, const zlhip_xfade_request *reqs, int32_t count, zlhip_xfade *out);
/* zlhip_sound_edit_batch on every member, in member order, with zlhip_group_sound_convert_rate_batch's semantics; out receives member
 * 0's results (the members hold the same data: every member finds the same frames) */
int  zlhip_group_sound_edit_batch(zlhip_group *g, const zlhip_edit_request *reqs, int32_t count, zlhip_edit *out);
/* zlhip_sound_peak_batch: member 0 answers */
int  zlhip_group_sound_peak_batch(zlhip_group *g, const zlhip_peak_request *reqs, int32_t nreq, zlhip_peak *out);
/* zlhip_sound_limit_batch on every member, in member order, with zlhip_group_sound_convert_rate_batch's semantics; out receives member
 * 0's results (the members hold the same data: every member computes the same gains) */
int  zlhip_group_sound_limit_batch(zlhip_group *g, const zlhip_limit_request *reqs, int32_t count, zlhip_limit *out);
/* zlhip_sound_warp_batch on every member, in member order, with zlhip_group_sound_convert_rate_batch's semantics; out receives member
 * 0's results (the members hold the same data: every member finds the same offsets) */
int  zlhip_group_sound_warp_batch(zlhip_group *g, const zlhip_warp_request *reqs, int32_t count, zlhip_warp *out);
/* zlhip_sound_key_batch: member 0 answers */
int  zlhip_group_sound_key_batch(zlhip_group *g, const zlhip_key_request *reqs, int32_t nreq, zlhip_key *out);
/* zlhip_handle_commands_voices over the whole synth (taken, voices optional) */
int  zlhip_group_handle_commands(zlhip_group *g, const zlhip_clip_command *cmds, int32_t count, uint64_t current_tick, int32_t *taken,
                                 int32_t *voices);
int  zlhip_group_start_voice(zlhip_group *g, int32_t bus, int32_t slot, const zlhip_clip_command *cmd, uint64_t current_tick);
int  zlhip_group_stop_voice(zlhip_group *g, int32_t bus, int32_t slot, int allow_tail_off);
int  zlhip_group_update_voice(zlhip_group *g, int32_t bus, int32_t slot, const zlhip_clip_command *cmd);
int  zlhip_group_voice_is_playing(zlhip_group *g, int32_t bus, int32_t slot);
int  zlhip_group_bus_set_enabled(zlhip_group *g, int32_t bus, int enabled);
/* Asynchronous, like zlhip_render_batch.  bus_out_dev: span only, optional, a DEVICE buffer on the root's device laid out
 * [num_buses][2][nblocks*nframes] (NULL: the root's internal buffer, read with zlhip_group_read_bus); bus-aligned: must be NULL. */
int  zlhip_group_render_batch(zlhip_group *g, int32_t nblocks, int32_t nframes, const zlhip_clock *clocks, float *bus_out_dev);
int  zlhip_group_synchronize(zlhip_group *g);
int  zlhip_group_read_bus(zlhip_group *g, float *out, size_t out_floats);               /* [num_buses][2][nblocks*nframes] */
int  zlhip_group_voice_reports(zlhip_group *g, zlhip_voice_report *out, int32_t count);  /* [num_buses*voices_per_bus] */
int  zlhip_group_levels_tick(zlhip_group *g, int32_t block_index, int32_t with_hold_bus, zlhip_levels *out);   /* [num_buses] */
int  zlhip_group_block_peaks(zlhip_group *g, int32_t *out, size_t out_ints);           /* [nblocks][num_buses][2] */

/* ---- JackPassthrough fan-out ---------------------------------------------------------------- */
void zlhip_passthrough_params_default(zlhip_passthrough_params *p);
/* in_dev: [num_buses][2][frames]; out_dev: [num_buses][6][frames] = dryL,dryR,fx1L,fx1R,fx2L,fx2R.
 * params: host [num_buses]. */
int zlhip_passthrough_process(zlhip_engine *e, const zlhip_passthrough_params *params, const float *in_dev,
                              float *out_dev, int64_t frames, void *stream);

/* zlhip_render_batch with the fan-out (JackPassthroughPrivate::process, JackPassthrough.cpp:45-115) fused into the bus
 * write: the JackPassthrough client is the next node after a
 * SamplerSynth bus in the reference's graph, and its three output pairs are computed from the registers that hold the
 * finished mix (24 more bytes written per bus frame, no second pass over the bus).  fan_params: host [num_buses];
 * fan_out_dev: DEVICE [num_buses][6][nblocks*nframes] in the order of zlhip_passthrough_process.  Bit-identical to
 * zlhip_render_batch followed by zlhip_passthrough_process.  Both NULL = zlhip_render_batch. */
int zlhip_render_batch_fanout(zlhip_engine *e, int32_t nblocks, int32_t nframes, const zlhip_clock *clocks,
                              float *bus_out_dev, const zlhip_passthrough_params *fan_params, float *fan_out_dev,
                              void *stream);

/* ---- offline bounce (BASELINE configs[4]; the recorder side of the bus, AudioLevels.cpp:35-119) ----------------------------
 * Renders nblocks consecutive blocks exactly like consecutive zlhip_render_batch calls (voice state, levels and reports carry on;
 * afterwards zlhip_levels_tick / zlhip_block_peaks / zlhip_voice_reports see the last chunk) and delivers every bus to HOST memory.
 * The bounce is cut into chunks of sub_blocks blocks (0 = max_batch_blocks, the longest call the engine takes), each ONE render call
 * whose plan windows pipeline as in a device-resident batch; every window is handed to the copy engine as soon as its render kernel
 * has finished (16-bit: converted first), so PCIe runs next to the rendering of the following windows.  Synchronous.
 *   clocks    host [nblocks]
 *   host_out  ZLHIP_BOUNCE_F32_PLANAR:  float   [num_buses][2][nblocks*nframes]     (the layout of zlhip_render_batch)
 *             ZLHIP_BOUNCE_PCM16_STEREO: int16_t [num_buses][nblocks*nframes][2]     (the data chunk of one 16-bit stereo WAV per
 *             bus, converted on the GPU as the reference's recorder converts -- juce::WavAudioFormat 16 bit, AudioLevels.cpp:53-58;
 *             restated, JUCE version unpinned: clamp, x 0x7fffffff in double, round to nearest even, upper 16 bits; half the PCIe bytes)
 *             Page-locked memory (zlhip_host_alloc, or the caller's hipHostMalloc / hipHostRegister) gives the full PCIe rate;
 *             pageable memory works through the runtime's staging copies.
 * zlhip_host_alloc / zlhip_host_free: page-locked host memory for callers that do not link HIP. */
enum { ZLHIP_BOUNCE_F32_PLANAR = 0, ZLHIP_BOUNCE_PCM16_STEREO = 1 };
int  zlhip_bounce(zlhip_engine *e, int64_t nblocks, int32_t nframes, const zlhip_clock *clocks, void *host_out, int32_t format,
                  int32_t sub_blocks);
int  zlhip_host_alloc(size_t bytes, void **out);
void zlhip_host_free(void *p);

/* ---- introspection / measurement ------------------------------------------------------------ */
int zlhip_set_profiling(zlhip_engine *e, int enable);
int zlhip_last_timings(zlhip_engine *e, zlhip_timings *out);
/* Sums of the timings of every profiled zlhip_render_batch call since the last reset (and their number): lets a caller
 * queue calls back to back -- consecutive calls pipeline, the planning of call i+1 overlaps the rendering of call i --
 * and read the kernel times once at the end.  Waits for outstanding calls. */
int zlhip_profile_totals(zlhip_engine *e, zlhip_timings *totals, int32_t *calls, int reset);
float *zlhip_bus_device_ptr(zlhip_engine *e);                   /* internal [B][2][Kmax*Nmax] buffer */
/* the resident real-time kernel behind zlhip_render: how many times it was launched, how many cycles it rendered (a parameter edit,
 * a command or a quiet spell shorter than the idle timeout do not relaunch it; a batch, an upload or a block-size change do) */
int zlhip_rt_stats(zlhip_engine *e, uint64_t *kernel_starts, uint64_t *cycles_rendered);
/* Is this engine's resident kernel on the device right now (*resident), and which share of the device's resident-workgroup capacity
 * does it take (*share, 0..1)?  The resident kernels of ALL engines of a process together take at most three quarters of a device; an
 * engine that does not fit next to the others renders its cycles with launches (same results) until there is room. */
int zlhip_rt_residency(zlhip_engine *e, int32_t *resident, double *share);
/* HBM the engine allocated at creation: everything (source arena, voice / plan records, control pool, bus, levels) and the
 * arena's share of it */
/* Where the LAST zlhip_render / zlhip_render_fanout cycle spent its time, seen from the calling thread (engines created with ZL_RT_TRACE=1
 * in the environment; ZL_RT_TRACE_SLOW_US=<n> also reports every cycle longer than n microseconds on stderr).  total = before_post (command
 * upload, a restart of the resident kernel; for launches: the launch calls) + wait (for the device) + after (copies into the caller's
 * buffers).  max_poll_gap_us: the longest time between two polls of the waiting thread -- a gap of milliseconds means the THREAD was
 * off its core (scheduler, cgroup quota), not that the device was late; involuntary_switches: getrusage(RUSAGE_THREAD) over the cycle;
 * device_us: the resident kernel's own stage times for the cycle (with ZL_RT_STAMPS=1, else 0). */
typedef struct zlhip_rt_cycle_trace {
    uint64_t cycle;
    int32_t  resident, reserved;
    double   total_us, before_post_us, wait_us, after_us, max_poll_gap_us, device_us;
    int64_t  involuntary_switches;
} zlhip_rt_cycle_trace;
int zlhip_rt_last_cycle(zlhip_engine *e, zlhip_rt_cycle_trace *out);
int zlhip_memory_bytes(zlhip_engine *e, uint64_t *total_device_bytes, uint64_t *arena_bytes);
int zlhip_device_name(zlhip_engine *e, char *buf, size_t len);

#ifdef __cplusplus
}
#endif
#endif
