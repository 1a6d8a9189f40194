/*
 * libzl_hotpath.h -- the libzl.h-named entry points of the hot path, served by the MI355X engine.
 *
 * Same unmangled symbol names, argument orders and (absent) error behaviour as the reference's
 * extern "C" block (/root/reference/lib/libzl.h:18-179, implemented in lib/libzl.cpp:107-575), for
 * the functions that feed or read the sampler hot path.  A host that drives libzl through ctypes
 * (reference test/playtest.py:25-49) binds these exactly as before; handles stay opaque pointers.
 * Functions of libzl.h that belong to out-of-scope subsystems (SyncTimer scheduling, MIDI routing,
 * WAV recording, QML registration) are NOT declared here; see INTEGRATION.md for how they keep
 * linking against the unchanged reference objects.
 *
 * Differences that are visible at this boundary:
 *   - ClipAudioSource_new decodes RIFF/WAVE itself (PCM 8/16/24/32, float32/64; first two channels,
 *     as SamplerSynthSound.cpp:45) instead of going through JUCE / tracktion: the file's `data` chunk goes to the engine as raw PCM
 *     and is decoded on the device (zlhip_sound_upload_pcm); ZL_PCM_DECODE=0, read per call, decodes on the host as before.
 *   - audio is pulled with libzl_hotpath_process() by whoever owns the JACK callback (the reference's
 *     SamplerChannel::process, SamplerSynth.cpp:116-148) instead of being pushed to JACK from inside.
 *   - ClipAudioSource_play/stop go through SyncTimer::scheduleClipCommand with delay 0 as in the reference
 *     (ClipAudioSource.cpp:428,437; SyncTimer.cpp:1011-1048): equivalent commands that meet in one step are merged, and
 *     a command reaches the sampler with the playhead of the step it is dispatched in (SyncTimer.cpp:553-558).  Two ways
 *     to run the cycle: libzl_hotpath_process (the host's own SyncTimer owns the transport and hands its getters over in
 *     zlhip_clock) and libzl_hotpath_cycle (this library runs the step ring itself, SyncTimer.cpp:452-702).
 *   - threading: setters, play / stop / queue calls and getters never take a lock the cycle holds (they publish a
 *     snapshot or post a request that the next cycle picks up); clip creation / destruction, initJuce / shutdownJuce do.
 *     The progress / level callbacks fire on the cycle's thread after its lock is released: they may call this API.
 */
#ifndef LIBZL_HOTPATH_H
#define LIBZL_HOTPATH_H

#include <stdbool.h>
#include <stdint.h>

#include "zlhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ClipAudioSource ClipAudioSource;

/* ---- ClipAudioSource API bridge (libzl.h:23-61, libzl.cpp:107-302) ------------------------- */
ClipAudioSource *ClipAudioSource_byID(int id);                                          /* libzl.h:23 */
ClipAudioSource *ClipAudioSource_new(const char *filepath, bool muted);                 /* libzl.h:24 */
void ClipAudioSource_setProgressCallback(ClipAudioSource *c, void (*functionPtr)(float)); /* libzl.h:25 */
void ClipAudioSource_play(ClipAudioSource *c, bool loop);                               /* libzl.h:28 */
void ClipAudioSource_stop(ClipAudioSource *c);                                          /* libzl.h:29 */
void ClipAudioSource_playOnChannel(ClipAudioSource *c, bool loop, int midiChannel);     /* libzl.h:30 */
void ClipAudioSource_stopOnChannel(ClipAudioSource *c, int midiChannel);                /* libzl.h:31 */
float ClipAudioSource_getDuration(ClipAudioSource *c);                                  /* libzl.h:32 */
const char *ClipAudioSource_getFileName(ClipAudioSource *c);                            /* libzl.h:33 */
void ClipAudioSource_setStartPosition(ClipAudioSource *c, float startPositionInSeconds);/* libzl.h:34 */
void ClipAudioSource_setLength(ClipAudioSource *c, float beat, int bpm);                /* libzl.h:36 */
void ClipAudioSource_setPan(ClipAudioSource *c, float pan);                             /* libzl.h:37 */
void ClipAudioSource_setSpeedRatio(ClipAudioSource *c, float speedRatio);               /* libzl.h:38 (re-renders the clip on the device, clamped to [0.25, 4]; zlhip_sound_rerender) */
void ClipAudioSource_setPitch(ClipAudioSource *c, float pitchChange);                   /* libzl.h:39 (re-renders the clip on the device, clamped to [-24, 24] semitones) */
void ClipAudioSource_setGain(ClipAudioSource *c, float db);                             /* libzl.h:40 (re-renders the clip on the device; a NaN gain is ignored) */
void ClipAudioSource_setVolume(ClipAudioSource *c, float vol);                          /* libzl.h:41 */
void ClipAudioSource_setAudioLevelChangedCallback(ClipAudioSource *c, void (*functionPtr)(float)); /* libzl.h:42 */
void ClipAudioSource_setSlices(ClipAudioSource *c, int slices);                         /* libzl.h:44 */
int  ClipAudioSource_keyZoneStart(ClipAudioSource *c);                                  /* libzl.h:45 */
void ClipAudioSource_setKeyZoneStart(ClipAudioSource *c, int keyZoneStart);             /* libzl.h:46 */
int  ClipAudioSource_keyZoneEnd(ClipAudioSource *c);                                    /* libzl.h:47 */
void ClipAudioSource_setKeyZoneEnd(ClipAudioSource *c, int keyZoneEnd);                 /* libzl.h:48 */
int  ClipAudioSource_rootNote(ClipAudioSource *c);                                      /* libzl.h:49 */
void ClipAudioSource_setRootNote(ClipAudioSource *c, int rootNote);                     /* libzl.h:50 */
void ClipAudioSource_destroy(ClipAudioSource *c);                                       /* libzl.h:51 */
int  ClipAudioSource_id(ClipAudioSource *c);                                            /* libzl.h:52 */
float ClipAudioSource_adsrAttack(ClipAudioSource *c);                                   /* libzl.h:54 */
void ClipAudioSource_setADSRAttack(ClipAudioSource *c, float newValue);                 /* libzl.h:55 */
float ClipAudioSource_adsrDecay(ClipAudioSource *c);                                    /* libzl.h:56 */
void ClipAudioSource_setADSRDecay(ClipAudioSource *c, float newValue);                  /* libzl.h:57 */
float ClipAudioSource_adsrSustain(ClipAudioSource *c);                                  /* libzl.h:58 */
void ClipAudioSource_setADSRSustain(ClipAudioSource *c, float newValue);                /* libzl.h:59 */
float ClipAudioSource_adsrRelease(ClipAudioSource *c);                                  /* libzl.h:60 */
void ClipAudioSource_setADSRRelease(ClipAudioSource *c, float newValue);                /* libzl.h:61 */

/* ---- SyncTimer API bridge, the part that schedules ClipCommands (libzl.h:69-79, libzl.cpp:311-349) ----
 * Served by the step ring of libzl_hotpath_cycle; the registered timer callbacks fire on the cycle's thread after each cycle, once per
 * tick the timer went through.  SyncTimer_instance returns the reference's Qt object and is not declared here. */
void SyncTimer_startTimer(int interval);                                                /* libzl.h:70: SyncTimer::start(bpm), SyncTimer.cpp:870-879 */
/* SamplerSynth::setChannelEnabled(channel, enabled) (SamplerSynth.h:48-53, SamplerSynth.cpp:343-351; a method of the SamplerSynth singleton, not a
 * libzl.h symbol): channels -2 .. 9.  A disabled channel takes its commands, its voices stand still, its output is silent (zlhip_bus_set_enabled). */
void SamplerSynth_setChannelEnabled(int channel, bool enabled);
void SyncTimer_setBpm(unsigned int bpm);                                                /* libzl.h:71, SyncTimer.cpp:954-975 */
int  SyncTimer_getMultiplier(void);                                                     /* libzl.h:72, SyncTimer.cpp:946-948 */
void SyncTimer_stopTimer(void);                                                         /* libzl.h:73, SyncTimer.cpp:881-925 */
void SyncTimer_registerTimerCallback(void (*functionPtr)(int));                         /* libzl.h:74, SyncTimer.cpp:790-794: functionPtr(beat) per timer tick */
void SyncTimer_deregisterTimerCallback(void (*functionPtr)(int));                       /* libzl.h:75, SyncTimer.cpp:796-812 */
void SyncTimer_queueClipToStart(ClipAudioSource *clip);                                 /* libzl.h:76 */
void SyncTimer_queueClipToStartOnChannel(ClipAudioSource *clip, int midiChannel);       /* libzl.h:77, SyncTimer.cpp:815-832 */
void SyncTimer_queueClipToStop(ClipAudioSource *clip);                                  /* libzl.h:78 */
void SyncTimer_queueClipToStopOnChannel(ClipAudioSource *clip, int midiChannel);        /* libzl.h:79, SyncTimer.cpp:834-860 */

/* ---- misc (libzl.h:84-90) ----------------------------------------------------------------- */
void initJuce(void);                                                                    /* libzl.h:84: brings the engine up (12 channels x 8 voices) */
void shutdownJuce(void);                                                                /* libzl.h:85 */
void stopClips(int size, ClipAudioSource **clips);                                      /* libzl.h:89 */
float dBFromVolume(float vol);                                                          /* libzl.h:90 */

/* ---- JackPassthrough API bridge (libzl.h:117-175, libzl.cpp JackPassthrough_*) --------------- */
void  JackPassthrough_setPanAmount(int channel, float amount);
float JackPassthrough_getPanAmount(int channel);
float JackPassthrough_getWetFx1Amount(int channel);
void  JackPassthrough_setWetFx1Amount(int channel, float amount);
float JackPassthrough_getWetFx2Amount(int channel);
void  JackPassthrough_setWetFx2Amount(int channel, float amount);
float JackPassthrough_getDryAmount(int channel);
void  JackPassthrough_setDryAmount(int channel, float amount);
float JackPassthrough_getMuted(int channel);
void  JackPassthrough_setMuted(int channel, bool muted);

/* the parameter set of one passthrough client as zlhip_passthrough_process takes it (build-defined) */
int   JackPassthrough_getParams(int channel, zlhip_passthrough_params *out);

/* ---- build-defined additions (absent in libzl.h) ---------------------------------------------- */
/* engine configuration used by the next initJuce() (defaults: 12 x 8 voices, 48 kHz, faithful mode) */
void libzl_hotpath_configure(const zlhip_config *cfg);
/* 0 if the engine is up, else the zlhip status that initJuce() hit (e.g. ZLHIP_ERR_NO_DEVICE) */
int  libzl_hotpath_status(void);
zlhip_engine *libzl_hotpath_engine(void);
/* the millisecond clock behind the 30 ms / 100 ms rate limits and the positions model's time stamps (the reference reads
 * QDateTime::currentMSecsSinceEpoch(), ClipAudioSource.cpp:89,111,226,238): NULL = the wall clock.  A host that renders
 * faster or slower than real time (offline bounce, deterministic tests) installs its own. */
void libzl_hotpath_set_clock_ms(int64_t (*clock_ms)(void));
/* a clip from memory instead of a file (planar fp32, right == NULL for mono) */
ClipAudioSource *ClipAudioSource_newFromBuffer(const float *left, const float *right, int length, double sampleRate, const char *name);
/* the per-cycle seam: what SamplerChannel::process does for every channel (SamplerSynth.cpp:116-148).
 * out_left / out_right: [num_buses][nframes].  Afterwards the per-clip positions models are updated from
 * the voice reports and the progress / audio-level callbacks fire (ClipAudioSource.cpp:88-113,225-240). */
int  libzl_hotpath_process(uint32_t nframes, const zlhip_clock *clock, float *out_left, float *out_right);
/* The same cycle with the JackPassthrough clients behind the channels (JackPassthroughPrivate::process, JackPassthrough.cpp:45-115; clients
 * and their channels: MidiRouter.cpp:876-883 -- "GlobalPlayback" behind channel -1 = bus 1, "FXPassthrough-Channel<n>" behind channel n-1 = bus
 * n+1; a bus without a client in the reference gets one at its defaults): fan_out [num_buses][6][nframes] = dryL, dryR, fx1L, fx1R, fx2L, fx2R of
 * every bus, with the dry / wet / pan amounts and mute flags the JackPassthrough_set* calls stored -- read per cycle, no lock, no HIP call;
 * on the real-time cycle the resident kernel writes the rows from the registers that hold the mix.  fan_out == NULL: libzl_hotpath_process. */
int  libzl_hotpath_process_fanout(uint32_t nframes, const zlhip_clock *clock, float *out_left, float *out_right, float *fan_out);
/* The same cycle with this library's own transport: SyncTimerPrivate::process (SyncTimer.cpp:452-702) for the JACK cycle
 * [current_usecs, next_usecs) -- the steps of the 32768-step ring that fall due are played, their ClipCommands dispatched
 * with the playhead (:553-558), SetBpm commands applied, playhead and step clock rolled -- then every channel is rendered
 * with the clock SyncTimer's getters return (:990-1009), and, while the timer runs, the timer thread's tick
 * (hiResTimerCallback, :391-418) is taken once.  Arguments as jack_get_cycle_times returns them (SamplerSynth.cpp:128). */
int  libzl_hotpath_cycle(uint32_t nframes, uint64_t current_usecs, uint64_t next_usecs, float period_usecs, float *out_left, float *out_right);
int  libzl_hotpath_cycle_fanout(uint32_t nframes, uint64_t current_usecs, uint64_t next_usecs, float period_usecs, float *out_left, float *out_right,
                                float *fan_out /* as libzl_hotpath_process_fanout */);
/* play / stop / queue / timer calls are handed to the cycle through a bounded queue (4096 requests, FreshCommandStashSize of SyncTimer.cpp:252;
 * ClipAudioSource_stop(-3) alone is 12 of them) that only a cycle drains: how many requests were LOST because it was full -- no cycle ran
 * (before JACK starts, during libzl_hotpath_bounce_to_wav).  The callers return void as in libzl.h; a host that floods the queue reads this. */
uint64_t libzl_hotpath_dropped_requests(void);
/* Offline bounce of the running session to WAV files (BASELINE configs[4] from / to real files): what nblocks calls of
 * libzl_hotpath_cycle would render -- the library's own transport, JACK time start_usecs + k * round(1e6 * nframes / fs), commands
 * dispatched in the cycle their step falls due in -- rendered in batches through zlhip_bounce and written as one stereo WAV per sampler
 * channel, "<prefix>-channel_<bus>.wav": bits_per_sample 16 = the recorder's format (AudioLevels.cpp:53-58), 32 = float.  The
 * positions models and callbacks are not driven.  Returns 0 or a negative zlhip status. */
int  libzl_hotpath_bounce_to_wav(const char *prefix, int64_t nblocks, uint32_t nframes, uint64_t start_usecs, int bits_per_sample);
/* Extension: the parameters of a clip as the engine receives them at the next cycle -- among them the slice table that
 * ClipAudioSource_setSlices builds (ClipAudioSource.cpp:495-528; the reference exposes it as a Qt property only).  No device needed.
 * Returns 0, or -1 for a null argument. */
int  libzl_hotpath_clip_params(ClipAudioSource *c, zlhip_clip_params *out);
/* SyncTimer::scheduleClipCommand(command, delay) (SyncTimer.cpp:1011-1048): what ClipAudioSource_play / _stop call with delay 0;
 * command->clip is the zlhip clip id (ClipAudioSource_engineClip) */
void libzl_hotpath_schedule_clip_command(const zlhip_clip_command *command, uint64_t delay);
/* one more tick of the timer thread (hiResTimerCallback) before the next libzl_hotpath_cycle */
void libzl_hotpath_timer_tick(void);
/* SyncTimer::jackPlayhead / jackPlayheadUsecs / jackSubbeatLengthInMicroseconds (SyncTimer.cpp:990-1009) of the library's own
 * transport, in the playhead fields of *out */
int  libzl_hotpath_transport(zlhip_clock *out);
/* ClipAudioSourcePositionsModel read-outs of a clip (ClipAudioSourcePositionsModel.cpp:160-185) */
float  ClipAudioSource_peakGain(ClipAudioSource *c);
double ClipAudioSource_firstProgress(ClipAudioSource *c);
float  ClipAudioSource_volumeAbsolute(ClipAudioSource *c);                              /* ClipAudioSource.cpp:338-346 */
void   ClipAudioSource_setVolumeAbsolute(ClipAudioSource *c, float vol);                /* ClipAudioSource.cpp:328-336 */
int    ClipAudioSource_engineClip(ClipAudioSource *c);                                  /* zlhip clip id */
/* The data behind WaveFormItem (lib/WaveFormItem.cpp:130-139 paints a juce::AudioThumbnail of the clip between `start` and
 * qMin(end, total length) seconds): per pixel column (minL, maxL, minR, maxR) of the clip's current playback data -- after setPitch /
 * setSpeedRatio / setGain the re-rendered clip -- computed on the device (zlhip_sound_overview); out: [columns][4] floats, a mono clip
 * repeats its channel.  Seconds are seconds of the playback data; frames are floor(seconds * sample rate) in double, clamped to the
 * data; end_seconds <= start_seconds or an end beyond the data means "to the end".  1 <= columns <= ZLHIP_OVERVIEW_MAX_COLUMNS.
 * Returns 0 or a negative zlhip status (out is not written then).  The painting stays the host's. */
int  libzl_hotpath_clip_waveform(ClipAudioSource *c, float start_seconds, float end_seconds, int columns, float *out);
/* Slice the clip at its transients (build-defined: the reference's setSlices only divides evenly, ClipAudioSource.cpp:495-528).  The
 * transients of the clip's current playback data between its start and its start + length -- in frames, cast as SamplerSynthSound
 * does (SamplerSynthSound.cpp:96-104) -- are found on the device (zlhip_sound_onsets with its defaults and max_onsets = the number of
 * slices asked for: with more transients than slices the strongest stay).  Slice 0 is 0.0; an onset nearer to the region's start than
 * (min_gap_hops + 1) * hop_frames frames is slice 0 itself and is dropped; every other onset becomes
 * (double)(frame - start) / (double)(stop - start).  At most min(max_slices, ZLHIP_MAX_SLICES) entries; `slices` becomes the table's
 * length, as setSlicePositions does (ClipAudioSource.cpp:535-543), and the table is published like ClipAudioSource_setSlices.
 * Returns the number of slices, or a negative zlhip status that leaves the clip as it was. */
int  libzl_hotpath_clip_slice_at_transients(ClipAudioSource *c, int max_slices);
/* The clip's tempo (build-defined: the reference has no tempo estimate; setLength(beat, bpm) and setSpeedRatio take one the caller
 * must know).  Estimated on the device (zlhip_sound_tempo, hop_frames at its default) over the clip's current playback data between its
 * start and its start + length, in frames as for libzl_hotpath_clip_slice_at_transients.  bpm_min / bpm_max of 0 take 75 / 150.
 * *bpm = 0 (and *confidence = 0) means "no tempo": silence, or a region too short for the range; that is not an error.  Returns 0 or a
 * negative zlhip status (nothing is written then). */
int  libzl_hotpath_clip_tempo(ClipAudioSource *c, float bpm_min, float bpm_max, float *bpm, float *confidence);
/* Fit the clip to target_bpm: detects as libzl_hotpath_clip_tempo(c, 0, 0, ...) over the data the clip plays now and sets the speed
 * ratio (float)(target_bpm * current speed ratio / detected) through ClipAudioSource_setSpeedRatio's path (its clamp to [0.25, 4]
 * stays; a re-render starts from the original upload, hence the current ratio in the product).  *ratio_out: the ratio now in effect.
 * Returns 1, or 0 where there is no tempo or the confidence is below min_confidence (nothing changes then), or a negative status. */
int  libzl_hotpath_clip_match_tempo(ClipAudioSource *c, float target_bpm, float min_confidence, float *ratio_out);
/* The clip's pitch (build-defined: the reference has no pitch detection; ClipAudioSource_setRootNote takes a note the caller must
 * know).  Detected on the device (zlhip_sound_pitch, every other field at its default) over the clip's current playback data between
 * its start and its start + length, in frames as for libzl_hotpath_clip_tempo.  f_min / f_max of 0 take 55 / 1760 Hz.  *note is the
 * fractional MIDI note.  *hz = 0 (and *note = *confidence = 0) means "no pitch": silence, noise, a drum hit, or a region shorter than
 * one analysis frame; that is not an error.  A note above f_max comes back an octave low.  Returns 0 or a negative zlhip status
 * (nothing is written then). */
int  libzl_hotpath_clip_pitch(ClipAudioSource *c, float f_min, float f_max, float *hz, float *note, float *confidence);
/* Set the clip's root note from its pitch: detects as libzl_hotpath_clip_pitch(c, 0, 0, ...) and sets root_note = clamp(rint(note), 0,
 * 127) through ClipAudioSource_setRootNote's path, so the next startNote uses it.  *root_note_out: the note set.  Returns 1, or 0 where
 * there is no pitch or the confidence is below min_confidence (nothing changes then, *root_note_out included), or a negative status. */
int  libzl_hotpath_clip_detect_root_note(ClipAudioSource *c, float min_confidence, int *root_note_out);
/* The clip's loudness (build-defined: the reference has no loudness measurement; ClipAudioSource_setGain takes a dB value the caller
 * must know).  Measured on the device (zlhip_sound_loudness, sub_frames at its default) over the clip's current playback data between
 * its start and its start + length, in frames as for libzl_hotpath_clip_pitch.  *lufs: the integrated loudness of ITU-R BS.1770-4 /
 * EBU R 128; *peak_db: 20 log10 of the largest sample peak (not a true peak).  Returns 1, or 0 for "no loudness" -- silence, or
 * nothing above -70 LUFS; *lufs is -inf then -- or a negative zlhip status (nothing is written then). */
int  libzl_hotpath_clip_loudness(ClipAudioSource *c, double *lufs, float *peak_db);
/* Bring the clip to target_lufs: measures as libzl_hotpath_clip_loudness, delta = target_lufs - lufs, held so that the sample peak
 * stays at or below ceiling_db (delta = min(delta, ceiling_db - 20 log10(peak))), and sets the gain (float)(current gain + delta)
 * through ClipAudioSource_setGain's path (a re-render starts from the original upload and the measured data already carries the
 * current gain, hence the sum).  *gain_db_out: the gain now in effect.  Returns 1, or 0 where there is no loudness (nothing changes
 * then), or a negative status; a NaN target or ceiling is ZLHIP_ERR_INVALID. */
int  libzl_hotpath_clip_normalize(ClipAudioSource *c, float target_lufs, float ceiling_db, float *gain_db_out);
/* Level a bank: ONE zlhip_sound_loudness_batch call for all clips and ONE zlhip_sound_rerender_batch call for those that change.  A
 * clip that is NULL, not in the engine or without loudness stays as it is; gains_out[i] (may be NULL) is clip i's gain afterwards (0
 * for NULL).  Duplicate clips are ZLHIP_ERR_INVALID.  If the re-render fails every clip and every stored gain is as it was.  Returns
 * the number of clips levelled, or a negative status. */
int  libzl_hotpath_clips_level(ClipAudioSource **clips, int count, float target_lufs, float ceiling_db, float *gains_out);
/* extension (build-defined: the reference has no loop finder): the seamless loop points of the data the clip plays now, searched on
 * the device near its start and its start + length (zlhip_sound_loop), in frames as for
 * libzl_hotpath_clip_pitch.  search_ms: how far around each point to look (0: 10 ms; at most 2047 frames); window: the frames
 * compared around each point (0: 256).  *start_frame, *stop_frame: the pair whose surroundings match best; *seam_db, *nominal_db:
 * 10 log10 of the mismatch against the windows' energy at that pair and at the clip's own points (0 where those are no candidate
 * pair).  A candidate's window lies inside the data, so a clip whose region is the whole file is searched from window / 2 frames in:
 * the call is meant for sustain loops inside a sound.  Returns 1, or 0 where no pair was found, or a negative zlhip status (nothing
 * is written then). */
int  libzl_hotpath_clip_find_loop(ClipAudioSource *c, float search_ms, int window, int *start_frame, int *stop_frame, double *seam_db, double *nominal_db);
/* Move the clip's loop to its seamless points: finds them as libzl_hotpath_clip_find_loop (window 256) and, where the seam improves on
 * the clip's own points by at least min_improvement_db, sets startPositionInSeconds and lengthInSeconds to the float seconds from
 * which a voice derives exactly those frames (zlhip_loop_seconds), under ClipAudioSource_setStartPosition's lock and through its
 * publish.  lengthInBeats stays; the slices are fractions of the length and move with it.  Returns 1 if applied; 0 where nothing was
 * found, the improvement is below the bar or the frames are not representable in float seconds -- the clip is untouched then; or a
 * negative status. */
int  libzl_hotpath_clip_snap_loop(ClipAudioSource *c, float search_ms, float min_improvement_db, int *start_frame, int *stop_frame);
/* A bank: ONE zlhip_sound_loop_batch call for all clips.  A clip that is NULL or not in the engine stays as it is; applied_out[i] (may
 * be NULL) is 1 where clip i's loop was moved.  Duplicate clips are ZLHIP_ERR_INVALID.  Returns the number of clips moved, or a
 * negative status (nothing has changed then). */
int  libzl_hotpath_clips_snap_loops(ClipAudioSource **clips, int count, float search_ms, float min_improvement_db, int *applied_out);
/* extension (build-defined: the reference has no loop crossfade): bakes a crossfade into the clip's data on the device, so that its
 * sustain loop wraps without a jump (zlhip_sound_loop_crossfade).  The loop is the clip's start .. start + length
 * in the frames a voice derives from them; fade_ms: the length of the fade (0: 20 ms), cut to what the lead-in in front of the start
 * and the loop itself hold, at most 65536 frames; curve: ZLHIP_XFADE_AUTO (from the measured correlation of the two regions),
 * ZLHIP_XFADE_LINEAR or ZLHIP_XFADE_EQUAL_POWER.  *fade_frames, *correlation (may be NULL): what was faded and measured.  The clip keeps
 * its id and its parameters; a voice playing it reads the new data from its next block.  The fade cannot be taken back: reload the
 * clip.  A clip that plays a re-render (a gain, pitch or speed other than the identity) is refused with ZLHIP_ERR_STATE: crossfade
 * first, level afterwards -- a later gain keeps the seam, a pitch or speed render moves the frames.  Returns 1 if applied, 0 where there
 * is nothing to fade (a loop from frame 0 has no lead-in), or a negative status (nothing has changed then). */
int  libzl_hotpath_clip_crossfade_loop(ClipAudioSource *c, float fade_ms, int curve, int *fade_frames, double *correlation);
/* A bank: ONE zlhip_sound_loop_batch with libzl_hotpath_clips_snap_loops' logic, then ONE zlhip_sound_loop_crossfade_batch.  results[i]
 * (may be NULL): bit 0 = clip i's loop was moved, bit 1 = its loop was crossfaded.  A clip that is NULL, not in the engine or playing a
 * re-render stays as it is.  Duplicate clips are ZLHIP_ERR_INVALID.  Returns the number of clips crossfaded, or a negative status. */
int  libzl_hotpath_clips_seal_loops(ClipAudioSource **clips, int count, float search_ms, float min_improvement_db, float fade_ms, int curve, int *results);
/* extension (build-defined: the reference has no such edit): cuts the silence off the front and the back of the clip's data, on the
 * device and under the clip's own id (zlhip_sound_edit with ZLHIP_EDIT_TRIM over the whole data).  threshold_db:
 * a frame at or above it in any channel is loud (0: the default, 2^-10 of full scale, about -60 dBFS); pre_roll_ms, hold_ms: what is
 * kept in front of the first and behind the last loud frame.  Afterwards the duration is the new data's, startPositionInSeconds has
 * moved back by the frames removed in front (not below 0) and lengthInSeconds is cut to what lies behind the start, both as the float
 * seconds from which a voice derives exactly those frames.  *removed_front_frames, *new_length_frames may be NULL.  The trim cannot be
 * taken back: reload the clip.  A clip that plays a re-render is refused with ZLHIP_ERR_STATE: trim first, then tune and level.
 * Returns 1, or 0 for a silent or already tight clip (nothing has changed), or a negative status (nothing has changed). */
int  libzl_hotpath_clip_trim_silence(ClipAudioSource *c, float threshold_db, float pre_roll_ms, float hold_ms, int *removed_front_frames, int *new_length_frames);
/* A bank: ONE zlhip_sound_edit_batch call for all clips.  A clip that is NULL, not in the engine or playing a re-render stays as it is;
 * applied_out[i] (may be NULL) is 1 where clip i was trimmed.  Duplicate clips are ZLHIP_ERR_INVALID.  Returns the number of clips
 * trimmed, or a negative status (nothing has changed then). */
int  libzl_hotpath_clips_trim(ClipAudioSource **clips, int count, float threshold_db, float pre_roll_ms, float hold_ms, int *applied_out);
/* extension (build-defined: the reference measures no peak): the sample peak and the true peak of the data the clip plays now between
 * its start and its start + length, measured on the device (zlhip_sound_peak with ZLHIP_LIMIT_TRUE_PEAK), in dB
 * (20 log10; -inf for silence).  Returns 1, or a negative zlhip status (nothing is written then; ZLHIP_ERR_INVALID at a rate the true
 * peak cannot be asked at). */
int  libzl_hotpath_clip_true_peak(ClipAudioSource *c, float *sample_peak_db, float *true_peak_db);
/* extension: brings the clip's peaks under ceiling_db (<= 0 dBFS) with a look-ahead limiter baked into its data at its current level,
 * on the device and under the clip's own id (zlhip_sound_limit with gain 1).  lookahead_ms: the ramp in front of
 * and behind a peak (0: 5 ms; at most 512 frames); hold_ms: how long the reduction stays behind a peak (at most 512 frames); true_peak:
 * detect on the inter-sample peaks as well.  A frame out of reach of every peak keeps its bits.  *reduction_db (may be NULL): the largest
 * reduction, >= 0.  The limit cannot be taken back: reload the clip.  A clip that plays a re-render is refused with ZLHIP_ERR_STATE:
 * limit first, then tune.  Returns 1, or 0 for a clip already under the ceiling (nothing has changed), or a negative status (nothing
 * has changed). */
int  libzl_hotpath_clip_limit(ClipAudioSource *c, float ceiling_db, float lookahead_ms, float hold_ms, int true_peak, float *reduction_db);
/* Level a bank under a ceiling: ONE zlhip_sound_loudness_batch and ONE zlhip_sound_limit_batch.  Every clip is driven by target_lufs -
 * lufs -- NOT held by the ceiling, as libzl_hotpath_clips_level is -- the drive is baked as the limiter's gain and the peaks it lifts
 * over ceiling_db are limited.  The limiter takes some loudness back, so a clip lands at or under the target; the caller may measure
 * again (libzl_hotpath_clip_loudness) and call again.  The clip's gain (ClipAudioSource_setGain) is not touched: the levelled data is the
 * clip's original from now on.  A clip that is NULL, not in the engine, playing a re-render or without loudness stays as it is;
 * drive_db_out[i], reduction_db_out[i] (may be NULL): the drive baked into clip i and its largest reduction (0 where it was left).
 * Duplicate clips are ZLHIP_ERR_INVALID.  Returns the number of clips changed, or a negative status (nothing has changed then). */
int  libzl_hotpath_clips_level_limited(ClipAudioSource **clips, int count, float target_lufs, float ceiling_db, float lookahead_ms, float hold_ms, int true_peak,
                                       float *drive_db_out, float *reduction_db_out);
/* Crops the clip's data to its selected region -- exactly the frames a voice derives from start .. start + length -- and fades its ends:
 * fade_in_ms, fade_out_ms (each cut to half the region), curve ZLHIP_EDIT_LINEAR, _SQRT or _SMOOTH.  Afterwards the start is 0 and the
 * length and the duration are the data's.  *new_length_frames may be NULL.  No undo; a clip that plays a re-render is ZLHIP_ERR_STATE.
 * Returns 1, or 0 where the region is the whole data and nothing fades, or a negative status (nothing has changed then). */
int  libzl_hotpath_clip_crop(ClipAudioSource *c, float fade_in_ms, float fade_out_ms, int curve, int *new_length_frames);
/* Turns the clip's whole data round.  The start becomes duration - (start + length), computed in frames, so that the clip plays the same
 * region backwards; the length stays.  Reversing twice restores the data bit for bit.  A clip that plays a re-render is
 * ZLHIP_ERR_STATE.  Returns 1, or a negative status (nothing has changed then). */
int  libzl_hotpath_clip_reverse(ClipAudioSource *c);
/* extension (build-defined: the reference has no warp): fits a loop to the session grid hit by hit, on the device (zlhip_sound_warp,
 * DESIGN.md section 19) -- what a sampler calls "warp" or "quantise audio".  The clip's transients are found over its whole original
 * (zlhip_sound_onsets with its defaults); every hit is moved by `strength` (0 .. 1) towards the nearest step of the grid of src_bpm
 * with steps_per_beat steps (1 .. 64) per beat, counted from the clip's start frame, and the whole is scaled to the session's bpm (the
 * scheduler's); zlhip_warp_plan makes the anchors, hits that would need a region outside a ratio of 2 are left where the stretch puts
 * them.  src_bpm 0: detected as libzl_hotpath_clip_tempo(c, 0, 0, ...) does; no tempo returns 0 and changes nothing.  *onsets_moved
 * (may be NULL): the hits that became anchors; *new_length_frames (may be NULL): the frames of the clip's data now.  The clip keeps its
 * id and its parameters (seconds of the playback data); the warp cannot be taken back: reload the clip.  A clip that plays a re-render
 * is refused with ZLHIP_ERR_STATE: warp first, then tune and level.  Returns 1 for warped, 0 for nothing to do, or a negative status
 * (nothing has changed then). */
int  libzl_hotpath_clip_warp_to_grid(ClipAudioSource *c, float src_bpm, int steps_per_beat, float strength, int *onsets_moved, int *new_length_frames);
/* extension (build-defined: the reference has no key detection): the musical key of the data the clip plays now between its start and
 * its start + length, detected on the device (zlhip_sound_key with the defaults).  *tonic: 0 = C .. 11 = B, or
 * -1 for "no key" (silence, a region shorter than one analysis frame, a flat chroma), which is not an error; *mode: 0 major, 1 minor;
 * *confidence: Pearson's r of the chroma with the key's Krumhansl-Kessler profile.  Returns ZLHIP_OK or a negative status. */
int  libzl_hotpath_clip_key(ClipAudioSource *c, int *tonic, int *mode, double *confidence);
/* A bank: ONE zlhip_sound_key_batch call for all clips.  A clip that is NULL or not in the engine reads "no key".  The out arrays may
 * be NULL.  Returns the number of clips with a key, or a negative status. */
int  libzl_hotpath_clips_keys(ClipAudioSource **clips, int count, int *tonics, int *modes, double *confidences);
/* Transpose the clip into the session's key (tonic 0 .. 11, mode 0 major / 1 minor), the counterpart of libzl_hotpath_clip_match_tempo:
 * detects the clip's key and adds shift = ((target - clip_tonic + 6) mod 12) - 6 semitones, -6 .. +5, to its current pitch change, as
 * ClipAudioSource_setPitch would (same locks, same clamp, one re-render).  Where the modes differ the clip is compared through its
 * relative key (major: tonic + 9, minor: tonic + 3).  *semitones_out (may be NULL): the shift.  Returns 1, or 0 for "no key" (the clip
 * is untouched and *semitones_out is 0), or a negative status. */
int  libzl_hotpath_clip_match_key(ClipAudioSource *c, int tonic, int mode, int *semitones_out);
/* A bank of clips in one engine call: every file is read, their `data` chunks go to the engine as raw PCM in ONE
 * zlhip_sound_upload_pcm_batch call (decoded on the device, one wait for the whole bank).  out[i] is the clip of paths[i], or NULL
 * for a file that cannot be opened or decoded -- it does not fail the others.  Returns the number of clips loaded (or a negative
 * zlhip status for bad arguments).  ZL_PCM_DECODE=0 (read per call) and files with more than ZLHIP_PCM_MAX_CHANNELS channels take
 * ClipAudioSource_new's host decode, clip by clip; the playback data is bit-identical either way. */
int  libzl_hotpath_clips_new(const char *const *paths, int count, ClipAudioSource **out);
/* Convert clips to the engine's sample rate on the device, band-limited, in ONE zlhip_sound_convert_rate_batch call: from then on they
 * play as unit-step sources (the on-grid path) instead of through the pitched path.  Build-defined and opt-in: the reference resamples
 * while it plays, so a converted clip no longer reproduces its bits.  A clip the conversion does not take -- NULL, not in the engine,
 * re-rendered by setPitch / setSpeedRatio / setGain, or at a ratio beyond the limits (zlhip.h) -- stays as it is and plays pitched.
 * ClipAudioSource_getDuration, the start, the length and the slices are seconds and do not change.  Convert before playing.
 * Returns how many of the clips are at the engine's rate afterwards, or a negative zlhip status (every clip is as it was then).
 * ZL_LOAD_CONVERT=1 (read per call, default 0) makes ClipAudioSource_new and libzl_hotpath_clips_new convert what they loaded; the
 * clips of one libzl_hotpath_clips_new call go in one batch.  With 0 the loaders do exactly what they did before. */
int  libzl_hotpath_clips_convert(ClipAudioSource *const *clips, int count);
/* minimal RIFF/WAVE IO (decode side of SamplerSynthSound.cpp:28-59; record side of AudioLevels.cpp:35-119) */
int  libzl_wav_read(const char *path, float **left, float **right, int *length, double *sampleRate);  /* malloc'd planes; free with libzl_wav_free */
void libzl_wav_free(float *plane);
int  libzl_wav_write(const char *path, const float *left, const float *right, int length, double sampleRate, int bitsPerSample /* 16 or 32(float) */);
/* the same file from already interleaved frames: 16 bit = int16_t pairs as zlhip_bounce(ZLHIP_BOUNCE_PCM16_STEREO) delivers them per bus, 32 = float */
int  libzl_wav_write_interleaved(const char *path, const void *frames, int length, int channels, double sampleRate, int bitsPerSample);

#ifdef __cplusplus
}
#endif
#endif
