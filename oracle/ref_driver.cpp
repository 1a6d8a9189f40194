/*
 * ref_driver.cpp -- drives the reference's own SamplerSynthVoice.cpp, compiled UNMODIFIED.  TEST INFRASTRUCTURE ONLY.
 *
 * libzl_amd/build.py build_reference() compiles <reference>/lib/SamplerSynthVoice.cpp against the stand-in headers of
 * oracle/ref_shim/ and links it with this file and zl_oracle.c into oracle/_ref/libzl_refvoice.so (never committed).  Every
 * statement of setCurrentCommand, startNote, stopNote and process then is the reference's text run by a compiler.
 *
 * This file is ours.  It supplies what the voice calls on its neighbours as "return the field the test set":
 *   ClipAudioSource   getStartPosition(slice), volumeAbsolute, pan, getLengthInBeats, getDuration, adsrParameters, playbackPositionsModel
 *   SamplerSynthSound isValid, audioData, length, stopPosition(slice), rootMidiNote, sourceSampleRate, clip
 *   SyncTimer         jackPlayhead, jackPlayheadUsecs, jackSubbeatLengthInMicroseconds, getBpm, getMultiplier, subbeatCountToSeconds,
 *                     deleteClipCommand
 *   positions model   createPositionID / removePosition (row bookkeeping of the oracle's zlo_positions_*), setPositionGainAndProgress
 *                     (records the voice's report)
 *   juce::ADSR        a wrapper over the oracle's zlo_adsr_* : the envelope is the SAME restatement on both sides and is not pinned.
 * Slice start / stop positions and subbeatCountToSeconds are values the test hands in (it takes them from the oracle's clip
 * functions): ClipAudioSource.cpp, SamplerSynthSound.cpp and SyncTimer.cpp are outside the anchor.
 *
 * The reference's loop stores to leftBuffer[1 .. nframes]; a channel's buffers here are nframes + 1 floats, all returned.
 */
#include "SamplerSynthVoice.h"

#include "ClipAudioSourcePositionsModel.h"
#include "ClipCommand.h"
#include "SamplerSynthSound.h"
#include "SyncTimer.h"
#include "libzl.h"

#include <cstring>
#include <vector>

namespace {

constexpr int kSliceEntries = ZLO_MAX_SLICES + 1;          /* entry 0: slice -1 (and every slice outside the table), entry s + 1: slice s */
inline int sliceEntry(int slice) { return (slice > -1 && slice < ZLO_MAX_SLICES) ? slice + 1 : 0; }

struct TimerFields {
    quint64 jackPlayhead = 0, jackPlayheadUsecs = 0, jackSubbeatLengthInMicroseconds = 0, bpm = 120;
    int multiplier = ZLO_BEAT_SUBDIVISIONS;
    float oneSubbeatInSeconds = 0.0f;
};
struct ModelFields {
    zlo_positions rows;
};
struct ClipFields {
    float volumeAbsolute = 1.0f, pan = 0.0f, lengthInBeats = -1.0f, duration = 0.0f;
    float startPosition[kSliceEntries] = {};
    juce::ADSR::Parameters adsr = {0.0f, 0.1f, 1.0f, 0.05f};
    ClipAudioSourcePositionsModel *model = nullptr;
};
struct SoundFields {
    ClipAudioSource *clip = nullptr;
    juce::AudioBuffer<float> *data = nullptr;
    int length = 0, rootMidiNote = 60, valid = 1;
    int stopPosition[kSliceEntries] = {};
    double sourceSampleRate = 44100.0;
};

/* the members `d` of the reference's classes are private: each constructor below leaves its fields here for the C interface */
TimerFields *g_timer = nullptr;
ClipFields *g_newClip = nullptr;
SoundFields *g_newSound = nullptr;
SyncTimer *g_syncTimer = nullptr;
zlo_report *g_report = nullptr;                            /* where the voice being processed reports to */

} // namespace

/* ---- juce::ADSR over the oracle's restatement -------------------------------------------------------------------------- */
namespace juce {
ADSR::ADSR() { zlo_adsr_init(&state); parameters = {state.p.attack, state.p.decay, state.p.sustain, state.p.release}; }
void ADSR::setParameters(const Parameters &p)
{
    parameters = p;
    const zlo_adsr_params q = {p.attack, p.decay, p.sustain, p.release};
    zlo_adsr_set_parameters(&state, &q);
}
const ADSR::Parameters &ADSR::getParameters() const noexcept { return parameters; }
bool ADSR::isActive() const noexcept { return zlo_adsr_is_active(&state) != 0; }
void ADSR::setSampleRate(double sr) noexcept { zlo_adsr_set_sample_rate(&state, sr); }
void ADSR::reset() noexcept { zlo_adsr_reset(&state); }
void ADSR::noteOn() noexcept { zlo_adsr_note_on(&state); }
void ADSR::noteOff() noexcept { zlo_adsr_note_off(&state); }
float ADSR::getNextSample() noexcept { return zlo_adsr_next(&state); }
} // namespace juce

/* ---- SyncTimer ---------------------------------------------------------------------------------------------------------- */
class SyncTimerPrivate : public TimerFields {};
SyncTimer::SyncTimer(QObject *parent) : QObject(parent), d(new SyncTimerPrivate) { g_timer = d; }
SyncTimer::~SyncTimer() { delete d; }
const quint64 &SyncTimer::jackPlayhead() const { return d->jackPlayhead; }
const quint64 &SyncTimer::jackPlayheadUsecs() const { return d->jackPlayheadUsecs; }
const quint64 &SyncTimer::jackSubbeatLengthInMicroseconds() const { return d->jackSubbeatLengthInMicroseconds; }
quint64 SyncTimer::getBpm() const { return d->bpm; }
int SyncTimer::getMultiplier() { return d->multiplier; }
float SyncTimer::subbeatCountToSeconds(quint64, quint64) const { return d->oneSubbeatInSeconds; }   /* asked for (bpm, 1) only */
void SyncTimer::deleteClipCommand(ClipCommand *command) { delete command; }

extern "C" QObject *SyncTimer_instance()
{
    if (!g_syncTimer) g_syncTimer = new SyncTimer(nullptr);
    return g_syncTimer;
}

/* ---- ClipAudioSourcePositionsModel --------------------------------------------------------------------------------------- */
class ClipAudioSourcePositionsModelPrivate : public ModelFields {};
ClipAudioSourcePositionsModel::ClipAudioSourcePositionsModel(ClipAudioSource *) : QAbstractListModel(nullptr), d(new ClipAudioSourcePositionsModelPrivate)
{
    zlo_positions_init(&d->rows);
}
ClipAudioSourcePositionsModel::~ClipAudioSourcePositionsModel() {}
template <typename K, typename V> class QHash {};
QHash<int, QByteArray> ClipAudioSourcePositionsModel::roleNames() const { return {}; }
int ClipAudioSourcePositionsModel::rowCount(const QModelIndex &) const { return ZLO_POSITION_COUNT; }
QVariant ClipAudioSourcePositionsModel::data(const QModelIndex &, int) const { return {}; }
qint64 ClipAudioSourcePositionsModel::createPositionID(float initialProgress) { return zlo_positions_create(&d->rows, initialProgress, 0); }
void ClipAudioSourcePositionsModel::removePosition(qint64 positionID) { zlo_positions_remove(&d->rows, positionID, 0); }
void ClipAudioSourcePositionsModel::setPositionGainAndProgress(qint64 positionID, float gain, float progress)
{
    zlo_positions_set_gain_and_progress(&d->rows, positionID, gain, progress, 0);
    if (g_report) { g_report->valid = 1; g_report->gain = gain; g_report->progress = progress; }
}

/* ---- ClipAudioSource ------------------------------------------------------------------------------------------------------ */
class ClipAudioSource::Private : public ClipFields {};
ClipAudioSource::ClipAudioSource(tracktion_engine::Engine *, SyncTimer *, const char *, bool, QObject *parent) : QObject(parent), d(new Private)
{
    d->model = new ClipAudioSourcePositionsModel(this);
    g_newClip = d;
}
ClipAudioSource::~ClipAudioSource() { delete d->model; delete d; }
float ClipAudioSource::getStartPosition(int slice) const { return d->startPosition[sliceEntry(slice)]; }
float ClipAudioSource::getLengthInBeats() const { return d->lengthInBeats; }
float ClipAudioSource::volumeAbsolute() const { return d->volumeAbsolute; }
float ClipAudioSource::getDuration() { return d->duration; }
float ClipAudioSource::pan() { return d->pan; }
const juce::ADSR::Parameters &ClipAudioSource::adsrParameters() const { return d->adsr; }
ClipAudioSourcePositionsModel *ClipAudioSource::playbackPositionsModel() { return d->model; }

/* ---- SamplerSynthSound ---------------------------------------------------------------------------------------------------- */
class SamplerSynthSoundPrivate : public SoundFields {};
SamplerSynthSound::SamplerSynthSound(ClipAudioSource *clip) : d(new SamplerSynthSoundPrivate) { d->clip = clip; g_newSound = d; }
SamplerSynthSound::~SamplerSynthSound() { delete d->data; delete d; }
ClipAudioSource *SamplerSynthSound::clip() const { return d->clip; }
bool SamplerSynthSound::isValid() const { return d->valid != 0; }
AudioBuffer<float> *SamplerSynthSound::audioData() const noexcept { return d->data; }
int SamplerSynthSound::length() const { return d->length; }
int SamplerSynthSound::stopPosition(int slice) const { return d->stopPosition[sliceEntry(slice)]; }
int SamplerSynthSound::rootMidiNote() const { return d->rootMidiNote; }
double SamplerSynthSound::sourceSampleRate() const { return d->sourceSampleRate; }

/* ---- the C interface (tests/ref_voice.py) ---------------------------------------------------------------------------------- */
struct zr_world {
    double playbackSampleRate;
    int nchannels, nvoices;
    std::vector<ClipAudioSource *> clips;
    std::vector<ClipFields *> clipFields;
    std::vector<SamplerSynthSound *> sounds;
    std::vector<SoundFields *> soundFields;
    std::vector<SamplerSynthVoice *> voices;                /* [nchannels * nvoices] */
    std::vector<zlo_report> reports;
    std::vector<float> left, right;
};

extern "C" {

zr_world *zr_world_new(int nchannels, int nvoices, double playbackSampleRate)
{
    SyncTimer_instance();
    zr_world *w = new zr_world;
    w->playbackSampleRate = playbackSampleRate;
    w->nchannels = nchannels;
    w->nvoices = nvoices;
    for (int i = 0; i < nchannels * nvoices; ++i) {
        SamplerSynthVoice *voice = new SamplerSynthVoice();
        voice->setCurrentPlaybackSampleRate(playbackSampleRate);
        w->voices.push_back(voice);
    }
    w->reports.assign((size_t)(nchannels * nvoices), zlo_report{0, 0.0f, 0.0f});
    return w;
}

void zr_world_free(zr_world *w)
{
    for (SamplerSynthVoice *voice : w->voices) delete voice;
    for (SamplerSynthSound *sound : w->sounds) delete sound;
    for (ClipAudioSource *clip : w->clips) delete clip;
    delete w;
}

/* one ClipAudioSource and its SamplerSynthSound (SamplerSynth::registerClip makes one sound per clip); left / right stay the caller's */
int zr_add_sound(zr_world *w, const float *left, const float *right, int length, double sourceSampleRate)
{
    ClipAudioSource *clip = new ClipAudioSource(nullptr, g_syncTimer, "", false, nullptr);
    w->clips.push_back(clip);
    w->clipFields.push_back(g_newClip);
    SamplerSynthSound *sound = new SamplerSynthSound(clip);
    g_newSound->data = new juce::AudioBuffer<float>(left, right);
    g_newSound->length = length;
    g_newSound->sourceSampleRate = sourceSampleRate;
    w->sounds.push_back(sound);
    w->soundFields.push_back(g_newSound);
    return (int)w->sounds.size() - 1;
}

/* startSeconds / stopFrames: kSliceEntries values, entry 0 for slice -1, entry s + 1 for slice s */
void zr_set_clip(zr_world *w, int index, float volumeAbsolute, float pan, float lengthInBeats, float duration, int rootMidiNote,
                 const zlo_adsr_params *adsr, const float *startSeconds, const int32_t *stopFrames)
{
    ClipFields *c = w->clipFields[(size_t)index];
    SoundFields *s = w->soundFields[(size_t)index];
    c->volumeAbsolute = volumeAbsolute; c->pan = pan; c->lengthInBeats = lengthInBeats; c->duration = duration;
    c->adsr = {adsr->attack, adsr->decay, adsr->sustain, adsr->release};
    s->rootMidiNote = rootMidiNote;
    for (int i = 0; i < kSliceEntries; ++i) { c->startPosition[i] = startSeconds[i]; s->stopPosition[i] = stopFrames[i]; }
}

void zr_set_timer(uint64_t jackPlayhead, uint64_t jackPlayheadUsecs, uint64_t jackSubbeatLengthInMicroseconds, uint64_t bpm,
                  int multiplier, float oneSubbeatInSeconds)
{
    SyncTimer_instance();
    g_timer->jackPlayhead = jackPlayhead; g_timer->jackPlayheadUsecs = jackPlayheadUsecs;
    g_timer->jackSubbeatLengthInMicroseconds = jackSubbeatLengthInMicroseconds;
    g_timer->bpm = bpm; g_timer->multiplier = multiplier; g_timer->oneSubbeatInSeconds = oneSubbeatInSeconds;
}

static SamplerSynthVoice *voiceOf(zr_world *w, int channel, int slot) { return w->voices[(size_t)(channel * w->nvoices + slot)]; }

/* the voice takes ownership of a fresh ClipCommand (it deletes a merged one through SyncTimer::deleteClipCommand) */
void zr_set_current_command(zr_world *w, int channel, int slot, const zlo_clip_command *c)
{
    ClipCommand *command = new ClipCommand();
    command->clip = (c->clip >= 0 && c->clip < (int)w->clips.size()) ? w->clips[(size_t)c->clip] : nullptr;
    command->midiNote = c->midiNote; command->midiChannel = c->midiChannel;
    command->startPlayback = c->startPlayback != 0; command->stopPlayback = c->stopPlayback != 0;
    command->changeSlice = c->changeSlice != 0; command->slice = c->slice;
    command->changeLooping = c->changeLooping != 0; command->looping = c->looping != 0;
    command->changePitch = c->changePitch != 0; command->pitchChange = c->pitchChange;
    command->changeSpeed = c->changeSpeed != 0; command->speedRatio = c->speedRatio;
    command->changeGainDb = c->changeGainDb != 0; command->gainDb = c->gainDb;
    command->changeVolume = c->changeVolume != 0; command->volume = c->volume;
    voiceOf(w, channel, slot)->setCurrentCommand(command);
}

void zr_set_start_tick(zr_world *w, int channel, int slot, uint64_t tick) { voiceOf(w, channel, slot)->setStartTick(tick); }

/* juce::Synthesiser::startVoice: the sound becomes the voice's playing sound, then startNote */
void zr_start_note(zr_world *w, int channel, int slot, int midiNote, float velocity, int sound)
{
    SamplerSynthVoice *voice = voiceOf(w, channel, slot);
    voice->setCurrentlyPlayingSound(w->sounds[(size_t)sound]);
    voice->startNote(midiNote, velocity, w->sounds[(size_t)sound], 0);
}

void zr_stop_note(zr_world *w, int channel, int slot, int allowTailOff) { voiceOf(w, channel, slot)->stopNote(0.0f, allowTailOff != 0); }

int zr_is_playing(zr_world *w, int channel, int slot) { return voiceOf(w, channel, slot)->isPlaying ? 1 : 0; }

/* one cycle of one SamplerChannel: zero both buffers, then every voice with isPlaying in voice order.  outLeft / outRight receive
 * nframes + 1 floats; reports (nvoices entries) what each voice handed to the positions model in this cycle. */
void zr_channel_process(zr_world *w, int channel, uint32_t nframes, uint64_t current_usecs, uint64_t next_usecs,
                        float *outLeft, float *outRight, zlo_report *reports)
{
    w->left.assign((size_t)nframes + 1, 0.0f);
    w->right.assign((size_t)nframes + 1, 0.0f);
    for (int i = 0; i < w->nvoices; ++i) {
        zlo_report *report = &w->reports[(size_t)(channel * w->nvoices + i)];
        *report = zlo_report{0, 0.0f, 0.0f};
        SamplerSynthVoice *voice = voiceOf(w, channel, i);
        if (voice->isPlaying) {
            g_report = report;
            voice->process(w->left.data(), w->right.data(), nframes, 0, current_usecs, next_usecs, (float)(next_usecs - current_usecs));
            g_report = nullptr;
        }
        if (reports) reports[i] = *report;
    }
    std::memcpy(outLeft, w->left.data(), sizeof(float) * ((size_t)nframes + 1));
    std::memcpy(outRight, w->right.data(), sizeof(float) * ((size_t)nframes + 1));
}

} // extern "C"
