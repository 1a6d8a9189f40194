/* Stand-in for the seven juce_<module>/juce_<module>.h headers the reference's SamplerSynthVoice.cpp reaches.  Written from
 * what the compiler asks for.  AudioBuffer holds channel pointers; SynthesiserVoice holds the playing sound and the playback
 * rate (what juce::Synthesiser keeps there); ADSR is declared here and defined in oracle/ref_driver.cpp as a wrapper over the
 * oracle's zlo_adsr_* -- JUCE is not part of the reference tree, so the envelope is the same restatement on both sides of
 * the anchor and is NOT pinned by it.  No arithmetic in this file. */
#pragma once
#include <cmath>
#include "zl_oracle.h"

#define jassertfalse ((void) 0)
#define JUCE_DECLARE_NON_COPYABLE_WITH_LEAK_DETECTOR(ClassName) \
    ClassName(const ClassName &) = delete;                       \
    ClassName &operator=(const ClassName &) = delete;

namespace juce {

template <typename T> class AudioBuffer {
public:
    AudioBuffer(const T *left, const T *right) : channels{left, right}, numChannels(right ? 2 : 1) {}
    int getNumChannels() const noexcept { return numChannels; }
    const T *getReadPointer(int channel) const noexcept { return channels[channel]; }
private:
    const T *channels[2];
    int numChannels;
};

class ADSR {
public:
    struct Parameters { float attack, decay, sustain, release; };
    ADSR();
    void setParameters(const Parameters &newParameters);
    const Parameters &getParameters() const noexcept;
    bool isActive() const noexcept;
    void setSampleRate(double newSampleRate) noexcept;
    void reset() noexcept;
    void noteOn() noexcept;
    void noteOff() noexcept;
    float getNextSample() noexcept;
private:
    zlo_adsr state;
    Parameters parameters;
};

class SynthesiserSound {
public:
    struct Ptr {
        SynthesiserSound *object = nullptr;
        SynthesiserSound *get() const noexcept { return object; }
    };
    virtual ~SynthesiserSound() {}
    virtual bool appliesToNote(int midiNoteNumber) = 0;
    virtual bool appliesToChannel(int midiChannel) = 0;
};

class SynthesiserVoice {
public:
    virtual ~SynthesiserVoice() {}
    virtual bool canPlaySound(SynthesiserSound *) = 0;
    virtual void startNote(int midiNoteNumber, float velocity, SynthesiserSound *sound, int currentPitchWheelPosition) = 0;
    virtual void stopNote(float velocity, bool allowTailOff) = 0;
    virtual void pitchWheelMoved(int newPitchWheelValue) = 0;
    virtual void controllerMoved(int controllerNumber, int newControllerValue) = 0;
    double getSampleRate() const noexcept { return currentSampleRate; }
    SynthesiserSound::Ptr getCurrentlyPlayingSound() const noexcept { return currentlyPlayingSound; }
    /* what juce::Synthesiser (a friend in JUCE) sets on its voices */
    void setCurrentPlaybackSampleRate(double newRate) { currentSampleRate = newRate; }
    void setCurrentlyPlayingSound(SynthesiserSound *sound) { currentlyPlayingSound.object = sound; }
protected:
    void clearCurrentNote() { currentlyPlayingSound.object = nullptr; }
private:
    double currentSampleRate = 44100.0;
    SynthesiserSound::Ptr currentlyPlayingSound;
};

class SamplerVoice : public SynthesiserVoice {};

} // namespace juce
