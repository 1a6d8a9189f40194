"""Scenes for the reference anchor (tests/test_reference_anchor.py) and for the recorded reference fixtures
(tests/golden/make_reference_golden.py -> tests/golden/ref_*.npz): each builds a scenario.Scene in mode 0 around one statement
of SamplerSynthVoice.cpp that a restatement could mis-read.  Every builder takes `stereo`: the same scene on two-channel and on
mono sources (the mono `r = l` fall-through of :205)."""
import numpy as np

from scenario import Scene, play_cmd, rand_source, stop_cmd

FLT_MAX = np.finfo(np.float32).max


def _scene(seed, *, stereo, nsounds=1, length=6000, sr=48000.0, fs=48000.0, nframes=128, nblocks=10, vpb=8, buses=1, bpm=120):
    rng = np.random.default_rng(seed)
    sc = Scene(num_buses=buses, voices_per_bus=vpb, fs=fs, nframes=nframes, nblocks=nblocks, bpm=bpm)
    for i in range(nsounds):
        L, R = rand_source(rng, length + 37 * i, stereo=stereo)
        sc.sounds.append((L, R, sr))
    return sc


def _clip(sc, i, *, beats=7.3, seconds=None, start=None, vol=None, pan=None, adsr=None, root=None):
    """clip fields, written straight into the oracle's clip struct (seconds None: the whole file)"""
    def setup(lib, clip):
        clip.lengthInBeats = beats
        if seconds is not None:
            clip.lengthInSeconds = float(np.float32(seconds))
        if start is not None:
            clip.startPositionInSeconds = float(np.float32(start))
        if vol is not None:
            clip.volumeAbsolute = vol
        if pan is not None:
            clip.pan = pan
        if root is not None:
            clip.rootNote = root
        if adsr is not None:
            clip.adsr.p.attack, clip.adsr.p.decay, clip.adsr.p.sustain, clip.adsr.p.release = adsr
    sc.clip_setup[i] = setup


def interior(stereo, notes=(60,), sr=48000.0, fs=48000.0, nframes=128, nblocks=6, length=9000):
    """playback inside the file, no wrap and no end: the two-tap expression of :204-205, `++leftBuffer` before the store (:218-221),
    pow(2, (note - root) / 12) * sourceRate / playbackRate (:115-116)"""
    sc = _scene(0xA100 + len(notes), stereo=stereo, nsounds=len(notes), length=length, sr=sr, fs=fs, nframes=nframes, nblocks=nblocks)
    for i, note in enumerate(notes):
        _clip(sc, i, vol=0.5 + 0.1 * (i % 5), pan=-0.6 + 0.3 * (i % 5))
    sc.events[0] = [("cmd", play_cmd(i, loop=True, note=note, volume=0.9 - 0.1 * (i % 4)), 0) for i, note in enumerate(notes)]
    return sc


def free_running_loops(stereo, kind):
    """non-integer lengthInBeats: `sourceSamplePosition >= stopPosition` (:243) and the (int) truncation of the restart (:246)"""
    if kind == "ordinary":
        sc = _scene(0xA200, stereo=stereo, nsounds=3, nblocks=14)
        for i in range(3):
            _clip(sc, i, beats=0.37 + 0.1 * i, seconds=0.03 + 0.007 * i, start=0.004 * i, vol=0.8, pan=0.3 * (i - 1))
    elif kind == "shorter_than_a_block":
        sc = _scene(0xA201, stereo=stereo, nsounds=3, nblocks=8)
        for i, frames in enumerate((3, 40, 97)):
            _clip(sc, i, beats=0.013, seconds=frames / 48000.0, start=0.001 * i, vol=0.7, pan=0.2)
    else:                                                               # the stop position lies beyond the file: `sampleDuration > pos` false -> l = 0, r = l
        assert kind == "stop_beyond_the_file"
        sc = _scene(0xA202, stereo=stereo, nsounds=3, length=1500, nblocks=14)
        for i in range(3):
            _clip(sc, i, beats=0.3, seconds=0.05 + 0.01 * i, vol=0.9, pan=-0.4)
    sc.events[0] = [("cmd", play_cmd(i, loop=True, note=(60, 67, 53)[i], volume=0.6 + 0.1 * i), 0) for i in range(3)]
    return sc


def beat_locked(stereo, nframes, fs=48000.0, length=9000):
    """integer lengthInBeats against a moving playhead: nextLoopTick (:123), the u64 difference to the playhead (:180-181, :236-237) --
    one voice starts with a tick 200 behind it, so the difference wraps --, the INTEGER division (next_usecs - current_usecs) / nframes
    (:183; at 48 kHz the period is 20.8 us per frame and truncates to 20 for every block size but 1) and jack_time_t(frame * that) (:232)"""
    nblocks = max(6, min(1500, 20000 // nframes))
    sc = _scene(0xA300 + nframes, stereo=stereo, nsounds=3, length=length, fs=fs, nframes=nframes, nblocks=nblocks, bpm=200)
    sc.moving_playhead, sc.block0 = True, 9000 * max(1, 128 // nframes)    # a timer that has been running for 24 s: playhead ~ 7700
    for i in range(3):
        _clip(sc, i, beats=float(1 + (i == 2)), seconds=0.04 + 0.01 * i, vol=0.8, pan=0.25 * (i - 1))
    t = sc.tick_at
    assert t(0) > 1000
    sc.events[0] = [("cmd", play_cmd(0, note=60, volume=0.8), t(0)), ("cmd", play_cmd(1, note=64, volume=0.7), t(0) - 200)]
    sc.events[min(3, nblocks - 1)] = [("cmd", play_cmd(2, note=57, volume=0.6), t(min(3, nblocks - 1)) + 30)]
    return sc


def one_shots(stereo):
    """not looping: the end by position (:249-252), by release -- `stopPosition - release * rate` crossed and noteOff repeated in every
    frame from there (:253-256) --, by `!adsr.isActive()` after a stop command's release ran out (:258-261) and after a noteOff with
    release 0; then the blocks after each stop (voice silent, no report)"""
    sc = _scene(0xA400, stereo=stereo, nsounds=4, length=3000, nblocks=16)
    _clip(sc, 0, beats=0.21, seconds=0.0263, adsr=(0.0, 0.1, 1.0, 0.0))                    # 1262 frames, ends inside block 9 by position
    _clip(sc, 1, beats=0.23, seconds=0.02, adsr=(0.0, 0.1, 1.0, 0.004), pan=0.4)           # release of 192 frames before the stop position
    _clip(sc, 2, beats=0.31, seconds=0.05, adsr=(0.002, 0.003, 0.7, 0.003), pan=-0.5)      # stopped by a command at block 3: release 144 frames
    _clip(sc, 3, beats=0.33, seconds=0.05, adsr=(0.0, 0.1, 1.0, 0.0), vol=0.6)             # stopped by a command with release 0
    sc.events[0] = [("cmd", play_cmd(i, loop=False, note=(60, 62, 57, 65)[i], volume=0.9 - 0.1 * i), 0) for i in range(4)]
    sc.events[3] = [("cmd", stop_cmd(2, note=57), 0)]
    sc.events[5] = [("cmd", stop_cmd(3, note=65), 0)]
    sc.events[12] = [("cmd", play_cmd(1, loop=False, note=55, volume=1.0), 0)]              # a freed slot is taken again
    return sc


def commands_on_playing_voices(stereo):
    """every branch of setCurrentCommand on a playing voice (:60-93): changeLooping both ways, changeVolume, the stored-only
    changePitch / changeSpeed / changeGainDb, changeSlice, startPlayback = restart (alone and with changeSlice); then
    stopNote(true) followed by stopNote(false) (:146-169)"""
    sc = _scene(0xA500, stereo=stereo, nsounds=4, length=5000, nblocks=14, vpb=6)
    _clip(sc, 0, beats=0.37, seconds=0.03, adsr=(0.0, 0.1, 1.0, 0.004), pan=-0.2)
    _clip(sc, 1, beats=0.41, seconds=0.05, adsr=(0.002, 0.003, 0.7, 0.006), pan=0.3)
    _clip(sc, 2, beats=0.29, seconds=0.09, adsr=(0.0, 0.1, 1.0, 0.002))
    _clip(sc, 3, beats=0.43, seconds=0.1, vol=0.7)                                         # 16 slices (the constructor's table)
    sc.events[0] = [("start", 0, 0, play_cmd(0, note=60, volume=0.8), 0), ("start", 0, 1, play_cmd(1, note=64, volume=0.7), 0),
                    ("start", 0, 2, play_cmd(2, loop=False, note=62, volume=0.9), 0),
                    ("start", 0, 3, play_cmd(3, note=57, volume=0.6, changeSlice=1, slice=2), 0)]
    base = lambda clip, note: dict(clip=clip, midiChannel=-2, midiNote=note)
    sc.events[2] = [("update", 0, 0, dict(base(0, 60), changeLooping=1, looping=0)), ("update", 0, 2, dict(base(2, 62), changeLooping=1, looping=1))]
    sc.events[3] = [("update", 0, 1, dict(base(1, 64), changeVolume=1, volume=0.25)),
                    ("update", 0, 1, dict(base(1, 64), changePitch=1, pitchChange=0.5, changeSpeed=1, speedRatio=1.5, changeGainDb=1, gainDb=-6.0))]
    sc.events[4] = [("update", 0, 3, dict(base(3, 57), changeSlice=1, slice=5))]
    sc.events[5] = [("update", 0, 3, dict(base(3, 57), startPlayback=1)), ("update", 0, 1, dict(base(1, 64), changeSlice=1, slice=3, startPlayback=1)),
                    ("update", 0, 4, dict(base(0, 60), changeVolume=1, volume=0.1))]       # slot 4 does not play
    sc.events[7] = [("update", 0, 2, dict(base(2, 62), changeVolume=1, volume=0.0))]        # command volume 0
    sc.events[8] = [("stopv", 0, 1, True)]
    sc.events[9] = [("stopv", 0, 1, False)]
    sc.events[11] = [("stopv", 0, 3, False), ("stopv", 0, 5, True)]                         # slot 5 does not play
    return sc


def pan_and_volume(stereo):
    """pan at -1, 0, 1 and beyond (:192-194, :207-211), clipVolume 0 and 1 (:189), command volume 0 (:131-132)"""
    rows = [(-1.0, 1.0, 0.8), (0.0, 1.0, 0.7), (1.0, 1.0, 0.9), (2.5, 0.6, 0.5), (-3.0, 0.8, 1.0), (0.3, 0.0, 0.9), (-0.3, 1.0, 0.0), (0.7, 0.0, 0.0)]
    sc = _scene(0xA600, stereo=stereo, nsounds=len(rows), length=4000, nblocks=6)
    for i, (pan, vol, _) in enumerate(rows):
        _clip(sc, i, beats=0.37, seconds=0.02 + 0.003 * i, pan=pan, vol=vol)
    sc.events[0] = [("cmd", play_cmd(i, loop=True, note=57 + i, volume=rows[i][2]), 0) for i in range(len(rows))]
    return sc


def special_source_values(stereo, kind):
    """source values at the edges of the format through :204-221.  `infinite` meets inf - inf in the M/S matrix: NaN frames, compared as
    "NaN in the same frames"."""
    sc = _scene(0xA700, stereo=stereo, nsounds=3, length=3000, nblocks=6)
    rng = np.random.default_rng(0xA701)
    for i, (L, R, sr) in enumerate(sc.sounds):
        for x in (L, R):
            if x is None:
                continue
            at = rng.integers(0, x.size, 400)
            if kind == "signed_zeros":
                x[:] = np.where(rng.random(x.size) < 0.5, np.float32(0.0), np.float32(-0.0)); x[at[:40]] = np.float32(0.5)
            elif kind == "denormals":
                x[at] = (rng.uniform(-1, 1, at.size) * 1e-39).astype(np.float32); x[at[:50]] = np.float32(1.4e-45)
            elif kind == "flt_max":
                x[at[:200]] = FLT_MAX; x[at[200:]] = -FLT_MAX
            else:
                assert kind == "infinite"
                x[at[:100]] = np.inf; x[at[100:200]] = -np.inf; x[at[200:260]] = np.nan
        _clip(sc, i, beats=0.37, seconds=0.025 + 0.004 * i, vol=0.9, pan=0.4 * (i - 1))
    sc.events[0] = [("cmd", play_cmd(i, loop=True, note=(60, 66, 55)[i], volume=0.8), 0) for i in range(3)]
    return sc


def eight_voices_one_channel(stereo):
    """SamplerSynth.cpp:134-140: eight voices of one channel, started in different blocks, accumulate into the bus in voice order"""
    sc = _scene(0xA800, stereo=stereo, nsounds=8, length=4000, nblocks=14)
    for i in range(8):
        _clip(sc, i, beats=0.37 if i % 3 else 1.0, seconds=0.02 + 0.005 * i, vol=0.5 + 0.06 * i, pan=-0.7 + 0.2 * i, adsr=(0.001 * i, 0.002, 0.8, 0.003))
    for i in range(8):
        sc.events.setdefault(i, []).append(("cmd", play_cmd(i, loop=(i != 5), note=55 + 2 * i, volume=0.9 - 0.05 * i), 0))
    sc.events.setdefault(10, []).append(("cmd", stop_cmd(2, note=59), 0))
    return sc


# ---- the fixture subset: a dozen scenes that cover every group above once (tests/golden/ref_*.npz); sources kept short
FIXTURES = {
    "ref_01_interior_unit_ratio": lambda: interior(True, notes=(60,), length=2000),
    "ref_02_interior_pitched_mono": lambda: interior(False, notes=(36, 55, 61, 72, 84), sr=44100.0, length=4000),
    "ref_03_interior_pitched_96k": lambda: interior(True, notes=(48, 67, 84), sr=44100.0, fs=96000.0, nframes=256, nblocks=4, length=3000),
    "ref_04_free_loops_short_and_beyond": lambda: _join(free_running_loops(True, "shorter_than_a_block"), free_running_loops(True, "stop_beyond_the_file")),
    "ref_05_free_loops_mono": lambda: _join(free_running_loops(False, "ordinary"), free_running_loops(False, "stop_beyond_the_file")),
    "ref_06_beat_locked_100": lambda: beat_locked(True, 100, length=3000),
    "ref_07_beat_locked_64_mono": lambda: beat_locked(False, 64, length=3000),
    "ref_08_one_shots": lambda: one_shots(True),
    "ref_09_commands": lambda: commands_on_playing_voices(True),
    "ref_10_pan_and_volume": lambda: pan_and_volume(False),
    "ref_11_special_values": lambda: _join(special_source_values(True, "signed_zeros"), special_source_values(False, "denormals"), special_source_values(True, "flt_max")),
    "ref_12_eight_voices": lambda: eight_voices_one_channel(True),
}


def _join(*scenes):
    """several one-channel scenes of one shape side by side: scene j becomes channel j (its clips renumbered, its commands readdressed)"""
    a = scenes[0]
    out = Scene(num_buses=len(scenes), voices_per_bus=a.voices_per_bus, fs=a.fs, nframes=a.nframes, nblocks=min(s.nblocks for s in scenes), bpm=a.bpm)
    for j, s in enumerate(scenes):
        assert (s.num_buses, s.fs, s.nframes, s.voices_per_bus, s.moving_playhead) == (1, a.fs, a.nframes, a.voices_per_bus, False)
        base = len(out.sounds)
        out.sounds.extend(s.sounds)
        for i, fn in s.clip_setup.items():
            out.clip_setup[base + i] = fn
        for k, evs in s.events.items():
            for ev in evs:
                assert ev[0] == "cmd"
                out.events.setdefault(k, []).append(("cmd", dict(ev[1], clip=ev[1]["clip"] + base, midiChannel=j - 2), ev[2]))
    return out
