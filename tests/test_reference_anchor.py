"""CPU tier: the C oracle against the reference's OWN SamplerSynthVoice.cpp, compiled unmodified (oracle/_ref/libzl_refvoice.so:
libzl_amd/build.py build_reference, oracle/ref_shim/, oracle/ref_driver.cpp) -- bit for bit, block by block: both buffers, the frame
the reference stores to [nframes], isPlaying, and every block's report (validity, gain, progress = sourceSamplePosition / length).

Everything else in this suite compares the engine with oracle/zl_oracle.c, oracle/np_restatement.py or goldens the numpy restatement
wrote -- all three one reading of the reference.  This module is where a mis-reading of SamplerSynthVoice::setCurrentCommand,
startNote, stopNote or process shows.  Mode 0 only (modes 1, 2, 4 are build-defined).  What it does NOT pin: juce::ADSR and the
positions model's rows (the oracle's code on both sides), ClipAudioSource / SamplerSynthSound / SyncTimer / SamplerSynth::handleCommand
(their results are handed to both sides by tests/ref_voice.py), and a negative float -> quint64 conversion (undefined in C++)."""
import numpy as np
import pytest

import reference_scenes as rs
import ref_voice as rv
from edge_scenes import SCENES
from golden_util import golden_names, load_golden
from scenario import random_scene


@pytest.fixture(scope="module")
def reflib():
    """builds the library where the reference tree is present (a failing build fails the tests); skips only where there is neither a
    tree nor a library that was built elsewhere"""
    path = rv.build()
    if path is None:
        pytest.skip("no reference tree (ZL_REFERENCE_DIR) and no oracle/_ref/libzl_refvoice.so built elsewhere")
    return path


def _anchor(reflib, sc, what, audible=True):
    out = rv.run_reference(sc, reflib)
    if audible:
        # (with one frame per block every frame goes to [nframes]: the block itself stays silent)
        assert max(np.nanmax(np.abs(out["ref"]["bus"])), np.nanmax(np.abs(out["ref"]["tail"]))) > 0, f"{what}: the reference voice rendered silence"
    rv.assert_sides_equal(out, what)
    return out


STEREO = [pytest.param(True, id="stereo"), pytest.param(False, id="mono")]


@pytest.mark.parametrize("stereo", STEREO)
def test_interior_playback_at_ratio_one(reflib, stereo):
    out = _anchor(reflib, rs.interior(stereo, notes=(60,)), "ratio 1")
    assert out["ref"]["tail"].any(), "the frame stored to [nframes] is audible here and was compared"


@pytest.mark.parametrize("stereo", STEREO)
@pytest.mark.parametrize("fs", [48000.0, 96000.0])
def test_interior_playback_pitched(reflib, stereo, fs):
    """notes 36 .. 84 against root 60, 44.1 kHz sources"""
    _anchor(reflib, rs.interior(stereo, notes=(36, 43, 48, 55, 59, 61, 67, 72, 84), sr=44100.0, fs=fs, nblocks=5 if fs == 48000.0 else 10), f"pitched at {fs}")


@pytest.mark.parametrize("stereo", STEREO)
@pytest.mark.parametrize("kind", ["ordinary", "shorter_than_a_block", "stop_beyond_the_file"])
def test_free_running_loops(reflib, stereo, kind):
    out = _anchor(reflib, rs.free_running_loops(stereo, kind), kind)
    if kind == "stop_beyond_the_file":
        bus = out["ref"]["bus"][0]
        assert (bus[:, 1500:] == 0).all(axis=0).any(), "no frame past the file's end was rendered"


@pytest.mark.parametrize("stereo", STEREO)
@pytest.mark.parametrize("nframes", [1, 33, 64, 100, 256, 1024, 4096])
def test_beat_locked_loops(reflib, stereo, nframes):
    sc = rs.beat_locked(stereo, nframes)
    ck = sc.make_clocks(0, 1)[0]
    assert ((ck.next_usecs - ck.current_usecs) % nframes != 0) == (nframes != 1), "the period per frame is meant to truncate"
    out = _anchor(reflib, sc, f"beat-locked, {nframes} frames")
    prog = out["ref"]["reports"][:, :3, 2]
    if nframes * sc.nblocks > 15000:                                    # one beat at 200 bpm is 14 400 frames
        assert (np.diff(prog, axis=0) < 0).any(axis=0)[:2].all(), "voices 0 and 1 restarted on the beat"
    else:                                                               # (1500 blocks of one frame: the restarts of the voice that starts behind the playhead)
        assert prog[2, 1] < prog[2, 0]


@pytest.mark.parametrize("stereo", STEREO)
def test_beat_locked_loops_at_44100(reflib, stereo):
    _anchor(reflib, rs.beat_locked(stereo, 256, fs=44100.0), "beat-locked at 44.1 kHz")


@pytest.mark.parametrize("stereo", STEREO)
def test_one_shots_end_by_position_release_and_envelope(reflib, stereo):
    out = _anchor(reflib, rs.one_shots(stereo), "one-shots")
    playing = out["ref"]["playing"]
    assert playing[0, :4].all() and not playing[11, :4].any(), "all four ended"
    ends = [int(np.argmin(playing[:12, v])) for v in range(4)]
    assert len(set(ends)) >= 3, f"the voices end in different blocks: {ends}"
    for v in range(4):                                                  # the block a voice ends in carries no report; nor do the blocks after it
        assert not out["ref"]["reports"][ends[v]:12, v, 0].any()


@pytest.mark.parametrize("stereo", STEREO)
def test_commands_on_playing_voices_and_stop_note(reflib, stereo):
    out = _anchor(reflib, rs.commands_on_playing_voices(stereo), "commands")
    playing = out["ref"]["playing"]
    assert playing[8, 1] and not playing[9, 1] and playing[10, 3] and not playing[11, 3]
    assert not playing[13, 0], "the loop that became a one-shot ended"
    assert playing[13, 2], "the one-shot that became a loop plays on"


@pytest.mark.parametrize("stereo", STEREO)
def test_pan_and_volume_extremes(reflib, stereo):
    _anchor(reflib, rs.pan_and_volume(stereo), "pan / volume")


@pytest.mark.parametrize("stereo", STEREO)
@pytest.mark.parametrize("kind", ["signed_zeros", "denormals", "flt_max", "infinite"])
def test_special_source_values(reflib, stereo, kind):
    out = _anchor(reflib, rs.special_source_values(stereo, kind), kind)
    if kind == "infinite":
        assert np.isnan(out["ref"]["bus"]).any() and not np.isnan(out["ref"]["bus"]).all()


@pytest.mark.parametrize("stereo", STEREO)
def test_eight_voices_sum_in_voice_order(reflib, stereo):
    out = _anchor(reflib, rs.eight_voices_one_channel(stereo), "eight voices")
    assert out["ref"]["playing"][8].sum() == 8


_SHAPES = [{}, dict(nframes=64, nblocks=30), dict(nframes=256, nblocks=10), dict(fs=44100.0), dict(voices_per_bus=2), dict(num_buses=4, nclips=12),
           dict(nframes=100), dict(nframes=33, nblocks=40)]


@pytest.mark.parametrize("seed", range(208))
def test_random_scenes(reflib, seed):
    """tests/scenario.random_scene: looping, beat-locked and one-shot clips, mono and stereo, pitched and resampled, envelopes, slices,
    stop / patch / retrigger commands, channels switched off and clip edits between blocks.  Its commands go through the restated
    handleClipCommand on both sides (tests/ref_voice.py); what differs between the sides is the voice alone."""
    kw = dict(num_buses=3, voices_per_bus=8, nframes=128, nblocks=20, nclips=10, min_len=900, max_len=4000)
    kw.update(_SHAPES[seed % len(_SHAPES)])
    _anchor(reflib, random_scene(0xF000 + seed, **kw), f"seed {seed}")


# ---- the scenes the rest of the suite already stands on, replayed through the reference voice.  Two of them start notes with
# lengthInBeats = -1 (quirk Q10): a negative float -> quint64 conversion, undefined in C++ and therefore outside the anchor.
OUTSIDE = {"negative_beats_q10", "g7_past_the_end_q10"}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_edge_scenes_through_the_reference_voice(reflib, name):
    sc = SCENES[name]()
    assert sc.mode == 0
    if name in OUTSIDE:
        with pytest.raises(rv.OutsideAnchor):
            rv.run_reference(sc, reflib)
        return
    _anchor(reflib, sc, name)


@pytest.mark.parametrize("name", [n for n in golden_names() if load_golden(n)[0].mode == 0])
def test_goldens_through_the_reference_voice(reflib, name):
    """the mode-0 goldens (written by the numpy restatement): the compiled reference voice renders the stored audio"""
    sc, ex = load_golden(name)
    if name in OUTSIDE:
        with pytest.raises(rv.OutsideAnchor):
            rv.run_reference(sc, reflib)
        return
    out = _anchor(reflib, sc, name)
    assert np.array_equal(out["ref"]["bus"].view(np.int32), ex["bus"].view(np.int32)), "the reference voice differs from the stored golden"
    V = sc.num_buses * sc.voices_per_bus
    assert np.array_equal(out["ref"]["playing"][-1], ex["state"][:V, 0].astype(np.uint8))
    last = out["ref"]["reports"][-1]
    assert np.array_equal(last[:, 0], ex["reports"][:V, 0].astype(np.float32))
    valid = last[:, 0] > 0
    assert np.array_equal(last[valid, 1:], ex["reports"][:V][valid, 1:].astype(np.float32))


def test_the_anchor_covers_every_mode_0_golden():
    assert sum(1 for n in golden_names() if load_golden(n)[0].mode == 0) >= 12


# ---- the recorded fixtures (tests/golden/ref_*.npz) cannot drift from the reference unnoticed
@pytest.mark.parametrize("name", sorted(rs.FIXTURES))
def test_committed_fixture_is_what_the_reference_voice_gives(reflib, name):
    import os
    import sys
    from golden_util import GOLDEN_DIR
    sys.path.insert(0, GOLDEN_DIR)
    import make_reference_golden as mk
    fresh = mk.record(name, rs.FIXTURES[name](), reflib)
    stored = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    assert sorted(fresh) == sorted(stored.files)
    for key, value in fresh.items():
        assert value.dtype == stored[key].dtype and value.shape == stored[key].shape, key
        assert value.tobytes() == stored[key].tobytes(), f"{name}: {key} differs from a fresh recording"


def test_every_fixture_scene_has_its_file():
    from golden_util import reference_fixture_names
    assert reference_fixture_names() == sorted(rs.FIXTURES)
