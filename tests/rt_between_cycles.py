"""A clip service called between the cycles of the resident real-time kernel (test_the_resident_kernel_stays of the loop finder and of the
key detection): the scene and the cycle loop of tests/test_loudness_gpu.py::test_the_resident_kernel_stays with "what to call between
the cycles" handed in.  ZL_RT_PERSISTENT is the caller's to set (a fixture of its own), before run() creates the engine."""
import numpy as np

from scenario import engine_cmd, random_scene, run_oracle, snapshot_clip

f32 = np.float32


def scene(seed=341):
    return random_scene(seed, num_buses=12, voices_per_bus=8, nclips=20, mode=0, nframes=128, nblocks=40)


def run(sc, extras, warm_up, between):
    """sc: the scene; extras: [(planar float32 [channels][frames], rate)], clips no voice plays, registered behind the scene's own.
    warm_up(syn, planar, rates) makes the service's first call (it allocates the call's buffers) before the first cycle;
    between(syn, k, playing, planar, rates) is called after cycle k with the clips that play (the looping ones where none is reported)
    and returns [(request, result)].  planar / rates: every clip's source and rate by id.
    Returns (audio [buses][2][frames], the oracle's audio, (rt starts after the first cycle, rt starts, rt cycles), the collected
    (request, result) pairs, planar, rates)"""
    from libzl_amd import SamplerSynth
    from oracle import zl_oracle as zo
    ref_bus, _, _ = run_oracle(sc)
    ref = zo.OracleSynth(1, 1, sc.fs, sc.mode, max_sounds=max(8, len(sc.sounds)))
    syn = SamplerSynth(num_buses=sc.num_buses, voices_per_bus=sc.voices_per_bus, mode=sc.mode, playback_sample_rate=sc.fs,
                       max_frames=max(64, sc.nframes), max_batch_blocks=4, max_sounds=max(8, len(sc.sounds) + len(extras)),
                       sound_arena_bytes=(1 << 20) + sum((s[0].shape[0] + 16) * 8 for s in sc.sounds) + sum((x.shape[1] + 16) * 8 for x, _ in extras) + (1 << 16))
    try:
        planar, rates = [], []
        for i, (L, R, sr) in enumerate(sc.sounds):
            assert ref.register_clip(L, R, sr) == i and syn.register_clip(L, R, sr) == i
            if i in sc.clip_setup:
                sc.clip_setup[i](ref.lib, ref.clips[i])
            syn.set_clip_params(i, snapshot_clip(ref.clips[i]))
            planar.append(np.stack([L, R]) if R is not None else L[None, :])
            rates.append(float(sr))
        for x, sr in extras:
            assert syn.register_clip(x[0], x[1] if x.shape[0] == 2 else None, sr) == len(planar)
            planar.append(x); rates.append(float(sr))
        warm_up(syn, planar, rates)
        N = sc.nframes
        out = np.zeros((sc.num_buses, 2, sc.nblocks * N), dtype=f32)
        starts_after_first = None
        looping = [ev[1]["clip"] for ev in sc.events[0] if ev[1].get("looping")]      # started in block 0, play to the end
        todo = []
        for k in range(sc.nblocks):
            for ev in sc.events.get(k, []):
                if ev[0] == "cmd":
                    syn.handle_clip_command(engine_cmd(**ev[1]), ev[2])
                elif ev[0] == "start":
                    syn.start_voice(ev[1], ev[2], engine_cmd(**ev[3]), ev[4])
                elif ev[0] == "clip":
                    ev[2](ref.lib, ref.clips[ev[1]])
                    syn.set_clip_params(ev[1], snapshot_clip(ref.clips[ev[1]]))
                elif ev[0] == "update":
                    syn.update_voice(ev[1], ev[2], engine_cmd(**ev[3]))
                elif ev[0] == "stopv":
                    syn.stop_voice(ev[1], ev[2], ev[3])
                elif ev[0] == "enable":
                    syn.set_bus_enabled(ev[1], ev[2])
                else:
                    raise AssertionError(ev[0])
            L, R = syn.process(N, sc.make_clocks(k, 1)[0])
            out[:, 0, k * N:(k + 1) * N] = L
            out[:, 1, k * N:(k + 1) * N] = R
            if starts_after_first is None:
                starts_after_first = syn.rt_stats()[0]
            playing = sorted({r.clip for r in syn.voice_reports() if r.playing and r.clip >= 0}) or looping
            todo += list(between(syn, k, playing, planar, rates))
        starts, cycles = syn.rt_stats()
        return out, ref_bus, (starts_after_first, starts, cycles), todo, planar, rates
    finally:
        syn.close()
