"""bench.py's plain run, --full and --dump-outputs: a plain run times the steps and nothing else, --dump-outputs writes what the
last timed step computed (float32 / float64 .npy, within 64 MB), and the same arguments render the same outputs -- with or without
--full, whose extra legs run after the dump."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--voices", "64", "--buses", "8", "--blocks-per-step", "256", "--steps", "3", "--warmup", "1"]


def test_steps_and_warmup_are_checked():
    import bench
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    a = bench.parse_args(["--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)


class _Report:
    def __init__(self, v):
        self.playing, self.gain, self.progress, self.source_sample_position = 1, 0.5, v / 64.0, v + 0.25


class _Engine:
    """The two readers dump_outputs calls, with the engine's shapes."""
    def __init__(self, KB, B, V):
        self.KB, self.B, self.V = KB, B, V

    def block_peaks(self):
        return np.arange(self.KB * self.B * 2, dtype=np.int32).reshape(self.KB, self.B, 2)

    def voice_reports(self):
        return [_Report(v) for v in range(self.V)]


@pytest.mark.parametrize("B,KB,N,fan", [(8, 8192, 256, False), (8, 64, 128, True), (128, 8200, 8, False)])
def test_dump_layout_dtypes_and_budget(tmp_path, monkeypatch, B, KB, N, fan):
    import torch
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)       # host tensors stand in for the device buffers
    g = torch.Generator().manual_seed(1)
    bus = torch.rand((B, 2, KB * N), generator=g)
    fanout = torch.rand((B, 6, KB * N), generator=g) if fan else None
    bench.dump_outputs(str(tmp_path), _Engine(KB, B, 1024), torch, bus, fanout, B, KB, N)
    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(f.endswith(".npy") and a.dtype in (np.float32, np.float64) for f, a in files.items())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    blocks = files["bus_sample_blocks.npy"].astype(np.int64)
    assert np.all(np.diff(blocks) > 0) and blocks[-1] < KB
    assert np.array_equal(files["bus_sample.npy"], bus.view(B, 2, KB, N)[:, :, blocks].numpy())
    if fan:
        assert np.array_equal(files["fanout_sample.npy"], fanout.view(B, 6, KB, N)[:, :, blocks].numpy())
    peaks = np.arange(KB * B * 2).reshape(KB, B, 2)
    if "block_peaks_blocks.npy" in files:
        assert np.array_equal(files["block_peaks_blocks.npy"], blocks) and np.array_equal(files["block_peaks.npy"], peaks[blocks])
    else:
        assert np.array_equal(files["block_peaks.npy"], peaks)
    assert files["voice_reports.npy"].shape == (1024, 4) and files["voice_reports.npy"][3, 3] == 3.25
    # the sample is fixed: a second dump of the same shapes picks the same blocks
    again = tmp_path / "again"
    bench.dump_outputs(str(again), _Engine(KB, B, 1024), torch, bus, fanout, B, KB, N)
    assert np.array_equal(np.load(again / "bus_sample_blocks.npy"), files["bus_sample_blocks.npy"])


def _bench(args, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _bench(SMALL + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] > 0 and plain["unit"] == "voice-samples/s" and plain["dtype"] == "f32" and plain["higher_is_better"] is True
    # a plain run measures nothing beyond its steps
    assert plain["value_per_gpu_repeats"] == [] and plain["output_check"] is None and "cpu_baseline" not in plain
    assert plain["roofline"]["no_reuse_variant"] is None and plain["roofline"]["device_copy_GBs"] is None

    full = _bench(SMALL + ["--full", "--no-cpu-baseline", "--no-reuse-check", "--dump-outputs", str(tmp_path / "full")])
    assert len(full["value_per_gpu_repeats"]) == 2 and full["roofline"]["device_copy_GBs"] > 0
    rows = full["output_check"]["rows_vs_oracle"]
    assert rows and all(r["bit_exact"] for r in rows)

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    assert {"bus_sample.npy", "bus_sample_blocks.npy", "block_peaks.npy", "voice_reports.npy"} <= set(names)
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), n
    bus = np.load(tmp_path / "plain" / "bus_sample.npy")
    assert bus.shape == (8, 2, 256, 256) and np.abs(bus).max() > 0
    assert np.load(tmp_path / "plain" / "voice_reports.npy")[:, 0].all()          # every voice still playing
