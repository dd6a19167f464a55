"""CPU: bench.py's command line: a plain run keeps the headline pass only, --full keeps every leg, and
--dump-outputs writes float32 .npy files."""
import numpy as np

import bench

LEGS = ("no_sync_pass", "no_c4", "no_c5", "no_shard", "no_cadence", "no_bilinear", "no_costmap")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "30", "--warmup", "4")
    assert (a.gpus, a.steps, a.warmup) == (1, 30, 4)
    assert not a.full and a.dump_outputs is None
    assert a.cpu_baseline_seconds == 0 and all(getattr(a, k) for k in LEGS)


def test_full_keeps_every_leg_and_its_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.cpu_baseline_seconds > 0 and not any(getattr(a, k) for k in LEGS)
    a = _parse(monkeypatch, "--full", "--no-c5", "--cpu-baseline-seconds", "0")
    assert a.no_c5 and not a.no_c4 and a.cpu_baseline_seconds == 0


def test_dump_outputs_writes_float32_npy(tmp_path):
    arrays = {"u1_opt": np.arange(5, dtype=np.float32), "traj_sim": np.arange(12, dtype=np.float64).reshape(4, 3)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    for name, a in arrays.items():
        b = np.load(tmp_path / "d" / (name + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(b, a.astype(np.float32))
