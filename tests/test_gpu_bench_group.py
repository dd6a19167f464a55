"""GPU: bench.py's in-process group path, the one `bench.py --gpus N` takes in one process (VERDICT r05
item 1): Runner(devices=...), mppi_group_create, member threads, solo_rate and the line's group fields.
Two members share device 0 (records exchanged by device copies); C2 size so it runs in seconds.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_group_line_fields():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--config", "c2", "--group-devices", "0,0",
           "--steps", "10", "--warmup", "2", "--prewarm-ms", "20", "--cpu-baseline-seconds", "0", "--no-c4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    c = d["config"]
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["steps"] == 10
    assert c["launcher"].startswith("one process, C-ABI group (mppi_group_create), member threads"), c["launcher"]
    assert "device-copy record exchange" in c["launcher"], c["launcher"]
    g = c["group"]
    assert g["members"] == 2 and g["devices"] == 1 and g["rccl"] == 0 and g["threaded"] == 1, g
    assert c["rccl_ranks"] == 0 and c["global_K"] == 4096 and c["k_per_gpu"] == 2048, c
    assert c["speedup_vs_1"] is not None and c["speedup_vs_1"] > 0
    # 8 leaves per member (a power of two): the group's controls equal one context's bit for bit
    assert c["group_parity_bitwise"] is True, c
    assert c["parallelism"].startswith("K-sharded over 2 members on 1 GPU(s)"), c["parallelism"]


def _plain(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "7",
           "--warmup", "2", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run carries the headline fields and none of the --full legs; --dump-outputs writes the
    last timed step's outputs and costs as float32 .npy, bitwise equal between two runs whatever
    ran before the headline pass (the second run's pre-warm is a different number of steps)."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    a = _plain(tmp_path / "a")
    _plain(tmp_path / "b", "--prewarm-ms", "5")
    assert a["steps"] == 7 and a["warmup"] == 2 and a["dtype"] == "f32" and a["higher_is_better"] is True
    # value = 1000 / ms_per_step; the line rounds ms_per_step to 1e-4 ms (0.5 % of a 0.01 ms step)
    assert a["ms_per_step"] > 0.01 and abs(a["value"] * a["ms_per_step"] / 1e3 - 1.0) < 5e-3
    for leg in ("roofline", "c4", "c4_shard", "cadence", "bilinear_roofline", "c5", "costmap_builder",
                "cpu_baseline"):
        assert leg not in a, leg
    assert a["config"]["sync_steps_per_s"] is None
    K, H = 4096, 50
    shapes = {"u1_opt": (H,), "u2_opt": (H,), "lin_vel": (H,), "ang_vel": (H,), "traj_sim": (H, 3),
              "heading_sim": (H, 3), "left_wheel_sim": (H, 3), "right_wheel_sim": (H, 3), "costs": (K,)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in shapes)
    for name, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and x.shape == shape, (name, x.dtype, x.shape)
        assert np.isfinite(x).all(), name
        assert np.array_equal(x, y), name
    assert np.abs(np.load(tmp_path / "a" / "u1_opt.npy")).max() > 0
