"""bench.py's plain run on the GPU: the headline job alone, its line and its --dump-outputs, in a small configuration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    """Without --full the line holds the headline figures and the timed volume's own counters, and none of the legs, rooflines or baselines that
    --full adds; the timed volume was handed every frame of the K steps, and --dump-outputs wrote the last step's depth maps and the volume's planes."""
    steps, batch = 2, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch), "--frames", "8",
           "--voxel", "0.04", "--dump-outputs", str(tmp_path / "dump")]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 - batch) < 1e-3 * batch
    assert line["metric"].startswith("frames/sec (depth+TSDF integrate) @640x480, 128^3 vol")
    for key in ("roofline", "roofline_room", "roofline_dpt", "mesh", "cpu_baseline", "value_fp16", "small_batch", "config4", "no_overlap", "tsdf_source_stamp"):
        assert key not in line, key
    check = line["timed_volume_check"]
    assert check["frames_integrated"] == check["frames_expected"] == steps * batch
    assert check["weight_sum"] > 0 and "expected_weight_sum" not in check
    depth = np.load(tmp_path / "dump" / "depth.npy")
    assert depth.shape == (batch, 480, 640) and depth.dtype == np.float32 and np.isfinite(depth).all()
    for name in ("tsdf", "weight", "color"):
        assert np.load(tmp_path / "dump" / f"{name}.npy").shape == (128 ** 3,), name
