"""CPU-only checks of bench.py's argument rules, its synthetic sequence and its --dump-outputs writer (the timed job itself needs an MI355X)."""
import sys

import numpy as np
import pytest
import torch

import bench


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "0", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.steps == 3 and args.warmup == 0 and args.dump_outputs == "out"


def test_full_is_opt_in(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    assert not bench.parse_args().full  # a plain run is the headline job alone
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse_args().full


@pytest.mark.parametrize("frames, height, width, seed, yaw", [(5, 48, 64, 1234, 72.0), (9, 30, 40, 7, 2.4)])
def test_sequence_is_the_librarys(frames, height, width, seed, yaw, monkeypatch):
    """bench.make_sequence (frames on a thread pool, the seeded draws in order on the caller's thread) gives synthetic.make_sequence's arrays bit for bit,
    with as many workers as frames in flight and with one."""
    from hive_amd import synthetic
    want = synthetic.make_sequence(num_frames=frames, height=height, width=width, seed=seed, yaw_step_deg=yaw)
    for threads in ("3", "1"):
        monkeypatch.setenv("HIVE_BENCH_CPU_THREADS", threads)
        got = bench.make_sequence(frames, height, width, seed=seed, yaw_step_deg=yaw)
        assert sorted(got) == sorted(want)
        for key, a in want.items():
            assert got[key].dtype == a.dtype and np.array_equal(got[key], a), (threads, key)


def test_dump_outputs_writes_a_fixed_float32_sample(tmp_path, monkeypatch):
    assert 4 * bench.DUMP_VALUES * 4 + 4 * 128 <= 64 * 10 ** 6  # four float32 arrays (and their .npy headers) stay within 64 MB
    monkeypatch.setattr(bench, "DUMP_VALUES", 1000)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)

    class Volume:
        def device_tensors(self):  # (tsdf, weight, colour) planes, told apart by an offset
            return tuple(torch.arange(5000, dtype=torch.float32) + k for k in range(3))

    depth = torch.rand(2, 12, 16)  # 384 values: written whole
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), depth, Volume())
    got = {name: np.load(tmp_path / "a" / f"{name}.npy") for name in ("depth", "tsdf", "weight", "color")}
    for name, a in got.items():
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy")), name
    assert np.array_equal(got["depth"], depth.numpy())
    tsdf = got["tsdf"]
    assert 900 < tsdf.size <= 1000 and np.all(np.diff(tsdf) > 0)  # sorted, distinct voxel indices
    assert np.array_equal(got["weight"] - 1, tsdf) and np.array_equal(got["color"] - 2, tsdf)  # one draw for the three planes
