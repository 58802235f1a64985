"""The float64 sums that the tests elsewhere hold only within a summation bound -- the ICP normal equations (csrc/track.hip), the trajectory smoothing
(csrc/fts.hip), the pose optimiser (csrc/poseopt.hip) and the layer means of LPIPS (csrc/lpips.hip) -- against their recorded bits (tests/golden/sum_pins.npz, written by tools/record_sum_pins.py at the
commit the file names): the order of every addition is part of the interface (include/hive_mi355x.h), so a consolidation of the sum helpers must not move a bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def test_recorded_sums_bit_for_bit(gpu_ctx, oracle_lib):
    import record_sum_pins
    want = np.load(record_sum_pins.PINS)
    got = record_sum_pins.compute(gpu_ctx, oracle_lib)
    assert sorted(got) == sorted(k for k in want.files if k != "commit")
    moved = [k for k in sorted(got) if got[k].shape != want[k].shape or not np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64))]
    assert not moved, f"bits differ from commit {want['commit']}: {moved}"
    assert all(np.isfinite(v).all() for v in got.values()) and got["fts_losses"][-1] != got["fts_losses"][0]
