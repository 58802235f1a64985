"""Host side of the foreground trajectory smoothing (hive_amd/pose_optimisation.py) and the restatements its GPU tests lean on (tests/fts_restatement.py):
the chunking rule on hand-made count vectors, the command-line switches, and the float64 restatement of the loss against an independent formulation."""
import numpy as np
import pytest

import fts_restatement as F


@pytest.mark.parametrize("counts, want", [
    ([5, 5, 5], [(0, 3)]),
    ([5, 5, 0, 5, 5], []),                                   # runs of two are dropped
    ([0, 0, 0, 0], []),                                      # no run at all
    ([], []),
    ([0, 4, 4, 4, 0, 0, 1, 1, 0, 9, 9, 9, 9], [(1, 3), (9, 4)]),  # a run of two in the middle goes, the run at the end stays
    ([1] * 7, [(0, 7)]),
    ([3, 3, 3, 0, 2, 2, 2], [(0, 3), (4, 3)]),
    ([0, 1, 1, 1], [(1, 3)]),
])
def test_find_chunks_on_hand_made_counts(counts, want):
    """Maximal runs of frames with points, at least three long (pose_optimisation.py:1650-1663), as (first frame, length); equal to the restatement, which
    keeps the reference's lists of frame indices."""
    from hive_amd.pose_optimisation import find_chunks
    assert find_chunks(np.array(counts, np.int64)) == want
    assert find_chunks(counts) == want
    assert [(c[0], len(c)) for c in F.chunks_of(counts)] == want
    assert all(c == list(range(c[0], c[0] + len(c))) for c in F.chunks_of(counts))


def test_find_chunks_minimum_length_is_a_parameter():
    from hive_amd.pose_optimisation import find_chunks
    assert find_chunks([1, 1, 0, 1], min_chunk_size=2) == [(0, 2)]
    assert find_chunks([1, 1, 0, 1], min_chunk_size=1) == [(0, 2), (3, 1)]


def test_command_line_carries_both_switches():
    """``--billboard`` and ``--fts_num_epochs`` / ``--fts_learning_rate`` reach the pipeline's option groups; both are off by default."""
    from hive_amd.pipeline import Pipeline
    base = ["--dataset_path", "in", "--output_path", "out"]
    off = Pipeline.from_command_line(base)
    assert off.options.billboard is False and off.fts_options.num_epochs == 0 and off.fts_options.learning_rate == 1e-5
    on = Pipeline.from_command_line(base + ["--billboard", "--fts_num_epochs", "7", "--fts_learning_rate", "2e-5"])
    assert on.options.billboard is True and on.fts_options.num_epochs == 7 and on.fts_options.learning_rate == 2e-5


def test_jittery_case_has_three_chunks_and_frames_in_none():
    traj, centroids, counts = F.jittery_case()
    chunks = F.chunks_of(counts)
    assert [(c[0], len(c)) for c in chunks] == [(0, 20), (26, 19), (46, 14)]
    in_chunk = {i for c in chunks for i in c}
    assert traj.dtype == np.float32 and traj.shape == (60, 7) and centroids.shape == (60, 3)
    assert sorted(set(range(60)) - in_chunk) == [20, 21, 22, 23, 24, 25, 45] and counts[23] > 0 and counts[24] > 0


@pytest.mark.parametrize("relative", [1e-2, 1e-4, 1e-6])
def test_two_float64_formulations_agree_within_the_conditioning_bound(relative):
    """The yardstick of tests/test_fts_gpu.py: quaternion products against rotation matrices, both float64, loss (relative) and every gradient component
    (relative to the largest) within 16 kappa 2^-53 -- what the direction of the nearly cancelling residual gt - w loses in any float64 evaluation."""
    traj, centroids, counts = F.jittery_case()
    chunks = F.chunks_of(counts)
    start = traj.astype(np.float64)
    moved = start * (1.0 + relative * np.random.default_rng(11).standard_normal(start.shape))
    la, ga, gt, w = F.loss_and_gradient(moved, start, centroids, chunks)
    lb, gb, _, _ = F.loss_and_gradient(moved, start, centroids, chunks, world=F.world_centroids_matrix)
    tol = 16 * F.conditioning(gt, w, chunks) * F.U
    print(f"relative {relative:g}: kappa bound {tol:.3g}, loss {abs(la - lb) / abs(la):.3g}, gradient {np.abs(ga - gb).max() / np.abs(ga).max():.3g}")
    assert abs(la - lb) <= tol * abs(la)
    assert np.abs(ga - gb).max() <= tol * np.abs(ga).max()


def test_gradient_is_exactly_zero_where_the_residual_is():
    """gt is taken at the start values, so at epoch 0 every residual is exactly 0 and torch.norm's gradient there is 0: what is left is the temporal terms,
    which do not touch the quaternions."""
    traj, centroids, counts = F.jittery_case()
    start = traj.astype(np.float64)
    _, grad, gt, w = F.loss_and_gradient(start, start, centroids, F.chunks_of(counts))
    assert np.array_equal(gt, w)
    assert not grad[:, :4].any() and grad[:, 4:].any() and np.isfinite(grad).all()


def test_restated_run_float32_parameters_bound_the_float64_run():
    """The right-hand side of the whole-run check is neither zero nor large: float32 parameters (the reference) drift from the float64 run by far less than
    the parameters move, and by far more than float64 rounding."""
    traj, centroids, counts = F.jittery_case()
    chunks = F.chunks_of(counts)
    r64, l64 = F.run(traj, centroids, chunks, 1e-5, 10, "float64")
    r32, _ = F.run(traj, centroids, chunks, 1e-5, 10, "float32")
    gap, moved = np.abs(r32 - r64).max(), np.abs(r64 - traj.astype(np.float64)).max()
    assert 1e-12 < gap < 0.05 * moved
    assert l64[-1] < l64[0]
    # frames of no chunk move too: the weight decay acts on every parameter
    outside = [20, 21, 22, 23, 24, 25, 45]
    assert np.all(r64[outside] != traj.astype(np.float64)[outside])


@pytest.mark.parametrize("size", F.CENTROID_SIZES)
def test_centroid_order_shows_on_the_order_cases(size):
    """On exactly the inputs of tests/test_fts_gpu.py::test_centroids_in_the_stated_order_bit_for_bit the stated order and ``np.sum`` differ in at least one
    component: that test would see another order."""
    depth, masks, K = F.centroid_order_case(size)
    stated, counts, plain = F.centroids_ordered(depth, masks, np.linalg.inv(K))
    assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0 and not stated[1].any()
    assert (stated.view(np.uint64) != plain.view(np.uint64)).any()
    assert np.allclose(stated, plain, rtol=1e-12, atol=0.0)
