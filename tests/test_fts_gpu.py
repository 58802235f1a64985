"""Foreground trajectory smoothing on the GPU (csrc/fts.hip hive_fg_centroids / hive_fts_optimise, hive_amd/pose_optimisation.py) against exact sums, torch
autograd and torch.optim.Adam on the CPU (tests/fts_restatement.py), and Pipeline.run with both foreground switches on."""
import math
import os

import numpy as np
import pytest

import fts_restatement as F

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ centroids
class _Frames:
    """The part of a dataset the centroid pass reads."""

    def __init__(self, depth, masks, K):
        self.depth_dataset, self.mask_dataset, self.camera_matrix, self.num_frames = list(depth), list(masks), K, len(depth)


def _centroid_frames(h=120, w=160, n=7):
    from hive_amd import synthetic
    seq = synthetic.make_sequence(num_frames=n, height=h, width=w, yaw_step_deg=5.0)
    masks = synthetic.ellipse_masks(n, h, w, num_objects=3, seed=9)
    masks[1] = 0                      # an empty mask
    masks[2] = 0
    masks[2, 37, 91] = 2              # one pixel
    seq["depth"][2, 37, 91] = 2.75
    masks[3] = 1                      # all pixels (the invalid depths drop out)
    masks[4] = 0
    masks[4, 5, 5] = 1                # one pixel, of invalid depth: no point
    seq["depth"][4, 5, 5] = 0.0
    return seq, masks


def _assert_centroids(got, counts, depth, masks, K):
    from hive_amd import geometric
    for i in range(len(depth)):
        points = geometric.point_cloud_from_depth(depth[i], masks[i] > 0, K)
        n = len(points)
        assert counts[i] == n, i
        if n == 0:
            assert not got[i].any()
            continue
        for k in range(3):
            exact = math.fsum(points[:, k])
            # any summation order: |sum - exact| <= (n - 1) u sum|x_i|; then one rounding of the quotient
            bound = (n - 1) * F.U * math.fsum(np.abs(points[:, k])) / n + F.U * abs(exact / n)
            err = abs(got[i, k] - exact / n)
            assert err <= bound, (i, k, err, bound)


def test_centroids_against_exact_sums(gpu_ctx):
    """hive_fg_centroids == mean of point_cloud_from_depth(depth, mask > 0, K) within the bound that holds for ANY summation order, counts exact; frames with an
    empty mask, one pixel, one pixel without depth, all pixels; bit-identical from run to run."""
    import torch
    from hive_amd import pose_optimisation
    seq, masks = _centroid_frames()
    depth, K = seq["depth"], seq["K"]
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(masks).cuda()
    got, counts = pose_optimisation.centroids(d, m, K, ctx=gpu_ctx)
    assert got.shape == (7, 3) and counts.dtype == np.int64
    assert counts[1] == 0 and counts[2] == 1 and counts[4] == 0 and counts[3] == int((depth[3] > 0).sum()) and counts[0] > 100
    _assert_centroids(got, counts, depth, masks, K)
    again, counts2 = pose_optimisation.centroids(d, m, K, ctx=gpu_ctx)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and np.array_equal(counts, counts2)
    # a frame's result does not depend on its place in the batch
    one, c1 = pose_optimisation.centroids(d[5:6], m[5:6], K, ctx=gpu_ctx)
    assert np.array_equal(one[0].view(np.uint64), got[5].view(np.uint64)) and c1[0] == counts[5]


def test_centroids_at_vga_across_upload_chunks(gpu_ctx):
    """dataset_centroids at 480 x 640 (75 tiles a frame) with 5 frames through upload chunks of 2: equal to the one-batch call, within the bound."""
    import torch
    from hive_amd import pose_optimisation, synthetic
    n = 5
    seq = synthetic.make_sequence(num_frames=n, height=480, width=640, yaw_step_deg=5.0)
    masks = synthetic.ellipse_masks(n, 480, 640, num_objects=3, seed=4)
    masks[3] = 0
    data = _Frames(seq["depth"], masks, seq["K"])
    got, counts = pose_optimisation.dataset_centroids(data, chunk_frames=2, ctx=gpu_ctx)
    whole, counts_whole = pose_optimisation.centroids(torch.from_numpy(seq["depth"]).cuda(), torch.from_numpy(masks).cuda(), seq["K"], ctx=gpu_ctx)
    assert np.array_equal(got.view(np.uint64), whole.view(np.uint64)) and np.array_equal(counts, counts_whole)
    assert counts[3] == 0 and counts[0] > 10_000
    _assert_centroids(got, counts, seq["depth"], masks, seq["K"])
    assert pose_optimisation.find_chunks(counts) == [(0, 3)]


@pytest.mark.parametrize("size", F.CENTROID_SIZES)
def test_centroids_in_the_stated_order_bit_for_bit(gpu_ctx, size):
    """hive_fg_centroids == the order include/hive_mi355x.h states, restated in numpy float64 (fts_restatement.centroids_ordered), bit for bit: less than one
    wave, a full tile with a tile of 64 pixels, four tiles; a batch of three whose middle mask is empty; depths over 2^-6 .. 2^6, where
    tests/test_fts_cpu.py shows that another order gives other bits."""
    import torch
    from hive_amd import geometric, pose_optimisation
    depth, masks, K = F.centroid_order_case(size)
    want, want_counts, _ = F.centroids_ordered(depth, masks, geometric._kinv(K))
    got, counts = pose_optimisation.centroids(torch.from_numpy(depth).cuda(), torch.from_numpy(masks).cuda(), K, ctx=gpu_ctx)
    assert np.array_equal(counts, want_counts) and counts[1] == 0
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (size, got - want)


# ------------------------------------------------------------------------------------------------ loss and gradient
def _case():
    traj, centroids, counts = F.jittery_case()
    return traj, centroids, F.chunks_of(counts), [(c[0], len(c)) for c in F.chunks_of(counts)]


@pytest.mark.parametrize("relative", [1e-2, 1e-4, 1e-6])
def test_loss_and_gradient_against_autograd(gpu_ctx, relative):
    """Loss and hand-derived gradient of the kernel against torch autograd on the CPU in float64, the parameters moved away from the ones gt is taken at by
    ``relative``.  The residual gt - w is a difference of nearly equal vectors, so its direction -- and with it the gradient -- loses
    kappa = max_i (|gt_i| + |w_i|) / |gt_i - w_i| in relative accuracy in ANY float64 evaluation: tolerance 16 kappa 2^-53 on the loss (relative) and on every
    gradient component relative to the largest one (16: the handful of roundings in front of the subtraction).  tests/test_fts_cpu.py holds two independent
    float64 formulations to the same bound."""
    from hive_amd import pose_optimisation
    traj, centroids, chunks, spans = _case()
    start = traj.astype(np.float64)
    moved = start * (1.0 + relative * np.random.default_rng(11).standard_normal(start.shape))
    want_loss, want_grad, gt, w = F.loss_and_gradient(moved, start, centroids, chunks)
    tol = 16 * F.conditioning(gt, w, chunks) * F.U
    params, losses, grad = pose_optimisation.fts_optimise(moved, centroids, spans, num_epochs=0, gt_params=start, return_gradient=True, ctx=gpu_ctx)
    assert np.array_equal(params, moved) and losses.shape == (1,)
    loss_err = abs(losses[0] - want_loss) / abs(want_loss)
    grad_err = np.abs(grad - want_grad).max() / np.abs(want_grad).max()
    print(f"relative {relative:g}: tolerance {tol:.3g}, loss {loss_err:.3g}, gradient {grad_err:.3g}")
    assert loss_err <= tol
    assert grad_err <= tol
    outside = sorted(set(range(len(start))) - {i for c in chunks for i in c})
    assert not grad[outside].any()


def test_gradient_is_exactly_zero_where_the_residual_is(gpu_ctx):
    """gt taken at the parameters themselves: every residual is exactly 0, torch.norm's gradient there is 0 and so is the kernel's (no 0 / 0) -- the quaternion
    gradients are exact zeros, the translation gradients are the temporal terms alone; an all-zero difference matrix (a camera at rest) gives 0 as well."""
    from hive_amd import pose_optimisation
    traj, centroids, chunks, spans = _case()
    start = traj.astype(np.float64)
    _, losses, grad = pose_optimisation.fts_optimise(start, centroids, spans, num_epochs=0, return_gradient=True, ctx=gpu_ctx)
    want_loss, want_grad, _, _ = F.loss_and_gradient(start, start, centroids, chunks)
    assert not grad[:, :4].any() and np.isfinite(grad).all()
    # the temporal terms alone, float64 on both sides: only the summation order differs (the longest sum has 57 terms, hence 64 units)
    assert np.abs(grad - want_grad).max() <= 64 * F.U * np.abs(want_grad).max() and abs(losses[0] - want_loss) <= 64 * F.U * want_loss
    rest = start.copy()
    rest[:, 4:] = rest[0, 4:]
    _, losses, grad = pose_optimisation.fts_optimise(rest, centroids, spans, num_epochs=0, return_gradient=True, ctx=gpu_ctx)
    assert losses[0] == 0.0 and not grad.any()


# ------------------------------------------------------------------------------------------------ the whole run
@pytest.mark.parametrize("epochs", [1, 10, 100])
def test_run_is_closer_to_float64_than_the_reference_arithmetic(gpu_ctx, epochs):
    """The whole Adam loop against the float64 restatement (torch.optim.Adam on the CPU) on a jittery 60-frame trajectory with three chunks, a dropped run of two
    and frames in no chunk.  The yardstick is the reference's own arithmetic: the restatement run with float32 parameters, as the reference keeps them, and
    max|kernel - restatement64| <= max|restatement32 - restatement64| -- the kernel sits closer to exact arithmetic than the reference does.  Also: the loss after
    the last epoch is below the loss of epoch 0, frames of no chunk move (weight decay), two runs are bit-identical."""
    from hive_amd import pose_optimisation
    traj, centroids, chunks, spans = _case()
    start = traj.astype(np.float64)
    r64, l64 = F.run(traj, centroids, chunks, 1e-5, epochs, "float64")
    r32, _ = F.run(traj, centroids, chunks, 1e-5, epochs, "float32")
    got, losses = pose_optimisation.fts_optimise(start, centroids, spans, 1e-5, epochs, ctx=gpu_ctx)
    again, losses2 = pose_optimisation.fts_optimise(start, centroids, spans, 1e-5, epochs, ctx=gpu_ctx)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and np.array_equal(losses.view(np.uint64), losses2.view(np.uint64))
    ours, theirs, moved = np.abs(got - r64).max(), np.abs(r32 - r64).max(), np.abs(r64 - start).max()
    print(f"{epochs} epochs: |kernel - float64| = {ours:.3g}, |float32 - float64| = {theirs:.3g}, parameters moved {moved:.3g}")
    assert ours <= theirs
    assert losses.shape == (epochs + 1,) and losses[-1] < losses[0]
    assert abs(losses[0] - l64[0]) <= 64 * F.U * l64[0]  # the same float64 terms at the start values, summed in another order (the longest sum has 57 terms)
    outside = sorted(set(range(len(start))) - {i for c in chunks for i in c})
    assert np.all(got[outside] != start[outside])


def test_no_chunk_at_all(gpu_ctx):
    """Zero chunks.  The kernel then applies the weight decay alone (what torch.optim.Adam does with zero gradients); ForegroundPoseOptimiser.run -- where the
    reference calls backward() on a constant and raises -- logs a line and returns the input trajectory, quaternions normalised, nothing else changed."""
    from hive_amd import pose_optimisation
    from hive_amd.geometric import Trajectory
    traj, centroids, _, _ = _case()
    start = traj.astype(np.float64)
    got, losses = pose_optimisation.fts_optimise(start, np.zeros_like(centroids), [], 1e-5, 10, ctx=gpu_ctx)
    want, _ = F.run(traj, np.zeros_like(centroids), [], 1e-5, 10, "float64")
    reference, _ = F.run(traj, np.zeros_like(centroids), [], 1e-5, 10, "float32")
    assert not losses.any() and np.all(got != start)
    assert np.abs(got - want).max() <= np.abs(reference - want).max()  # the yardstick of the whole-run test

    class _Empty:
        num_frames = 4
        camera_matrix = np.array([[100.0, 0, 80], [0, 100.0, 60], [0, 0, 1]], np.float32)
        depth_dataset = [np.ones((120, 160), np.float32)] * 4
        mask_dataset = [np.zeros((120, 160), np.uint8), np.ones((120, 160), np.uint8), np.ones((120, 160), np.uint8), np.zeros((120, 160), np.uint8)]
        camera_trajectory = Trajectory(traj[:4].copy())

    optimiser = pose_optimisation.ForegroundPoseOptimiser(_Empty(), num_epochs=10)
    out = optimiser.run()
    want = traj[:4].astype(np.float64)
    want[:, :4] /= np.linalg.norm(want[:, :4], axis=1, keepdims=True)
    assert isinstance(out, Trajectory) and np.array_equal(out.values, want) and np.array_equal(_Empty.camera_trajectory.values, traj[:4])


def test_optimiser_class_equals_its_pieces(gpu_ctx):
    """ForegroundPoseOptimiser(dataset, lr, epochs).run() == centroids -> chunks -> kernel -> [q / |q|, t], from the float32 start values."""
    from hive_amd import pose_optimisation, synthetic
    from hive_amd.geometric import Trajectory
    n, h, w = 8, 120, 160
    seq = synthetic.make_sequence(num_frames=n, height=h, width=w, yaw_step_deg=3.0)
    masks = synthetic.ellipse_masks(n, h, w, num_objects=2, seed=2)
    masks[5] = 0
    data = _Frames(seq["depth"], masks, seq["K"])
    data.camera_trajectory = Trajectory(synthetic.trajectory_rows_world_to_cam(seq["poses"]))
    before = data.camera_trajectory.values.copy()
    out = pose_optimisation.ForegroundPoseOptimiser(data, learning_rate=1e-4, num_epochs=20).run()
    centroids, counts = pose_optimisation.dataset_centroids(data, ctx=gpu_ctx)
    chunks = pose_optimisation.find_chunks(counts)
    assert chunks == [(0, 5)]  # frames 6, 7: a run of two
    params, _ = pose_optimisation.fts_optimise(before.astype(np.float64), centroids, chunks, 1e-4, 20, ctx=gpu_ctx)
    want = params.copy()
    want[:, :4] = params[:, :4] / np.linalg.norm(params[:, :4], ord=2, axis=1).reshape((-1, 1))
    assert np.array_equal(out.values, want) and np.array_equal(data.camera_trajectory.values, before)
    assert np.abs(np.linalg.norm(out.values[:, :4], axis=1) - 1.0).max() <= 4 * F.U and not np.array_equal(out.values[:, 4:], before[:, 4:].astype(np.float64))


# ------------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_run_with_smoothing_and_billboards(gpu_ctx, tmp_path):
    """Pipeline.run on the TUM fixture with ellipse masks, fts num_epochs = 5 and billboard=True: nothing is listed as not applied, the smoothing is timed,
    fg/000000.ply is process_frame(..., billboard=True) with the pose ForegroundPoseOptimiser returns, bg.ply is byte-identical to a run with both off."""
    import json
    from PIL import Image
    from hive_amd import foreground, synthetic
    from hive_amd.dataset_adaptors import get_dataset
    from hive_amd.io import HiveDataset
    from hive_amd.options import BackgroundMeshOptions, ForegroundTrajectorySmoothingOptions, MeshDecimationOptions, PipelineOptions
    from hive_amd.pipeline import Pipeline
    from hive_amd.pose_optimisation import ForegroundPoseOptimiser
    from test_fgclean_gpu import read_ply
    from tum_fixture import write_tum_sequence
    tum, hive = str(tmp_path / "tum"), str(tmp_path / "hive")
    n = 3
    write_tum_sequence(tum, num_frames=n, yaw_step_deg=10.0)
    ds = get_dataset(tum, hive)
    masks = synthetic.ellipse_masks(n, ds.frame_height, ds.frame_width, num_objects=3, seed=5)
    names = sorted(os.listdir(os.path.join(hive, "mask")))
    for name, m in zip(names, masks):
        Image.fromarray(m).save(os.path.join(hive, "mask", name))
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.04, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)
    no_budget = MeshDecimationOptions(num_faces_object=-1)  # no face budget asked for: "decimation" is not listed either

    pipe = Pipeline(options=PipelineOptions(num_frames=n, billboard=True), background_mesh_options=bg_options, decimation_options=no_budget,
                    fts_options=ForegroundTrajectorySmoothingOptions(num_epochs=5))
    pipe.run(hive, str(tmp_path / "run"))
    with open(os.path.join(hive, "profiling.json")) as f:
        profiling = json.load(f)
    assert profiling["foreground_reconstruction"]["not_applied"] == []
    assert profiling["timing"]["foreground_reconstruction"]["trajectory_smoothing"] > 0
    fg = tmp_path / "run" / "mesh" / "fg"
    assert sorted(os.listdir(fg)) == sorted([f"{i:06d}.{ext}" for i in range(n) for ext in ("ply", "png")])

    data = HiveDataset(hive)
    stored = data.camera_trajectory.values.copy()
    smoothed = ForegroundPoseOptimiser(data, learning_rate=pipe.fts_options.learning_rate, num_epochs=5).run()
    assert np.array_equal(data.camera_trajectory.values, stored) and not np.array_equal(smoothed.values, stored.astype(np.float64))
    for i in (0, 1):
        want = foreground.process_frame(data.rgb_dataset[i], data.depth_dataset[i], data.mask_dataset[i], data.camera_matrix,
                                        smoothed.to_homogenous_transforms()[i], pipe.dilation_options, pipe.filtering_options, ctx=gpu_ctx,
                                        enable_cc_analysis=True, billboard=True)
        header, v, f = read_ply(str(fg / f"{i:06d}.ply"))
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), want["vertices"].cpu().numpy().astype(np.float32))
        assert np.array_equal(np.stack([v["texture_u"], v["texture_v"]], 1), want["uv"].cpu().numpy().astype(np.float32))
        assert np.array_equal(f, want["faces"].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(fg / f"{i:06d}.png")), want["texture"].cpu().numpy())
    unflattened = foreground.process_frame(data.rgb_dataset[0], data.depth_dataset[0], data.mask_dataset[0], data.camera_matrix,
                                           smoothed.to_homogenous_transforms()[0], pipe.dilation_options, pipe.filtering_options, ctx=gpu_ctx, enable_cc_analysis=True)
    _, v, _ = read_ply(str(fg / "000000.ply"))
    assert not np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), unflattened["vertices"].cpu().numpy().astype(np.float32))

    off = Pipeline(options=PipelineOptions(num_frames=n), background_mesh_options=bg_options, decimation_options=no_budget)
    off.run(hive, str(tmp_path / "run_off"))
    with open(os.path.join(hive, "profiling.json")) as f:
        profiling_off = json.load(f)
    assert profiling_off["foreground_reconstruction"]["not_applied"] == []
    assert "trajectory_smoothing" not in profiling_off["timing"]["foreground_reconstruction"]
    with open(tmp_path / "run" / "mesh" / "bg.ply", "rb") as a, open(tmp_path / "run_off" / "mesh" / "bg.ply", "rb") as b:
        assert a.read() == b.read()
    with open(fg / "000000.ply", "rb") as a, open(tmp_path / "run_off" / "mesh" / "fg" / "000000.ply", "rb") as b:
        assert a.read() != b.read()
