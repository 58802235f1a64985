"""The PoseOptimiser loop on the GPU (csrc/poseopt.hip hive_pose_optimise / hive_pose_project behind hive_amd.pose_optimisation) against torch autograd,
torch.optim.Adam, torch's ReduceLROnPlateau and the numpy statement of the projection (tests/pose_optimiser_restatement.py).  tests/test_pose_optimiser_cpu.py
proves the conditions on the cases that these tests lean on."""
import os

import numpy as np
import pytest

import pose_optimiser_restatement as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(name="common"):
    return _once(("case", name), {"common": R.make_case, "constrained": R.constrained_case}[name])


def _feature_set(case):
    import torch
    from hive_amd.pose_optimisation import FeatureData, FeatureSet
    side = lambda s: FeatureData(torch.from_numpy(case["index_" + s]), torch.from_numpy(case["points_" + s]), torch.from_numpy(case["depth_" + s]))
    return FeatureSet(torch.from_numpy(R.camera_matrix(case)), side("i"), side("j")).to("cuda")


def _parameters(case, affine=False, poses=None):
    from hive_amd.pose_optimisation import AlignmentType, OptimisationParameters
    poses = case["start"].astype(np.float64) if poses is None else poses
    if not affine:
        return OptimisationParameters(poses, AlignmentType.Rigid)
    rng = np.random.default_rng(3)
    n = len(poses)
    return OptimisationParameters(poses, AlignmentType.Affine, 1.0 + 0.05 * rng.standard_normal(n), 0.01 * rng.standard_normal(n))


def _options(**kw):
    from hive_amd.pose_optimisation import OptimisationOptions
    return OptimisationOptions(**kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _kinds(residual, affine):
    from hive_amd.pose_optimisation import AlignmentType, ResidualType
    return ResidualType[residual], AlignmentType.Affine if affine else AlignmentType.Rigid


# ------------------------------------------------------------------------------------------------ 1. loss and gradient
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("residual", ["World3D", "Image2D"])
def test_loss_and_gradient_against_autograd(gpu_ctx, residual, affine, smooth):
    """num_epochs = 0: loss and hand-derived gradient at the raw start parameters of the common case against torch autograd on the CPU in float64.

    The tolerance, derived.  A residual ends in a subtraction a - b of nearly equal vectors (two world points, or a pixel and a projection); its direction, and so
    the correspondence's gradient term, loses kappa = max_k (|a_k| + |b_k|) / |a_k - b_k| in relative accuracy in ANY float64 evaluation: 16 kappa u per term (16:
    the handful of roundings in front of the subtraction, the yardstick of tests/test_fts_gpu.py).  A frame's gradient component is the sum of L such terms
    (L <= the longest incidence list + 16 regulariser terms), which any summation order computes within (L - 1) u of the sum of their magnitudes.  So
    |got - want| <= 2 (16 kappa + L) u S per component, S = sum_k |d(|r_k| / M) / dtheta| + |d regularisers / dtheta| from autograd's per-correspondence
    Jacobian -- for a quaternion component the parts of (G_j - u_j (u . G)) / |q| in place of the result, which cancels where u is near an axis
    (pose_optimiser_restatement.gradient_term_magnitudes); the 2 because autograd carries the same error.  The loss is a sum of M norms, each within 16 kappa u: relative 2 (16 kappa + M) u."""
    from hive_amd import pose_optimisation as P
    case, n = _case(), _case()["n"]
    residual_type, _ = _kinds(residual, affine)
    params = _parameters(case, affine)
    scale, shift = (params.scale, params.shift) if affine else (np.ones(n), np.zeros(n))
    want_loss, want_grad = R.loss_and_gradient(params.poses(), scale, shift, case, residual, affine, smooth)
    magnitude = R.gradient_term_magnitudes(params.poses(), scale, shift, case, residual, affine, smooth)
    kappa = R.conditioning(params.poses(), scale, shift, case, residual, affine)
    longest = int(np.bincount(np.concatenate([case["index_i"], case["index_j"]])).max()) + 16
    out, losses, rates, ran, loss, grad = P.optimise_poses(_feature_set(case), params, _options(), residual_type, smooth, fps=case["fps"], num_epochs=0,
                                                            return_gradient=True, ctx=gpu_ctx)
    assert ran == 0 and len(losses) == 0 and len(rates) == 0 and np.array_equal(out.poses(), params.poses())
    loss_tol = 2 * (16 * kappa + len(case["index_i"])) * R.U
    grad_tol = 2 * (16 * kappa + longest) * R.U * magnitude
    loss_err, worst = abs(loss - want_loss) / want_loss, float(np.max(np.abs(grad - want_grad) / np.maximum(grad_tol, 1e-300)))
    print(f"{residual} affine={affine} smooth={smooth}: kappa {kappa:.3g}, loss error {loss_err:.3g} (tolerance {loss_tol:.3g}), gradient error / tolerance {worst:.3g}, "
          f"largest |gradient error| {np.abs(grad - want_grad).max():.3g} of {np.abs(want_grad).max():.3g}")
    assert loss_err <= loss_tol
    assert np.all(np.abs(grad - want_grad) <= grad_tol)
    if not affine:
        assert not grad[:, 7:].any()


# ------------------------------------------------------------------------------------------------ 2. exact zeros
def test_exact_zeros(gpu_ctx):
    """Frame 0's pose gradient is exactly 0; with position_only every rotation gradient is; the frame in no pair (7) gets the regularisers' gradient alone --
    exactly 0 without them; correspondences whose residual is exactly 0 (both sides the same pixel and depth under the same pose) give 0, not NaN."""
    from hive_amd import pose_optimisation as P
    case = _case()
    fs, params = _feature_set(case), _parameters(case)
    run = lambda options, smooth, f=fs, p=params: P.optimise_poses(f, p, options, smooth_trajectory=smooth, fps=case["fps"], num_epochs=0, return_gradient=True, ctx=gpu_ctx)
    *_, grad = run(_options(), True)
    assert not grad[0, :7].any() and np.isfinite(grad).all() and np.all(grad[1:, :7] != 0.0)
    *_, grad = run(_options(position_only=True), True)
    assert not grad[:, :4].any() and not grad[0].any() and np.all(grad[1:, 4:7] != 0.0)
    *_, grad = run(_options(), False)
    assert not grad[7].any() and np.all(grad[[6, 8], :7] != 0.0)
    *_, smooth_grad = run(_options(), True)
    _, want = R.loss_and_gradient(params.poses(), np.ones(12), np.zeros(12), case, smooth=True)  # frame 7 has no correspondence: its row is the regularisers' alone
    assert np.abs(smooth_grad[7] - want[7]).max() <= 64 * R.U * np.abs(want[7]).max()  # a dozen terms, float64 on both sides
    # residuals that are exactly 0: every pose the same, side j a copy of side i
    same = dict(case, index_j=case["index_j"], points_j=case["points_i"], depth_j=case["depth_i"])
    poses = np.tile(params.poses()[3], (12, 1))
    out = P.optimise_poses(_feature_set(same), _parameters(case, poses=poses), _options(), smooth_trajectory=False, fps=case["fps"], num_epochs=0, return_gradient=True,
                           ctx=gpu_ctx)
    assert out[4] == 0.0 and not out[5].any()


# ------------------------------------------------------------------------------------------------ 3. the projection
@pytest.mark.parametrize("n", [2, 3, 70, 1100])
def test_projection_is_the_stated_order_bit_for_bit(gpu_ctx, n):
    """hive_pose_project == the numpy statement of the stated order, bit for bit: raw quaternions of any length normalised, positions clipped with steps below,
    exactly at and above the limit and runs of consecutive violations (tests/pose_optimiser_restatement.clip_trajectory).  Against the reference's literal loop
    (clip a frame, shift every later frame): both compute t_0 + sum of the clipped differences; either carries at most 4 roundings a frame (difference,
    scaling, sum; the literal one a shift), each within u max|t|, and a frame has at most N frames before it: |stated - literal| <= 8 N u max|t|."""
    from hive_amd import pose_optimisation as P
    limit = 0.25
    poses, kinds = R.clip_trajectory(n, limit)
    got = P.project_poses(poses, limit, ctx=gpu_ctx)
    want = np.hstack((R.normalise_rows(poses[:, :4]), R.clip_stated(poses[:, 4:], limit)))
    assert _bits(got) == _bits(want)
    steps = np.linalg.norm(np.diff(got[:, 4:], axis=0), axis=1)
    assert steps.max() <= limit + 8 * R.U * np.abs(got[:, 4:]).max() and ("above" not in kinds or not np.array_equal(got[:, 4:], poses[:, 4:]))
    literal = R.clip_literal(poses[:, 4:], limit)
    bound = 8 * n * R.U * max(np.abs(poses[:, 4:]).max(), np.abs(literal).max())
    print(f"N = {n}: {kinds}, |stated - literal| = {np.abs(got[:, 4:] - literal).max():.3g}, bound {bound:.3g}")
    assert np.abs(got[:, 4:] - literal).max() <= bound
    # no clip asked for, or nothing to clip: the positions come back as they went in
    assert _bits(P.project_poses(poses, None, ctx=gpu_ctx)[:, 4:]) == _bits(poses[:, 4:])
    assert _bits(P.project_poses(poses, 10.0, ctx=gpu_ctx)[:, 4:]) == _bits(poses[:, 4:])


# ------------------------------------------------------------------------------------------------ 4. the whole run
def _restated(case, epochs, dtype, **kw):
    return _once(("run", id(case), epochs, dtype, tuple(sorted(kw.items()))), lambda: R.run(case, epochs, dtype=dtype, max_frame_distance=1.0 / case["fps"], **kw))


@pytest.mark.parametrize("epochs", [1, 10, 50])
def test_run_is_closer_to_float64_than_the_reference_arithmetic(gpu_ctx, epochs):
    """The projected Adam loop on the common case (default options, World3D, smoothing terms, clip at 1 / 30 m) against the float64 restatement with
    torch.optim.Adam.  The yardstick is the reference's own arithmetic, float32 parameters: max|kernel - restatement64| <= max|restatement32 - restatement64|.
    Two runs give the same bits, and so do check_every = 1, 7 and a value above the epoch count."""
    from hive_amd import pose_optimisation as P
    case = _case()
    fs, params = _feature_set(case), _parameters(case)
    r64, l64, _, _ = _restated(case, epochs, "float64")
    r32, _, _, _ = _restated(case, epochs, "float32")
    runs = [P.optimise_poses(fs, params, _options(), fps=case["fps"], num_epochs=epochs, check_every=c, ctx=gpu_ctx) for c in (64, 64, 1, 7, epochs + 5)]
    got, losses, rates, ran = runs[0]
    for other in runs[1:]:
        assert _bits(other[0].poses()) == _bits(got.poses()) and _bits(other[1]) == _bits(losses) and _bits(other[2]) == _bits(rates) and other[3] == ran
    ours, theirs, moved = np.abs(got.poses() - r64[:, :7]).max(), np.abs(r32 - r64).max(), np.abs(r64[:, :7] - case["start"]).max()
    print(f"{epochs} epochs: |kernel - float64| = {ours:.3g}, |float32 - float64| = {theirs:.3g}, parameters moved {moved:.3g}, loss {losses[0]:.4g} -> {losses[-1]:.4g}")
    assert ran == epochs and losses.shape == rates.shape == (epochs,)
    assert ours <= theirs
    assert np.abs(losses - l64).max() <= np.abs(_restated(case, epochs, "float32")[1] - l64).max()
    assert np.all(rates == 1e-2)


@pytest.mark.parametrize("residual,affine", [("Image2D", False), ("World3D", True), ("Image2D", True)])
def test_other_residuals_and_alignments_run_closer_to_float64_too(gpu_ctx, residual, affine):
    """Ten epochs of the same yardstick for Image2D and for Affine alignment (scale and shift start at 1 and 0, as the reference starts them)."""
    from hive_amd import pose_optimisation as P
    case = _case()
    residual_type, alignment = _kinds(residual, affine)
    params = P.OptimisationParameters(case["start"].astype(np.float64), alignment)
    r64 = _restated(case, 10, "float64", residual_type=residual, affine=affine)[0]
    r32 = _restated(case, 10, "float32", residual_type=residual, affine=affine)[0]
    got, losses, _, ran = P.optimise_poses(_feature_set(case), params, _options(alignment_type=alignment), residual_type, fps=case["fps"], num_epochs=10, ctx=gpu_ctx)
    mine = np.hstack((got.poses(), got.scale[:, None], got.shift[:, None])) if affine else got.poses()
    ours, theirs = np.abs(mine - r64[:, :mine.shape[1]]).max(), np.abs(r32 - r64).max()
    print(f"{residual} affine={affine}: |kernel - float64| = {ours:.3g}, |float32 - float64| = {theirs:.3g}")
    assert ran == 10 and ours <= theirs and (not affine or np.sum(got.scale != 1.0) >= 10)


def test_first_adam_step_is_the_learning_rate_along_the_sign(gpu_ctx):
    """Adam's first step is lr g / (|g| + eps): from the projected start, every unpinned component moves by lr against the sign of its gradient, short of lr by the
    relative eps / |g| (+ a few roundings), the pinned ones stay bit for bit.  The common case has no unpinned gradient component below 1e-6 of the largest
    (tests/test_pose_optimiser_cpu.py asserts it: the smallest is 1.4e-5 of the largest), so no component's direction hangs on rounding."""
    from hive_amd import pose_optimisation as P
    case = _case()
    fs = _feature_set(case)
    start = P.project_poses(case["start"].astype(np.float64), 1.0 / case["fps"], ctx=gpu_ctx)
    params = _parameters(case, poses=start)
    *_, grad = P.optimise_poses(fs, params, _options(), fps=case["fps"], num_epochs=0, return_gradient=True, ctx=gpu_ctx)
    got, _, _, _ = P.optimise_poses(fs, params, _options(), fps=case["fps"], num_epochs=1, ctx=gpu_ctx)
    delta, g = got.poses() - start, grad[:, :7]
    assert _bits(got.poses()[0]) == _bits(start[0])
    assert np.all(np.sign(delta[1:]) == -np.sign(g[1:]))
    assert np.all(np.abs(np.abs(delta[1:]) - 1e-2) <= 1e-2 * (1e-8 / np.abs(g[1:]) + 64 * R.U))


# ------------------------------------------------------------------------------------------------ 5. scheduler and stop
def test_scheduler_and_early_stop_replay_exactly(gpu_ctx):
    """A run with small patiences (5 and 20) that lowers the learning rate at least twice and stops early.  The kernel's OWN returned losses, replayed through
    torch's ReduceLROnPlateau and the EarlyStopping rule on the CPU, give exactly the returned learning rates and epochs_run -- independent of how sensitive the
    trajectory is.  The same with check_every = 1 and 1000: the same bits."""
    from hive_amd import pose_optimisation as P
    case = _case("constrained")
    options = _options(num_epochs=2000, lr_scheduler_patience=5, early_stopping_patience=20)
    fs, params = _feature_set(case), _parameters(case)
    got, losses, rates, ran = P.optimise_poses(fs, params, options, fps=case["fps"], ctx=gpu_ctx)
    want_rates, want_ran = R.replay(losses, dict(R.DEFAULTS, lr_scheduler_patience=5, early_stopping_patience=20))
    print(f"{ran} epochs, learning rates {sorted(set(rates.tolist()), reverse=True)}, loss {losses[0]:.4g} -> {losses[-1]:.4g}")
    assert ran == want_ran == len(losses) < 2000
    assert rates.tolist() == want_rates.tolist()
    assert len(set(rates.tolist())) >= 3 and np.isfinite(losses).all()
    for check_every in (1, 1000):
        other = P.optimise_poses(fs, params, options, fps=case["fps"], check_every=check_every, ctx=gpu_ctx)
        assert _bits(other[0].poses()) == _bits(got.poses()) and _bits(other[1]) == _bits(losses) and _bits(other[2]) == _bits(rates) and other[3] == ran


# ------------------------------------------------------------------------------------------------ 6. it optimises
def test_it_optimises(gpu_ctx):
    """Default options on the constrained common case (pose_optimiser_restatement.constrained_case: every frame held by at least 63 correspondences, points
    close to the cameras; fps 30, clip at 1 / 30 m), start poses drifting 16.0 mm / 0.038 rad from the truth, WITHOUT the smoothing terms -- the fine-tune step,
    the last word of the default pipeline.  The float64 restatement improves both errors more than a hundredfold -- asserted as a condition; on the CPU it went
    16.0 mm -> 0.0024 mm and 0.038 rad -> 8.8e-6 rad in 315 epochs with three reductions of the learning rate, and between 2 000 and 100 000 times over three
    seeds and both dtypes -- and the kernel's final position RMSE and largest rotation error are within a factor of two of the restatement's.
    Not asserted WITH the smoothing terms: there the restatement itself does not optimise this case -- 1 - (r_a . r_b)^2 on the raw quaternions rewards a
    longer quaternion, Adam's sign-like steps follow that radial gradient wherever the correspondences pull weakly, and the float64 loop ends at 12.6 mm /
    0.82 rad after 100 epochs (loss 0.021 -> 0.031).  test_run_is_closer_to_float64_than_the_reference_arithmetic covers the smoothing terms over 50 epochs."""
    from hive_amd import pose_optimisation as P
    case = _case("constrained")
    before = R.pose_errors(case["start"].astype(np.float64), case["truth"])
    r64, _, _, restated_epochs = _restated(case, 4000, "float64", smooth=False)
    want = R.pose_errors(r64, case["truth"])
    got, losses, rates, ran = P.optimise_poses(_feature_set(case), _parameters(case), _options(), smooth_trajectory=False, fps=case["fps"], ctx=gpu_ctx)
    mine = R.pose_errors(got.poses(), case["truth"])
    print(f"before {before}, restatement {want} in {restated_epochs} epochs, kernel {mine} in {ran} epochs, learning rates {sorted(set(rates.tolist()))}")
    assert want[0] <= before[0] / 100 and want[1] <= before[1] / 100
    assert mine[0] <= 2 * want[0] and mine[1] <= 2 * want[1]
    assert ran < 4000 and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 7. the class
class _Dataset:
    """The part of a HiveDataset the optimiser reads, around a case."""

    def __init__(self, case, base_path):
        from hive_amd.geometric import Trajectory
        self.num_frames, self.fps, self.base_path = case["n"], case["fps"], str(base_path)
        self.camera_matrix = R.camera_matrix(case)
        self.camera_trajectory = Trajectory(case["start"].copy())


def _planted_optimiser(case, base_path, **kw):
    from hive_amd import pose_optimisation as P

    class Planted(P.PoseOptimiser):
        def _extract_feature_points(self, frame_pairs, feature_extraction_options=None):
            return _feature_set(case)

    return Planted(_Dataset(case, base_path), **kw)


def test_class_equals_its_pieces(gpu_ctx, tmp_path):
    """PoseOptimiser.run() with the default pipeline (PairWise3D, Global3D) plus fine-tune and a planted FeatureSet == the two pair-wise runs merged from the
    identity pose by subtract_pose / add_pose, the global loop, the fine-tune loop without the smoothing terms, the gap (frame 7, in no pair) filled by Slerp and
    linear interpolation; debug files written; the dataset's stored trajectory untouched."""
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp
    from hive_amd import pose_optimisation as P
    from hive_amd.geometric import add_pose, get_identity_pose, subtract_pose
    case = _case()
    options = _options(num_epochs=20)
    optimiser = _planted_optimiser(case, tmp_path, optimisation_options=options)
    stored = optimiser.dataset.camera_trajectory.values.copy()
    trajectory, scale, shift = optimiser.run()
    assert np.array_equal(optimiser.dataset.camera_trajectory.values, stored) and scale.size == 0 and shift.size == 0
    assert [h[0] for h in optimiser.history] == ["PairWise/ConsecutiveNoOverlap", "PairWise/ConsecutiveNoOverlapOffset", "Global3D", "FineTune"]

    fs, n = _feature_set(case), case["n"]
    start = P.OptimisationParameters(case["start"].astype(np.float64), P.AlignmentType.Rigid)
    pose_data = {}
    for mode in (P.FrameSamplingMode.ConsecutiveNoOverlap, P.FrameSamplingMode.ConsecutiveNoOverlapOffset):
        pairs = P.sample_frame_pairs(mode, n)
        out = P.optimise_poses(fs.subset_from(pairs), start, options, fps=case["fps"], ctx=gpu_ctx)[0].get_trajectory()
        pose_data.update({pair: out[list(pair)] for pair in pairs})
    merged = [get_identity_pose()]
    for pair in sorted(pose_data):
        merged.append(add_pose(merged[-1], subtract_pose(*pose_data[pair])))
    step = P.optimise_poses(fs, P.OptimisationParameters(np.asarray(merged), P.AlignmentType.Rigid), options, fps=case["fps"], ctx=gpu_ctx)[0]
    fine = P.optimise_poses(fs, step, options, smooth_trajectory=False, fps=case["fps"], ctx=gpu_ctx)[0].get_trajectory().values
    want = fine.copy()
    want[6:9, 4:] = interp1d([0, 1], [fine[6, 4:], fine[8, 4:]], axis=0)(np.linspace(0, 1, 3))
    want[6:9, :4] = Slerp([0, 1], Rotation.from_quat(fine[[6, 8], :4]))(np.linspace(0, 1, 3)).as_quat()
    assert _bits(trajectory.values) == _bits(want)
    assert not np.array_equal(want[7], fine[7]) and np.abs(np.linalg.norm(trajectory.values[:, :4], axis=1) - 1).max() <= 4 * R.U
    names = sorted(os.listdir(tmp_path / "pose_optim"))
    assert {"optimised_camera_trajectory.txt", "scale.txt", "shift.txt"} <= set(names)
    assert np.array_equal(np.loadtxt(tmp_path / "pose_optim" / "optimised_camera_trajectory.txt"), want)
    try:
        import matplotlib  # noqa: F401
        assert {"initial_trajectory.png", "0_PairWise3D.png", "1_Global3D.png", "3_FineTune.png"} <= set(names)
    except ImportError:
        pass


def test_class_with_fewer_frames_affine_and_smoothing(gpu_ctx, tmp_path):
    """run(num_frames = 6) on the 12-frame dataset: six poses, from the correspondences whose two frames are both below 6; Affine alignment returns a scale and a
    shift per frame; trajectory_smoothing is the reference's moving average of the positions; debug=False writes nothing."""
    from hive_amd import pose_optimisation as P
    case = _case()
    options = _options(num_epochs=10, alignment_type=P.AlignmentType.Affine, steps=(P.OptimisationStep.Global2D,), fine_tune=False, trajectory_smoothing=0.5)
    optimiser = _planted_optimiser(case, tmp_path, optimisation_options=options, debug=False)
    trajectory, scale, shift = optimiser.run(6)
    fs = _feature_set(case).sample_at(range(6))
    start = P.OptimisationParameters(case["start"].astype(np.float64)[:6], P.AlignmentType.Affine)
    out = P.optimise_poses(fs, start, options, P.ResidualType.Image2D, fps=case["fps"], ctx=gpu_ctx)[0]
    want = out.get_trajectory().values
    for i in range(1, 6):
        want[i, 4:] = 0.5 * out.translation_vectors[i] + 0.5 * want[i - 1, 4:]
    assert trajectory.values.shape == (6, 7) and _bits(trajectory.values) == _bits(want)
    assert _bits(scale) == _bits(out.scale) and _bits(shift) == _bits(out.shift) and scale.shape == (6,) and np.any(scale != 1.0)
    assert os.listdir(tmp_path) == []


def test_class_through_the_real_feature_extractor(gpu_ctx, tmp_path):
    """One run through the real FeatureExtractor on tests/feature_cases.Dataset with a trajectory and fps attached: N unit-quaternion poses come back."""
    import feature_cases as C
    from hive_amd import pose_optimisation as P
    from hive_amd.geometric import Trajectory
    data = C.Dataset()
    data.camera_trajectory = Trajectory(np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (data.num_frames, 1)))
    data.fps, data.base_path = 30.0, str(tmp_path)
    optimiser = P.PoseOptimiser(data, feature_extraction_options=P.FeatureExtractionOptions(min_features=C.MIN_FEATURES, max_features=2048),
                                optimisation_options=_options(num_epochs=5), debug=False)
    trajectory, scale, shift = optimiser.run()
    assert trajectory.values.shape == (data.num_frames, 7) and np.isfinite(trajectory.values).all()
    assert np.abs(np.linalg.norm(trajectory.values[:, :4], axis=1) - 1).max() <= 4 * R.U


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(gpu_ctx):
    """Bad arguments fail with a message: Deformable, frame indices outside [0, n), fewer than two frames, depths and focal lengths that are not positive, a feature
    set on the CPU or without a row, a clip distance without fps."""
    import ctypes
    from hive_amd import _lib, pose_optimisation as P
    case = _case()
    fs, params = _feature_set(case), _parameters(case)
    go = lambda f=fs, p=params, o=None, **kw: P.optimise_poses(f, p, o or _options(), fps=kw.pop("fps", 30.0), num_epochs=1, ctx=gpu_ctx, **kw)
    with pytest.raises(NotImplementedError, match="Deformable"):
        go(o=_options(alignment_type=P.AlignmentType.Deformable))
    with pytest.raises(NotImplementedError, match="Deformable"):
        P.OptimisationParameters(case["start"], P.AlignmentType.Deformable)
    o, p, ran = P._PoseOptions(num_epochs=1, alignment_type=2, learning_rate=1e-2), params.poses(), ctypes.c_int(0)  # the C entry itself
    arrays = [_lib.ptr(t) for side in (fs.frame_i, fs.frame_j) for t in (side.index, side.points, side.depth)]
    rc = gpu_ctx.lib.hive_pose_optimise(gpu_ctx.handle, _lib.ptr(p), None, None, 12, 500.0, 500.0, 320.0, 240.0, *arrays, len(fs), ctypes.addressof(o), -1.0, 1,
                                        _lib.ptr(np.zeros(1)), _lib.ptr(np.zeros(1)), ctypes.byref(ran), None, None)
    assert rc == _lib.ERR_INVALID and b"Deformable" in gpu_ctx.lib.hive_last_error(gpu_ctx.handle)
    with pytest.raises(_lib.HiveError, match="names frame 12"):
        go(f=_feature_set(dict(case, index_j=np.where(np.arange(len(case["index_j"])) == 5, 12, case["index_j"]))))
    with pytest.raises(_lib.HiveError, match="names frame -1"):
        go(f=_feature_set(dict(case, index_i=np.where(np.arange(len(case["index_i"])) == 9, -1, case["index_i"]))))
    with pytest.raises(_lib.HiveError, match="at least 2"):
        go(f=_feature_set(dict(case, index_i=np.zeros_like(case["index_i"]), index_j=np.zeros_like(case["index_j"]))), p=_parameters(case, poses=params.poses()[:1]))
    with pytest.raises(_lib.HiveError, match="depth must be positive"):
        go(f=_feature_set(dict(case, depth_j=np.where(np.arange(len(case["depth_j"])) == 700, 0.0, case["depth_j"]).astype(np.float32))))
    flat = _feature_set(case)
    flat.camera_matrix = flat.camera_matrix.clone()
    flat.camera_matrix[1, 1] = 0.0
    with pytest.raises(_lib.HiveError, match="focal lengths must be positive"):
        go(f=flat)
    with pytest.raises(ValueError, match="on the device"):
        go(f=fs.to("cpu"))
    with pytest.raises(ValueError, match="no correspondence"):
        go(f=fs.sample_at([]))
    with pytest.raises(ValueError, match="fps"):
        go(fps=None)
    with pytest.raises(_lib.HiveError, match="check_every"):
        go(check_every=0)
    # and the context still works
    assert go()[3] == 1
