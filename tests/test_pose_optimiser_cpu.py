"""Host side of the pose optimiser (hive_amd/pose_optimisation.py: options, EarlyStopping, OptimisationParameters, HiveDataset.fps, the C declarations) and the
conditions on the cases and restatements (tests/pose_optimiser_restatement.py) that tests/test_pose_optimiser_gpu.py leans on."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_optimiser_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_validate_and_copy():
    from hive_amd.pose_optimisation import AlignmentType, OptimisationOptions as O, OptimisationStep as S
    o = O()
    assert (o.num_epochs, o.learning_rate, o.l2_regularisation, o.min_loss_delta, o.lr_scheduler_patience, o.early_stopping_patience) == (4000, 1e-2, 0.5, 1e-4, 50, 75)
    assert (o.alignment_type, o.steps, o.position_only, o.fine_tune, o.pose_t_reg, o.pose_r_reg, o.trajectory_smoothing, o.clip_distance) == \
        (AlignmentType.Rigid, (S.PairWise3D, S.Global3D), False, True, 0.5, 1.0, None, 1.0)
    changed = O(num_epochs=7, alignment_type=AlignmentType.Affine, steps=[S.Global2D], clip_distance=0.25, trajectory_smoothing=0.9, position_only=True, fine_tune=False)
    copy = changed.copy()
    assert copy is not changed and repr(copy) == repr(changed) and copy.clip_distance == 0.25  # the reference's copy() drops clip_distance
    assert "clip_distance=0.25" in repr(copy) and repr(copy).startswith("OptimisationOptions(num_epochs=7, learning_rate=0.01, ")
    assert O(clip_distance=None).copy().clip_distance is None
    for bad in (dict(num_epochs=0), dict(num_epochs=1.5), dict(learning_rate=0.0), dict(l2_regularisation=-1.0), dict(min_loss_delta=0.0), dict(lr_scheduler_patience=0),
                dict(early_stopping_patience=-3), dict(pose_t_reg=-0.1), dict(pose_r_reg=float("nan")), dict(trajectory_smoothing=-1.0), dict(clip_distance=-1.0),
                dict(steps=()), dict(steps="Global3D"), dict(steps=(S.Global3D, "Global3D")), dict(steps=[1]), dict(alignment_type="Rigid")):
        with pytest.raises(ValueError):
            O(**bad)


def test_early_stopping_rule():
    from hive_amd.pose_optimisation import EarlyStopping
    for cls in (EarlyStopping, lambda patience, min_difference: R.EarlyStopping(patience, min_difference)):
        stop = cls(patience=2, min_difference=0.1)
        # an improvement of exactly min_difference does not count; 1.0 -> 0.85 does
        assert [stop.step(v) for v in (1.0, 0.9, 0.95, 0.85, 0.85, 0.8, 0.76)] == [False, False, False, False, False, False, True]
        assert stop.should_stop


def test_optimisation_parameters_holder():
    from hive_amd.geometric import Trajectory
    from hive_amd.pose_optimisation import AlignmentType, OptimisationParameters as P
    poses = np.arange(28, dtype=np.float32).reshape(4, 7) + 1
    rigid = P(poses, AlignmentType.Rigid)
    assert rigid.dtype == np.float64 and len(rigid) == 28 and rigid.scale.size == 0 and rigid.shift.size == 0 and rigid.num_frames == 4
    affine = P(Trajectory(poses), AlignmentType.Affine)
    assert len(affine) == 36 and np.array_equal(affine.scale, np.ones(4)) and np.array_equal(affine.shift, np.zeros(4))
    trajectory = affine.get_trajectory()
    assert isinstance(trajectory, Trajectory) and np.abs(np.linalg.norm(trajectory.values[:, :4], axis=1) - 1).max() <= 2 * R.U
    assert np.array_equal(trajectory.values[:, 4:], poses[:, 4:]) and np.array_equal(affine.rotation_quaternions, poses[:, :4])  # the holder keeps the raw ones
    affine.scale[:] = [1, 2, 3, 4]
    part = affine.sample_at([3, 1])
    assert np.array_equal(part.scale, [4, 2]) and np.array_equal(part.poses(), poses[[3, 1]]) and part.alignment_type is AlignmentType.Affine
    clone = affine.clone()
    clone.translation_vectors[:] = 0
    clone.scale[:] = 0
    assert affine.translation_vectors.any() and affine.scale.all()
    clone.normalise_rotations()
    assert np.abs(np.linalg.norm(clone.rotation_quaternions, axis=1) - 1).max() <= 2 * R.U
    with pytest.raises(NotImplementedError, match="Deformable"):
        P(poses, AlignmentType.Deformable)
    with pytest.raises(ValueError):
        P(poses[:, :6], AlignmentType.Rigid)


def test_dataset_fps(tmp_path):
    from hive_amd.io import HiveDataset
    assert isinstance(HiveDataset.fps, property)

    class Meta:
        fps = 29.97

    data = HiveDataset.__new__(HiveDataset)
    data.metadata = Meta()
    assert data.fps == 29.97


def test_new_symbols_are_declared_and_exported():
    from hive_amd import _lib, pose_optimisation as P
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    assert re.search(r"^int hive_pose_optimise\(", header, flags=re.M) and re.search(r"^int hive_pose_project\(", header, flags=re.M)
    assert "projected Adam" in header and "DELIBERATE DEVIATION" in header
    assert len(_lib.SIGNATURES["hive_pose_optimise"][1]) == 24 and len(_lib.SIGNATURES["hive_pose_project"][1]) == 4
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "hive_pose_optimise") and hasattr(lib, "hive_pose_project")
    fields = re.search(r"typedef struct hive_pose_options \{(.*?)\} hive_pose_options;", header, flags=re.S).group(1)
    declared = [name for line in re.sub(r"/\*.*?\*/", "", fields).split(";") for name in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert declared == [name for name, _ in P._PoseOptions._fields_] and ctypes.sizeof(P._PoseOptions) == 72
    for name in ("AlignmentType", "ResidualType", "OptimisationStep", "EarlyStopping", "OptimisationOptions", "OptimisationParameters", "PoseOptimiser", "optimise_poses",
                 "project_poses", "main"):
        assert hasattr(P, name)
    assert "PROJECTED ADAM" in P.__doc__ and "Deformable" in P.__doc__


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("residual", ["World3D", "Image2D"])
def test_two_float64_formulations_agree(residual, affine, smooth):
    """Quaternion products against rotation matrices, both float64, held to the bound of tests/test_pose_optimiser_gpu.py::test_loss_and_gradient_against_autograd."""
    case, n = R.make_case(), 12
    rng = np.random.default_rng(3)
    scale, shift = (1.0 + 0.05 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)) if affine else (np.ones(n), np.zeros(n))
    start = case["start"].astype(np.float64)
    a_loss, a_grad = R.loss_and_gradient(start, scale, shift, case, residual, affine, smooth)
    b_loss, b_grad = R.loss_and_gradient(start, scale, shift, case, residual, affine, smooth, apply=R._apply_matrix)
    kappa = R.conditioning(start, scale, shift, case, residual, affine)
    longest = int(np.bincount(np.concatenate([case["index_i"], case["index_j"]])).max()) + 16
    magnitude = R.gradient_term_magnitudes(start, scale, shift, case, residual, affine, smooth)
    assert abs(a_loss - b_loss) / a_loss <= 2 * (16 * kappa + len(case["index_i"])) * R.U
    assert np.all(np.abs(a_grad - b_grad) <= 2 * (16 * kappa + longest) * R.U * magnitude)
    assert np.all(np.abs(a_grad) <= magnitude * (1 + 1e-9))  # the magnitudes bound the gradient they are made for
    assert not a_grad[0, :7].any() and (affine or not a_grad[:, 7:].any())


def test_the_common_case_is_what_the_tests_need():
    """12 frames, hierarchical pairs, frame 0 in four pairs, frame 7 in none, per-pair counts 1, 63, 64, 65 and 257 (so incidence lists cross the lane and the
    workgroup strides), shuffled rows, a start trajectory inside the clip distance, and no unpinned gradient component below 1e-6 of the largest."""
    case = R.make_case()
    pairs = list(zip(case["index_i"].tolist(), case["index_j"].tolist()))
    assert case["n"] == 12 and sum(0 in p for p in case["pairs"]) == 4 and not any(7 in p for p in case["pairs"])
    assert sorted(set(pairs.count(p) for p in case["pairs"])) == [1, 63, 64, 65, 257]
    assert pairs != sorted(pairs) and np.all(case["depth_i"] > 0) and np.all(case["depth_j"] > 0)
    lists = np.bincount(np.concatenate([case["index_i"], case["index_j"]]), minlength=12)
    assert lists[7] == 0 and lists.max() > 256 and any(64 < v <= 256 for v in lists) and any(0 < v <= 64 for v in lists)
    steps = np.linalg.norm(np.diff(case["start"][:, 4:].astype(np.float64), axis=0), axis=1)
    assert steps.max() < 1.0 / case["fps"]
    assert np.array_equal(R.clip_stated(case["start"][:, 4:].astype(np.float64), 1.0 / case["fps"]), case["start"][:, 4:].astype(np.float64))
    for residual in ("World3D", "Image2D"):
        _, grad = R.loss_and_gradient(case["start"], np.ones(12), np.zeros(12), case, residual)
        free = np.abs(grad[1:, :7])
        assert free.min() >= 1e-6 * free.max(), (residual, free.min() / free.max())
    # at the truth the correspondences are exact up to their float32 rounding
    at_truth, _ = R.loss_and_gradient(case["truth"], np.ones(12), np.zeros(12), case, smooth=False)
    assert at_truth < 1e-5 < 1e-3 < R.loss_and_gradient(case["start"], np.ones(12), np.zeros(12), case, smooth=False)[0]


@pytest.mark.parametrize("n", [2, 3, 70, 1100])
def test_stated_clip_against_the_literal_loop(n):
    """The stated order against the reference's sequential loop in numpy, within the bound test_pose_optimiser_gpu.py derives; steps at the limit are kept, steps
    above it end up at it, the untouched head is bit-identical."""
    limit = 0.25
    poses, kinds = R.clip_trajectory(n, limit)
    t = poses[:, 4:]
    stated, literal = R.clip_stated(t, limit), R.clip_literal(t, limit)
    assert np.abs(stated - literal).max() <= 8 * n * R.U * max(np.abs(t).max(), np.abs(literal).max())
    before = np.linalg.norm(np.diff(t, axis=0), axis=1)
    after = np.linalg.norm(np.diff(stated, axis=0), axis=1)
    assert "above" in kinds and (n < 3 or "at" in kinds) and (n < 70 or "below" in kinds)
    assert np.all(np.abs(after[before > limit] - limit) <= 8 * n * R.U) and np.allclose(after[before <= limit], before[before <= limit], rtol=0, atol=8 * n * R.U)
    first = int(np.argmax(before > limit)) + 1
    assert np.array_equal(stated[:first], t[:first])
    if n >= 70:
        over = before > limit
        assert max(len(run) for run in "".join("x" if v else " " for v in over).split()) >= 5 and (before == limit).sum() >= 5
    q = R.normalise_rows(poses[:, :4])
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 2 * R.U


def test_the_restatement_optimises_the_constrained_case():
    """The condition of test_it_optimises: without the smoothing terms the float64 loop, default options, improves both errors more than a hundredfold, stops
    early and lowers the learning rate on the way; replaying its losses gives its learning rates back."""
    case = R.constrained_case()
    assert min(np.bincount(np.concatenate([case["index_i"], case["index_j"]]), minlength=12)) >= 63
    before = R.pose_errors(case["start"].astype(np.float64), case["truth"])
    out, losses, rates, ran = R.run(case, 4000, smooth=False, max_frame_distance=1.0 / case["fps"])
    after = R.pose_errors(out, case["truth"])
    assert after[0] <= before[0] / 100 and after[1] <= before[1] / 100 and ran < 4000 and len(set(rates.tolist())) >= 3
    replayed, epochs = R.replay(losses)
    assert epochs == ran and replayed.tolist() == rates.tolist()
