"""Frame registration from 3-D feature matches: a first trajectory from the pictures and their depth maps alone.

The reference gets poses from COLMAP (``estimate_pose=True``) or, for ``MeshReconstructionMethod.BundleFusion``, from an external binary ("3D correspondence
guided frame registration"); both are absent.  Here every frame pair's matched SIFT keypoints, back-projected with their depth, go through a rigid (optionally
similarity) RANSAC on the device (``features.ransac_rigid``, csrc/register.hip) and the relative transforms are chained into a trajectory on the host
(``chain_pairs``).  The result is a start for ``PoseOptimiser`` and ``tsdf_fusion``; it is not pinned against COLMAP, BundleFusion, cv2's estimateAffine3D or
Open3D's correspondence RANSAC, none of which is available."""
import collections

import numpy as np

from hive_amd.pose_optimisation import FeatureExtractionOptions, FeatureExtractor, FrameSamplingMode, sample_frame_pairs

RegistrationResult = collections.namedtuple("RegistrationResult", "trajectory depth_scale lost pair_stats pair_transforms feature_set")
RegistrationResult.__doc__ = """``trajectory``: a ``Trajectory`` (world -> camera, one row a frame); ``depth_scale`` float64 (N,): what a frame's depth is multiplied by to
be in the root frame's unit (all 1 without ``with_scale``); ``lost``: the frames no chain of pairs reached (they copy a neighbour's pose); ``pair_stats`` and
``pair_transforms`` = (T, scale, rms, result): the extractor's host arrays per pair; ``feature_set``: the inlier correspondences, ready for ``PoseOptimiser``."""


def chain_pairs(num_frames, pairs, T, scale, result, min_inliers=20, root=0, first_pose=np.eye(4)):
    """Relative transforms -> ``(poses float64 (N, 4, 4) world -> camera, depth_scale float64 (N,), lost)``.  A host function in numpy float64 on one download of
    ``ransac_rigid``'s outputs: ``T`` (P, 4, 4) maps camera-i points onto camera-j points of pair (i, j) and holds s R and t, ``scale`` (P,) is s, ``result``
    (P, 3) the winning trial, the winner's count and the final count.

    A pair is an edge when it has a model (winning trial >= 0) and its final count is at least ``min_inliers``; an edge can be walked both ways.  The search is
    breadth-first from ``root`` (pose ``first_pose``, depth scale 1): the frontier in ascending frame index, a frame's edges in pair-list order, the first arrival
    wins.  With lambda the depth scale, a forward edge i -> j gives lambda_j = lambda_i / s and G_j = [R | lambda_j t] G_i; a backward edge gives lambda_i =
    lambda_j s and G_i = [R^T | -lambda_j R^T t] G_j; R = T[:3, :3] / s.  A frame that is not reached copies the pose and lambda of the nearest reached frame
    with a lower index (a higher one if none is lower) and is listed in ``lost``."""
    n = int(num_frames)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    T, scale, result = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4), np.asarray(scale, dtype=np.float64).reshape(-1), np.asarray(result).reshape(-1, 3)
    if not len(pairs) == len(T) == len(scale) == len(result):
        raise ValueError(f"{len(pairs)} pairs, {len(T)} transforms, {len(scale)} scales and {len(result)} results")
    if not 0 <= int(root) < n:
        raise ValueError(f"root = {root}; there are {n} frames")
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= n):
        raise ValueError(f"pairs name frames {int(pairs.min())} .. {int(pairs.max())}; there are {n}")
    edge = (result[:, 0] >= 0) & (result[:, 2] >= int(min_inliers))
    poses, lam = np.tile(np.eye(4), (n, 1, 1)), np.ones(n)
    reached = np.zeros(n, dtype=bool)
    poses[root], reached[root] = np.asarray(first_pose, dtype=np.float64), True
    frontier = [int(root)]
    while frontier:
        arrived = []
        for f in sorted(frontier):
            for p in np.nonzero(edge & ((pairs[:, 0] == f) | (pairs[:, 1] == f)))[0]:
                i, j = int(pairs[p, 0]), int(pairs[p, 1])
                if i == j:
                    continue
                s = scale[p]
                R, t = T[p, :3, :3] / s, T[p, :3, 3]
                step = np.eye(4)
                if i == f and not reached[j]:
                    lam[j] = lam[i] / s
                    step[:3, :3], step[:3, 3] = R, lam[j] * t
                    poses[j], reached[j] = step @ poses[i], True
                    arrived.append(j)
                elif j == f and not reached[i]:
                    lam[i] = lam[j] * s
                    step[:3, :3], step[:3, 3] = R.T, -lam[j] * (R.T @ t)
                    poses[i], reached[i] = step @ poses[j], True
                    arrived.append(i)
        frontier = arrived
    lost = [int(f) for f in np.nonzero(~reached)[0]]
    found = np.nonzero(reached)[0]
    for f in lost:
        lower = found[found < f]
        source = int(lower[-1]) if len(lower) else int(found[found > f][0])
        poses[f], lam[f] = poses[source], lam[source]
    return poses, lam, lost


def estimate_trajectory(dataset, frame_sampling=FrameSamplingMode.Hierarchical, num_frames=-1, feature_extraction_options=None, threshold=0.05, trials=2000, seed=0,
                        with_scale=False, sift=None) -> RegistrationResult:
    """A trajectory for a ``HiveDataset`` with depth maps, from its pictures alone -> ``RegistrationResult``.  Frame pairs by ``frame_sampling`` over the first
    ``num_frames`` frames (-1: all); one ``FeatureExtractor`` run with ``model="rigid"`` (SIFT once a frame, the pair matcher, the rigid RANSAC, the
    compaction; one synchronisation); then ``chain_pairs`` with ``min_inliers`` = the options' ``min_features``.  The
    trajectory is in HIVE's convention (world -> camera) and anchored at the dataset's stored first pose, as ``tracking.estimate_trajectory`` anchors its result.
    ``threshold`` is in the depth's unit: 0.05 is a parameter default (5 cm for metres), not a measured quantity.  With ``with_scale`` (depth maps known up to a
    scale per frame, such as estimated depth) ``depth_scale`` holds the factors; ``1 / depth_scale`` is the start for the Affine alignment's scale parameters."""
    from hive_amd.geometric import Trajectory
    n = dataset.num_frames if num_frames is None or int(num_frames) < 0 else min(int(num_frames), dataset.num_frames)
    if n < 1:
        raise ValueError("no frames")
    options = feature_extraction_options or FeatureExtractionOptions()
    pairs = sample_frame_pairs(frame_sampling, n)
    extractor = FeatureExtractor(dataset, pairs, options, sift=sift, seed=seed, model="rigid", rigid_threshold=threshold, ransac_trials=trials, with_scale=with_scale)
    feature_set = extractor.extract_feature_points()
    T, scale, rms, result = extractor.pair_transforms
    first_pose = np.asarray(dataset.camera_trajectory.to_homogenous_transforms()[0], dtype=np.float64)
    poses, depth_scale, lost = chain_pairs(n, pairs, T, scale, result, min_inliers=options.min_features, root=0, first_pose=first_pose)
    return RegistrationResult(Trajectory.from_homogenous_transforms(poses), depth_scale, lost, extractor.pair_stats, extractor.pair_transforms, feature_set)
