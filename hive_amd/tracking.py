"""Camera tracking against the TSDF volume on the MI355X: poses for a capture that has sensor depth and no trajectory (Kinect, TUM, StrayScanner).

The reference takes its poses from COLMAP, or from BundleFusion for the alternative background method -- external binaries, absent here
(``TUMAdaptor.convert(estimate_pose=True)`` keeps raising).  This module is the RGB-D alternative, KinectFusion-style: the volume is ray cast from the last
good pose (csrc/raycast.hip), the live depth frame is aligned to those model maps by point-to-plane ICP with projective association (csrc/track.hip: one
launch and one copy of 29 numbers per iteration, the 6 x 6 solve on the host in float64), and the frame is integrated at the pose found.  With
``photometric_weight`` > 0 the frame's colour is aligned to the model's ray-cast colour in the same launch (the photometric term of RGB-D odometry, 58 numbers
per iteration), which keeps a view of one or two planes with texture on them tracked; the rules are restated in tests/photometric_restatement.py.

The rules of the kernels are stated in include/hive_mi355x.h above ``hive_tsdf_raycast`` and restated in numpy in tests/raycast_restatement.py and
tests/tracking_restatement.py.  Poses are camera-to-world 4 x 4 float64, as ``TSDFVolume.integrate`` takes them; the trajectories returned are in HIVE's
convention (world-to-camera rows)."""
import ctypes
from typing import NamedTuple

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr

# cond(A) of the 6 x 6 normal equations above which a step counts as degenerate.  Measured with the numpy restatement (tests/test_tracking_cpu.py, DESIGN.md
# section 5): views of a room corner (two walls and the floor) gave 6.6e2 .. 1.9e3 over every level and iteration; the two-wall view, where the camera can
# slide along the edge, is exactly singular on clean depth (cond = inf) and gave 1.45e4 or more with 1 mm of depth noise.  The default is the geometric mean
# of 1.9e3 and 1.45e4, rounded.  Depth noise LOWERS the two-wall figure (3 mm: 2.3e3), so on a noisy sensor this gate alone does not tell the scenes apart.
DEFAULT_MAX_COND = 5.0e3
BOUNDS_MARGIN = 0.5  # metres added on every side of the first chunk's view frusta by estimate_trajectory


class TrackResult(NamedTuple):
    pose: np.ndarray      # camera-to-world 4 x 4 float64; the initial pose when tracking was lost
    ok: bool
    pairs: int            # pairs of the last step that ran
    rmse: float           # sqrt(sum r^2 / pairs) of that step, metres (before its update)
    cond: float           # cond(A) of that step
    iterations_run: int


class FrameMaps:
    """The pyramid of one depth frame on the device: per level ``depth`` (H_l, W_l), ``vertex`` and ``normal`` (H_l, W_l, 3) float32 views of three packed
    buffers, ``K`` float32 (levels, 3, 3) and ``sizes`` [(H_l, W_l)]."""

    def __init__(self, depth, vertex, normal, K, sizes):
        self.K, self.sizes = K, sizes
        self.depth, self.vertex, self.normal = [], [], []
        at = 0
        for h, w in sizes:
            self.depth.append(depth[at:at + h * w].view(h, w))
            self.vertex.append(vertex[at:at + h * w].view(h, w, 3))
            self.normal.append(normal[at:at + h * w].view(h, w, 3))
            at += h * w


def _device_depth(depth, device):
    import torch
    if not hasattr(depth, "data_ptr"):
        depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
    if depth.dtype != torch.float32 or depth.dim() != 2:
        raise ValueError(f"depth: a float32 (H, W) map in metres, got {tuple(depth.shape)} {depth.dtype}")
    return depth.to(device).contiguous()


def frame_maps(depth, cam_intr, levels=3, pyr_delta=0.05, ctx=None) -> FrameMaps:
    """Depth pyramid, vertex and normal maps of a live frame (``hive_frame_maps``): level l + 1 halves level l (2 x 2 blocks, averaging the samples within
    ``pyr_delta`` metres of the block's nearest one, so that a depth edge is not smeared), with intrinsics fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2."""
    import torch
    ctx = (ctx or _lib.default_context()).follow_torch_stream()
    depth = _device_depth(depth, f"cuda:{ctx.device}")
    h, w = (int(v) for v in depth.shape)
    levels = int(levels)
    if levels < 1 or (h >> (levels - 1)) == 0 or (w >> (levels - 1)) == 0:
        raise ValueError(f"{h} x {w} has no {levels} pyramid levels")
    sizes = [(h >> l, w >> l) for l in range(levels)]
    total = sum(a * b for a, b in sizes)
    d = torch.empty(total, dtype=torch.float32, device=depth.device)
    v = torch.empty((total, 3), dtype=torch.float32, device=depth.device)
    n = torch.empty((total, 3), dtype=torch.float32, device=depth.device)
    K = np.ascontiguousarray(cam_intr, dtype=np.float32).reshape(3, 3)
    K_levels = np.zeros((levels, 3, 3), np.float32)
    ctx.check(ctx.lib.hive_frame_maps(ctx.handle, ptr(depth), h, w, ptr(K), levels, float(pyr_delta), ptr(d), ptr(v), ptr(n), ptr(K_levels)))
    return FrameMaps(d, v, n, K_levels, sizes)


def icp_step(ctx, K, live_vertex, live_normal, model_vertex, model_normal, model_pose, est_pose, dist_thresh, cos_thresh, pair_mask=None):
    """``hive_icp_step``: (sums float64 [28], pairs) of one Gauss-Newton step at one level; synchronises (one copy of 29 numbers)."""
    h, w = (int(v) for v in live_vertex.shape[:2])
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)
    model_pose = np.ascontiguousarray(model_pose, dtype=np.float64).reshape(4, 4)
    est_pose = np.ascontiguousarray(est_pose, dtype=np.float64).reshape(4, 4)
    sums = np.zeros(28, np.float64)
    pairs = ctypes.c_int64(0)
    ctx.check(ctx.lib.hive_icp_step(ctx.handle, h, w, ptr(K), ptr(live_vertex), ptr(live_normal), ptr(model_vertex), ptr(model_normal), ptr(model_pose),
                                    ptr(est_pose), float(dist_thresh), float(cos_thresh), ptr(sums), ctypes.byref(pairs), ptr(pair_mask)))
    return sums, int(pairs.value)


def _device_color(color, device):
    import torch
    if not hasattr(color, "data_ptr"):
        color = torch.from_numpy(np.ascontiguousarray(color))
    if color.dtype != torch.uint8 or color.dim() != 3 or color.shape[2] != 3:
        raise ValueError(f"color: a uint8 (H, W, 3) picture, got {tuple(color.shape)} {color.dtype}")
    return color.to(device).contiguous()


def intensity_pyramid(color, levels=3, ctx=None):
    """The intensity pyramid of a colour frame (``hive_gray_pyramid``) -> per level a float32 (H_l, W_l) device view of one packed buffer: level 0 is the
    integer luma / 255, level l + 1 the plain 2 x 2 means of level l, with the sizes of ``frame_maps``."""
    import torch
    ctx = (ctx or _lib.default_context()).follow_torch_stream()
    color = _device_color(color, f"cuda:{ctx.device}")
    h, w = (int(v) for v in color.shape[:2])
    levels = int(levels)
    if levels < 1 or (h >> (levels - 1)) == 0 or (w >> (levels - 1)) == 0:
        raise ValueError(f"{h} x {w} has no {levels} pyramid levels")
    sizes = [(h >> l, w >> l) for l in range(levels)]
    gray = torch.empty(sum(a * b for a, b in sizes), dtype=torch.float32, device=color.device)
    ctx.check(ctx.lib.hive_gray_pyramid(ctx.handle, ptr(color), h, w, levels, ptr(gray)))
    out, at = [], 0
    for a, b in sizes:
        out.append(gray[at:at + a * b].view(a, b))
        at += a * b
    return out


def rgbd_icp_step(ctx, K, live_vertex, live_normal, live_gray, model_vertex, model_normal, model_depth, model_color, model_pose, est_pose, dist_thresh,
                  cos_thresh, pair_mask=None, photo_mask=None):
    """``hive_rgbd_icp_step``: (sums float64 [56], (geometric pairs, photometric pairs)) of one Gauss-Newton step at one level -- ``icp_step``'s 28 sums, then
    the photometric term's 28; synchronises (one copy of 58 numbers)."""
    h, w = (int(v) for v in live_vertex.shape[:2])
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)
    model_pose = np.ascontiguousarray(model_pose, dtype=np.float64).reshape(4, 4)
    est_pose = np.ascontiguousarray(est_pose, dtype=np.float64).reshape(4, 4)
    sums = np.zeros(56, np.float64)
    pairs = np.zeros(2, np.int64)
    ctx.check(ctx.lib.hive_rgbd_icp_step(ctx.handle, h, w, ptr(K), ptr(live_vertex), ptr(live_normal), ptr(live_gray), ptr(model_vertex), ptr(model_normal),
                                         ptr(model_depth), ptr(model_color), ptr(model_pose), ptr(est_pose), float(dist_thresh), float(cos_thresh), ptr(sums),
                                         ptr(pairs), ptr(pair_mask), ptr(photo_mask)))
    return sums, (int(pairs[0]), int(pairs[1]))


def combined_sums(sums, photometric_weight):
    """The 28 sums of A = A_geo + w^2 A_photo and b = b_geo + w^2 b_photo from the 56 of ``hive_rgbd_icp_step``; sum r^2 stays the geometric one."""
    out = np.array(sums[:28], np.float64)
    out[:27] = out[:27] + (float(photometric_weight) * float(photometric_weight)) * np.asarray(sums[28:55], np.float64)
    return out


def normal_equations(sums):
    """(A 6 x 6 symmetric, b 6, sum r^2) from the 28 sums of ``hive_icp_step``."""
    A = np.zeros((6, 6), np.float64)
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    return A, np.array(sums[21:27], np.float64), float(sums[27])


def se3_exp(xi):
    """[exp(omega) | v] as 4 x 4 float64 for xi = (omega, v): Rodrigues' formula; the translation is taken as it stands."""
    omega, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    theta = float(np.sqrt(omega @ omega))
    Wx = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if theta < 1e-12:
        R = np.eye(3) + Wx
    else:
        R = np.eye(3) + (np.sin(theta) / theta) * Wx + ((1.0 - np.cos(theta)) / (theta * theta)) * (Wx @ Wx)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, v
    return T


def solve_step(sums):
    """(xi or None, cond(A)): A xi = b by Cholesky in float64; None when A is not positive definite."""
    A, b, _ = normal_equations(sums)
    if not np.all(np.isfinite(A)) or not np.any(A):
        return None, float("inf")
    cond = float(np.linalg.cond(A))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, cond
    return np.linalg.solve(L.T, np.linalg.solve(L, b)), cond


def level_iterations(iterations, levels):
    """``iterations`` lists the coarsest level first; with fewer levels than entries the LAST ``levels`` entries are used (the finest levels keep theirs),
    with more levels than entries the coarser levels repeat the first entry.  Returns the counts indexed by level (0 = finest)."""
    its = [int(v) for v in iterations]
    its = its[-levels:] if len(its) >= levels else [its[0]] * (levels - len(its)) + its
    return its[::-1]


def icp_align(volume, depth, cam_intr, model_pose, init_pose=None, levels=3, iterations=(10, 5, 4), dist_thresh=None, angle_deg=20.0, min_pair_share=0.1,
              max_cond=DEFAULT_MAX_COND, pyr_delta=0.05, ctx=None, color=None, photometric_weight=0.0) -> TrackResult:
    """Align a depth frame to the volume: frame-to-model point-to-plane ICP, coarse to fine.

    The volume is ray cast once per level at ``model_pose`` (the last good pose) with that level's size and intrinsics; the estimate starts at ``init_pose``
    (default: ``model_pose``).  Per iteration one ``hive_icp_step`` and one 6 x 6 Cholesky solve on the host; the estimate moves by T <- [exp(omega) | v] T.
    ``dist_thresh`` (metres, default twice the truncation distance) and ``angle_deg`` gate the pairs.  Tracking is lost -- ``ok=False``, the pose returned is
    the initial one, nothing raises -- when a step has fewer pairs than ``min_pair_share`` of its level's pixels or cond(A) above ``max_cond`` (a scene that
    does not constrain all six degrees of freedom: one or two planes).

    With the frame's ``color`` (uint8 (H, W, 3)) and a ``photometric_weight`` w > 0 the photometric term of RGB-D odometry is added: each level's ray cast
    returns the model's colour too, each iteration is one ``hive_rgbd_icp_step``, and the step solves A = A_geo + w^2 A_photo, b = b_geo + w^2 b_photo.  w is
    in metres per unit of intensity (intensity in [0, 1]): texture then fixes the directions that one or two planes leave free.  The pair-share gate stays on
    the geometric pairs, ``max_cond`` applies to the combined A, ``rmse`` stays the geometric one.  Off by default: the model's colour is the nearest voxel's,
    and where geometry already fixes the pose a heavy colour term costs accuracy.  Without a colour or with a weight of 0 the launches
    and the result are those of the geometric alignment."""
    ctx = ctx or volume._ctx
    weight = float(photometric_weight)
    if not np.isfinite(weight) or weight < 0:
        raise ValueError(f"photometric_weight: a finite number >= 0, got {photometric_weight}")
    model_pose = np.ascontiguousarray(model_pose, dtype=np.float64).reshape(4, 4)
    init = model_pose.copy() if init_pose is None else np.array(init_pose, dtype=np.float64).reshape(4, 4)
    levels = int(levels)
    if color is not None and tuple(color.shape[:2]) != tuple(depth.shape[:2]):
        raise ValueError(f"color is {tuple(color.shape[:2])}, depth is {tuple(depth.shape[:2])}")
    maps = frame_maps(depth, cam_intr, levels, pyr_delta, ctx)
    gray = intensity_pyramid(color, levels, ctx) if color is not None and weight > 0 else None
    dist = float(2.0 * volume._trunc_margin if dist_thresh is None else dist_thresh)
    cos_min = float(np.cos(np.deg2rad(angle_deg)))
    counts = level_iterations(iterations, levels)
    est, pairs, rmse, cond, done = init.copy(), 0, 0.0, float("inf"), 0
    for l in range(levels - 1, -1, -1):
        h, w = maps.sizes[l]
        model_d, model_v, model_n, *model_c = volume.raycast(maps.K[l], model_pose, (h, w), return_vertex=True, return_normal=True, return_color=gray is not None)
        for _ in range(counts[l]):
            if gray is None:
                sums, pairs = icp_step(ctx, maps.K[l], maps.vertex[l], maps.normal[l], model_v, model_n, model_pose, est, dist, cos_min)
            else:
                both, (pairs, _) = rgbd_icp_step(ctx, maps.K[l], maps.vertex[l], maps.normal[l], gray[l], model_v, model_n, model_d, model_c[0], model_pose, est,
                                                 dist, cos_min)
                sums = combined_sums(both, weight)
            done += 1
            rmse = float(np.sqrt(sums[27] / pairs)) if pairs else 0.0
            xi, cond = (None, float("inf")) if pairs < min_pair_share * h * w else solve_step(sums)
            if xi is None or not cond <= max_cond:
                return TrackResult(init, False, pairs, rmse, cond, done)
            est = se3_exp(xi) @ est
    return TrackResult(est, True, pairs, rmse, cond, done)


class Tracker:
    """Tracks a camera through a depth sequence and fuses what it sees: the first frame is integrated at ``first_pose``; every later frame is aligned against
    the volume from the last good pose (``icp_align``) and integrated with ``TSDFVolume.integrate`` only when the alignment held.  ``icp_options`` go to
    ``icp_align``; with a ``photometric_weight`` > 0 among them every frame's colour goes there too."""

    def __init__(self, volume, cam_intr, first_pose=np.eye(4), **icp_options):
        self.volume = volume
        self.cam_intr = np.ascontiguousarray(cam_intr, dtype=np.float32).reshape(3, 3)
        self.pose = np.array(first_pose, dtype=np.float64).reshape(4, 4)
        self.icp_options = icp_options
        self.frames = 0

    def step(self, color, depth) -> TrackResult:
        """One frame: colour uint8 (H, W, 3) and depth float32 (H, W) metres, both numpy or both device tensors."""
        if self.frames == 0:
            result = TrackResult(self.pose.copy(), True, 0, 0.0, 0.0, 0)
        else:
            with_color = float(self.icp_options.get("photometric_weight", 0.0)) > 0  # (a negative weight goes on to icp_align, which raises)
            result = icp_align(self.volume, depth, self.cam_intr, self.pose, **self.icp_options, color=color if with_color else None)
        self.frames += 1
        if result.ok:
            self.volume.integrate(color, depth, self.cam_intr, result.pose)
            self.pose = result.pose.copy()
        return result


def _trajectory(poses_c2w):
    from hive_amd.geometric import Trajectory
    return Trajectory.from_homogenous_transforms(np.linalg.inv(np.stack(poses_c2w)))


def track_and_fuse(color_frames, depth_frames, cam_intr, vol_bnds, voxel_size, first_pose=np.eye(4), **icp_options):
    """A trajectory and a fused volume from depth frames alone -> ``(TSDFVolume, Trajectory, [TrackResult])``.  The trajectory has one world-to-camera row
    per frame (HIVE's convention: ``gt.calculate_ate(pred)`` and ``calculate_rpe`` apply directly); a lost frame repeats the previous pose."""
    from hive_amd.fusion import TSDFVolume
    volume = TSDFVolume(vol_bnds, voxel_size)
    tracker = Tracker(volume, cam_intr, first_pose, **icp_options)
    results, poses = [], []
    for color, depth in zip(color_frames, depth_frames):
        results.append(tracker.step(color, depth))
        poses.append(tracker.pose.copy())
    if not poses:
        raise ValueError("no frames")
    return volume, _trajectory(poses), results


def estimate_trajectory(dataset, options=None, num_frames=-1, chunk_frames=None, bounds_margin=BOUNDS_MARGIN, **icp_options):
    """Poses for a ``HiveDataset`` with sensor depth -> ``(TSDFVolume, Trajectory, [TrackResult])``: the RGB-D alternative to ``estimate_pose=True`` (COLMAP).

    Depth and colour are read through ``fusion.frame_chunks``; of the dataset's trajectory only the FIRST pose is used (it fixes the world frame).  The volume's
    bounds are ``fusion.scene_bounds`` of the first chunk's depth maps, all placed at the first pose, grown by ``bounds_margin`` metres on every side (the
    camera is expected to stay near what it saw first); the voxel size follows ``options`` (``BackgroundMeshOptions``) as in ``tsdf_fusion``.  Dynamic-object
    masks are not applied."""
    from hive_amd import fusion
    from hive_amd.options import BackgroundMeshOptions
    options = options or BackgroundMeshOptions()
    frame_set = fusion._resolve_frames(dataset, num_frames, None)
    chunk_frames = int(chunk_frames or fusion.CHUNK_FRAMES)
    first_pose = np.linalg.inv(dataset.camera_trajectory.to_homogenous_transforms()[frame_set[0]])
    tracker, results, poses = None, [], []
    for chunk in fusion.frame_chunks(dataset, frame_set, False, chunk_frames):
        if tracker is None:
            at_first = fusion.DeviceFrames(chunk.color, chunk.depth, np.tile(first_pose, (len(chunk), 1, 1)))
            bounds = fusion.scene_bounds(at_first, dataset.camera_matrix)
            bounds = bounds + np.array([-1.0, 1.0]) * float(bounds_margin)
            volume = fusion.TSDFVolume(bounds, fusion.voxel_size_for_budget(bounds, options))
            tracker = Tracker(volume, dataset.camera_matrix, first_pose, **icp_options)
        for i in range(len(chunk)):
            results.append(tracker.step(chunk.color[i], chunk.depth[i]))
            poses.append(tracker.pose.copy())
    return tracker.volume, _trajectory(poses), results
