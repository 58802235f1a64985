"""The rules of the ray cast and the tracker themselves, without a GPU: the numpy restatements (tests/raycast_restatement.py, tests/tracking_restatement.py)
over oracle volumes of the small room (tests/tracking_cases.py) against the room's analytic depth and the true poses.  What the kernels are then held to bit
for bit (tests/test_raycast_gpu.py, tests/test_tracking_gpu.py) is shown here to be worth matching; the bounds written here are the ones those tests reuse."""
import os
import re

import numpy as np
import pytest

import tracking_cases as tc
import tracking_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ICP_MEASURED_VOXELS, CORNER_COND_MAX_SEEN, TRACK_ATE_12, TRACK_ATE_6 = tc.ICP_MEASURED_VOXELS, tc.CORNER_COND_MAX_SEEN, tc.TRACK_ATE_12, tc.TRACK_ATE_6


def translation_error_voxels(pose, truth, voxels):
    return float(np.linalg.norm(pose[:3, 3] - truth[:3, 3]) / (tc.VOLUME / voxels))


@pytest.mark.parametrize("frames, bound_voxels", [(1, 0.75), (4, 0.75)])
def test_raycast_depth_against_the_analytic_room(oracle_lib, frames, bound_voxels):
    """48 x 64 into 64^3.  Measured maximum error: 0.572 voxel with 1 frame, 0.625 with 4 (medians 0.063 and 0.022); rounded up to the next quarter voxel.
    Share of pixels with a hit: 0.878 and 0.914."""
    H, W, voxels = 48, 64, 64
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    vol = tc.fuse_oracle(oracle_lib, orbit[:frames], K, H, W, voxels)
    depth = tr.raycast_oracle(vol, K, orbit[0], (H, W))[0]
    truth = tc.room_depth(orbit[0], K, H, W)[0]
    hit = depth > 0
    err = np.abs(depth - truth)[hit] / (tc.VOLUME / voxels)
    print(f"frames {frames}: median {np.median(err):.3f} max {err.max():.3f} voxel, hit share {hit.mean():.3f}")
    assert hit.mean() >= 0.8
    assert err.max() <= bound_voxels


def test_raycast_normals_on_the_walls(oracle_lib):
    """Away from the room's edges by the truncation distance, a ray-cast normal is within 2 degrees of the wall's, and points into the room.

    The frames fused are the sensor's 480 x 640: integrate looks the depth up at the NEAREST pixel, so a voxel's value carries up to half a pixel's change of
    depth, and on a wall seen obliquely that noise is what the central differences pick up -- it has to be small against the 2-voxel baseline.  At 480 x 640 a
    pixel covers 1.7 mm at 1 m against 25 mm voxels (measured: 0.68 degrees with these 4 frames, 1.42 with one); frames of 48 x 64 cover 17 mm and give up to
    9.8 degrees from the same rules -- a property of the fused volume, not of the ray cast.  The ray cast itself is 48 x 64."""
    H, W, voxels = 48, 64, 64
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    vol = tc.fuse_oracle(oracle_lib, orbit[:4], tc.intrinsics(480, 640), 480, 640, voxels)
    depth, _, normal, _ = tr.raycast_oracle(vol, K, orbit[0], (H, W))
    points = tc.room_depth(orbit[0], K, H, W)[1]
    trunc = 5 * tc.VOLUME / voxels
    checked = 0
    for axis in range(3):
        for side, sign in ((tc.ROOM_LO, 1.0), (tc.ROOM_HI, -1.0)):
            others = [a for a in range(3) if a != axis]
            on = np.abs(points[..., axis] - side) < 1e-9
            for a in others:
                on &= (points[..., a] > tc.ROOM_LO + trunc) & (points[..., a] < tc.ROOM_HI - trunc)
            on &= np.abs(normal).sum(axis=-1) > 0
            if not on.any():
                continue
            cosine = sign * normal[on][:, axis].astype(np.float64)
            angle = np.degrees(np.arccos(np.clip(cosine, -1, 1)))
            print(f"axis {axis} side {side}: {int(on.sum())} pixels, max angle {angle.max():.3f} deg")
            assert angle.max() <= 2.0
            assert np.allclose(np.linalg.norm(normal[on].astype(np.float64), axis=1), 1.0, atol=1e-6)
            checked += int(on.sum())
    assert checked >= 0.3 * H * W  # two walls and the floor are in view


@pytest.mark.parametrize("H, W, voxels", [(24, 32, 32), (48, 64, 64)])
def test_frame_to_model_icp_reaches_the_true_pose(oracle_lib, H, W, voxels):
    """The first orbit frame fused, the second aligned from the first's pose (one orbit step away: 15 mm, 1.5 degrees), default settings."""
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    vol = tc.fuse_oracle(oracle_lib, orbit[:1], K, H, W, voxels)
    depth = tc.room_depth(orbit[1], K, H, W)[0]
    res = tr.icp_align(vol, depth, K, orbit[0])
    err = translation_error_voxels(res["pose"], orbit[1], voxels)
    start = translation_error_voxels(orbit[0], orbit[1], voxels)
    print(f"{H} x {W} into {voxels}^3: {start:.3f} -> {err:.4f} voxel, pairs {res['pairs']}, cond(A) {min(res['conds']):.3g} .. {max(res['conds']):.3g}")
    assert res["ok"] and res["iterations_run"] == 19
    assert err <= 2 * ICP_MEASURED_VOXELS[(H, W, voxels)]
    assert max(res["conds"]) <= CORNER_COND_MAX_SEEN * 1.01


@pytest.mark.parametrize("H, W, voxels", [(24, 32, 32), (48, 64, 64)])
def test_two_wall_scene_is_lost_through_max_cond(oracle_lib, H, W, voxels):
    """Two vertical walls leave the slide along their edge free: A is singular, the step has pairs enough, and the default max_cond reports it as lost with the
    pose unchanged.  The corner scenes stay below the default (the test above): that is the evidence for it."""
    from hive_amd import tracking
    K, pose = tc.intrinsics(H, W), tc.two_wall_pose()
    moved = pose.copy()
    moved[:3, 3] += [0.010, 0.012, -0.008]
    vol = tc.fuse_oracle(oracle_lib, [pose], K, H, W, voxels)
    depth = tc.room_depth(moved, K, H, W)[0]
    res = tr.icp_align(vol, depth, K, pose, max_cond=tracking.DEFAULT_MAX_COND)
    coarse = (H // 4) * (W // 4)
    print(f"{H} x {W}: pairs {res['pairs']} of {coarse}, cond(A) {res['cond']:.3g}")
    assert not res["ok"] and np.array_equal(res["pose"], pose)
    assert res["pairs"] >= 0.1 * coarse and res["iterations_run"] == 1
    assert res["cond"] > 1e3 * tracking.DEFAULT_MAX_COND
    assert CORNER_COND_MAX_SEEN < tracking.DEFAULT_MAX_COND


def test_track_loop_on_the_cpu(oracle_lib):
    """The track-and-fuse loop restated (oracle integrate, restated ray cast and ICP) over the corner orbit: every frame tracks; the ATE written above is what
    the GPU test's bound is twice of."""
    from hive_amd.geometric import Trajectory
    H, W, voxels = 48, 64, 64
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    frames = [tc.room_frame(p, K, H, W, seed=i) for i, p in enumerate(orbit)]
    for n, written in ((12, TRACK_ATE_12), (6, TRACK_ATE_6)):
        _, poses, results = tr.track_and_fuse(oracle_lib, [f[0] for f in frames[:n]], [f[1] for f in frames[:n]], K, tc.bounds(), tc.VOLUME / voxels, orbit[0],
                                              levels=2)
        ate = Trajectory.from_homogenous_transforms(np.linalg.inv(orbit[:n])).calculate_ate(Trajectory.from_homogenous_transforms(np.linalg.inv(poses)))
        rmse = float(np.sqrt(np.mean(np.sum(ate ** 2, axis=1))))
        print(f"{n} frames: ATE RMSE {rmse * 1000:.3f} mm")
        assert all(r["ok"] for r in results)
        assert rmse <= 1.25 * written  # the figure written above is this run's, give or take the host's LAPACK


def test_pyramid_rules():
    """A depth step inside a 2 x 2 block on either side of pyr_delta, a block of zeros, and a block with one sample."""
    d = np.array([[1.0, 1.04, 0.0, 0.0, 2.0, 0.0],
                  [1.0, 1.06, 0.0, 0.0, 0.0, 0.0]], np.float32)
    out = tr.pyr_down(d, 0.05)
    assert out.shape == (1, 3)
    assert out[0, 0] == np.float32((np.float32(1.0) + np.float32(1.04) + np.float32(1.0)) / np.float32(3))  # 1.06 is beyond the nearest sample + 0.05
    assert out[0, 1] == 0 and out[0, 2] == 2
    K = tr.level_intrinsics(tc.intrinsics(48, 64), 3)
    assert np.allclose(K[1, :2, 2], (tc.intrinsics(48, 64)[:2, 2] - 0.5) / 2) and K[2, 0, 0] == tc.intrinsics(48, 64)[0, 0] / 4


def test_entry_points_are_declared():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    for name in ("hive_tsdf_raycast", "hive_frame_maps", "hive_icp_step"):
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    assert _lib.ABI_VERSION >= 6


def test_tracking_imports_without_a_gpu():
    """Like the other modules: importable, its host helpers usable, and an error only at the point of use."""
    import torch
    from hive_amd import _lib, tracking
    xi = np.array([0.01, -0.02, 0.03, 0.1, 0.2, 0.3])
    T = tracking.se3_exp(xi)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15) and np.array_equal(T[:3, 3], xi[3:])
    assert np.array_equal(T, tr.se3_exp(xi))
    assert tracking.level_iterations((10, 5, 4), 2) == [4, 5] and tracking.level_iterations((10, 5, 4), 3) == [4, 5, 10]
    sums = np.arange(28, dtype=np.float64)
    A, b, rr = tracking.normal_equations(sums)
    assert np.array_equal(A, A.T) and A[0, 5] == 5 and A[1, 1] == 6 and A[5, 5] == 20 and b[0] == 21 and rr == 27
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HiveError):
            tracking.frame_maps(np.ones((4, 4), np.float32), np.eye(3))
