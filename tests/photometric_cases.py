"""Scenes of the photometric tracking tests, on top of tests/tracking_cases.py: the two-wall view, which point-to-plane ICP alone reports as lost (its normal
matrix is singular: the slide along the walls' edge is free), as one alignment and as a slide of 8 poses; and the corner orbit, where geometry already fixes
the pose and the colour term can only cost accuracy.  The room's colour (hive_amd.synthetic.room_colour) is a smooth pattern with noise of sigma 4 grey levels
per frame; the model's colour is the nearest voxel's."""
import numpy as np

import tracking_cases as tc

TWO_WALL_MOVE = np.array([0.010, 0.012, -0.008])   # metres: the live frame of the two-wall alignment
SLIDE_STEP = np.array([0.006, 0.010, -0.005])      # metres per pose of the two-wall slide
SLIDE_POSES = 8
WEIGHTS = (0.03, 0.1)                              # metres per unit of intensity

# What tests/test_photometric_cpu.py measures with the numpy restatements and prints; the bounds of the CPU and the GPU tests are derived from these figures.
# Two-wall icp_align with photometric_weight = 0.1, defaults otherwise: (image H, W, voxels per side) -> final translation error in voxels (it starts at
# 0.351 and 0.702 voxel), and the largest cond(A) of the combined normal equations over every level and iteration.  Without colour both are lost (cond = inf).
TWO_WALL_MEASURED_VOXELS = {(24, 32, 32): 0.0602, (48, 64, 64): 0.0330}
TWO_WALL_COND_MAX_SEEN = {(24, 32, 32): 4.16e3, (48, 64, 64): 1.33e3}
# ATE RMSE (metres) of the track-and-fuse loop restated on the CPU at 48 x 64 into 64^3 (25 mm voxels) with 2 levels: weight -> figure
SLIDE_ATE = {0.03: 1.328e-3, 0.1: 1.194e-3}                # the 8-pose two-wall slide; without colour every frame after the first is lost
ORBIT_ATE = {0.03: 6.37e-4, 0.1: 2.074e-3}                # the 12-pose corner orbit; without colour tracking_cases.TRACK_ATE_12 = 0.632 mm


def two_wall_scene(oracle, H, W, voxels):
    """K, an oracle volume with the two-wall frame fused, its pose, the true pose of the live frame and that frame (colour seed 1, as test_tracking_gpu.py)."""
    K, pose = tc.intrinsics(H, W), tc.two_wall_pose()
    moved = pose.copy()
    moved[:3, 3] += TWO_WALL_MOVE
    vol = tc.fuse_oracle(oracle, [pose], K, H, W, voxels)
    color, depth = tc.room_frame(moved, K, H, W, seed=1)
    return dict(K=K, vol=vol, voxels=voxels, pose=pose, moved=moved, color=color, depth=depth)


def slide_poses(n=SLIDE_POSES):
    poses = np.tile(tc.two_wall_pose(), (n, 1, 1))
    for i in range(n):
        poses[i, :3, 3] += i * SLIDE_STEP
    return poses


def frames(poses, H=48, W=64):
    """K, colour frames and depth frames of the small room at ``poses`` (colour seed = the frame's index)."""
    K = tc.intrinsics(H, W)
    pairs = [tc.room_frame(p, K, H, W, seed=i) for i, p in enumerate(poses)]
    return K, [f[0] for f in pairs], [f[1] for f in pairs]


def ate_rmse(truth_c2w, poses_c2w):
    from hive_amd.geometric import Trajectory
    inv = lambda p: Trajectory.from_homogenous_transforms(np.linalg.inv(np.asarray(p)))
    ate = inv(truth_c2w).calculate_ate(inv(poses_c2w))
    return float(np.sqrt(np.mean(np.sum(ate ** 2, axis=1))))
