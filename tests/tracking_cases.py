"""Scenes of the ray-cast and tracking tests: the synthetic box room shrunk to [0.16, 1.44]^3 inside a [0, 1.6]^3 volume, seen from look-at poses.

Point-to-plane ICP needs three walls in view to fix all six degrees of freedom, so the tracked poses look towards a room corner; the two-wall view (a
vertical edge, neither floor nor ceiling in the picture) leaves the slide along the edge free and is the scene tracking must report as lost."""
import numpy as np

from hive_amd import synthetic

ROOM_LO, ROOM_HI, VOLUME = 0.16, 1.44, 1.6
CORNER = np.array([ROOM_HI, ROOM_HI, ROOM_HI])
PIVOT = CORNER - np.array([0.45, 0.30, 0.45])  # the point the orbit turns about and looks at, on the way to the floor corner (y points down)
ORBIT_RADIUS = 0.573      # metres, horizontal distance to the pivot: 1.5 degrees of orbit move the camera 15 mm
ORBIT_STEP_DEG = 1.5
ORBIT_DROP = 0.35         # the camera sits this far above the pivot

# What tests/test_tracking_cpu.py measures with the numpy restatements and prints; the bounds of the CPU and the GPU tests are derived from these figures.
# Final translation error of the restated icp_align against the true pose, in voxels: (image H, W, voxels per side) -> error.  The tests allow twice that.
ICP_MEASURED_VOXELS = {(24, 32, 32): 0.0427, (48, 64, 64): 0.0133}
# cond(A): corner scenes 6.6e2 .. 1.9e3 over every level and iteration of both sizes; the two-wall scene is exactly singular (inf).
CORNER_COND_MAX_SEEN = 1.91e3
# ATE RMSE (metres) of the track-and-fuse loop restated on the CPU over the 12-pose orbit at 48 x 64 into 64^3 with 2 levels, and over its first 6 poses
TRACK_ATE_12, TRACK_ATE_6 = 6.32e-4, 6.63e-4


def bounds():
    return synthetic.room_bounds(VOLUME)


def look_at(position, target, roll=0.0):
    """Camera-to-world 4 x 4 float64 of a camera at ``position`` looking at ``target`` (x right, y down, z forward; world y is down), rolled by ``roll``
    radians about its axis."""
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    fwd = target - position
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    c, s = np.cos(roll), np.sin(roll)
    right, down = c * right + s * down, c * down - s * right
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, position
    return pose


def corner_orbit(n=12, start_deg=None):
    """``n`` poses on a horizontal arc about the pivot, looking through it at the floor corner (two walls and the floor in view): steps of 15 mm and 1.5
    degrees, centred on the room's diagonal."""
    start = 45.0 - 0.5 * (n - 1) * ORBIT_STEP_DEG if start_deg is None else start_deg
    poses = []
    for i in range(n):
        th = np.deg2rad(start + i * ORBIT_STEP_DEG)
        position = PIVOT - np.array([ORBIT_RADIUS * np.cos(th), ORBIT_DROP, ORBIT_RADIUS * np.sin(th)])
        poses.append(look_at(position, PIVOT))
    return np.stack(poses)


def two_wall_pose():
    """Looking horizontally at the vertical edge x = z = ROOM_HI from the room's centre: two walls, no floor, no ceiling."""
    return look_at([0.8, 0.8, 0.8], [ROOM_HI, 0.8, ROOM_HI])


def outside_pose():
    """A camera outside the volume looking in at its centre."""
    return look_at([-0.6, 0.5, -0.4], [0.8, 0.8, 0.8])


def away_pose():
    """The first orbit position, looking away from the volume through the nearest face."""
    position = corner_orbit(1)[0][:3, 3]
    return look_at(position, position + np.array([0.0, -1.0, 0.0]) + np.array([1e-3, 0.0, 2e-3]))


def axis_pose():
    """Looking along +z with no rotation at all: with cx a whole number the centre column's rays have a zero x component (likewise the centre row)."""
    pose = np.eye(4)
    pose[:3, 3] = [1.1, 1.15, 0.5]
    return pose


def intrinsics(height, width, whole_centre=False):
    """Kinect intrinsics scaled to the picture; ``whole_centre``: the principal point moved onto a pixel, so that one column and one row of rays are
    parallel to a grid plane."""
    K = synthetic.scaled_intrinsics(height, width)
    if whole_centre:
        K = K.copy()
        K[0, 2], K[1, 2] = float(width // 2), float(height // 2)
    return K


def room_depth(pose, K, height, width):
    """Analytic z-depth float32 (H, W) of the small room and the hit points."""
    return synthetic.raycast_room_depth(pose, K, height, width, ROOM_LO, ROOM_HI)


def room_frame(pose, K, height, width, seed=0):
    """(colour uint8 (H, W, 3), depth float32 (H, W)) of the small room."""
    depth, points = room_depth(pose, K, height, width)
    return synthetic.room_colour(points, np.random.default_rng(seed), VOLUME), depth


def fuse_oracle(oracle, poses, K, height, width, voxels):
    """An oracle volume of ``voxels``^3 with the room's frames at ``poses`` fused in."""
    vol = oracle.TSDFVolume(bounds(), VOLUME / voxels)
    for i, pose in enumerate(poses):
        color, depth = room_frame(pose, K, height, width, seed=i)
        vol.integrate(color, depth, K, pose)
    return vol
