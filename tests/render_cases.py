"""Scenes with known answers for the rasteriser's tests (test_render_cpu.py pins them on the numpy restatement, test_render_gpu.py renders them on the GPU)."""
import numpy as np
from scipy.spatial.transform import Rotation

IDENTITY = np.eye(4)


def intrinsics(H, W, focal=58.0):
    """24 x 32 -> [[58, 0, 15.5], [0, 58, 11.5], [0, 0, 1]]: the principal point in the middle of the pixel grid."""
    return np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def general_pose():
    """A world-to-camera transform with nothing special about it."""
    M = np.eye(4)
    M[:3, :3] = Rotation.from_euler("xyz", [0.31, -0.52, 1.1]).as_matrix()
    M[:3, 3] = [-2.56, 1.7, 0.45]
    return M


def to_world(points_cam, pose):
    """The world points that `pose` maps onto the camera points."""
    return (pose[:3, :3].T @ (np.asarray(points_cam, np.float64).T - pose[:3, 3:4])).T


def unproject(K, u, v, z):
    u, v, z = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(z, np.float64))
    return np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], -1).reshape(-1, 3)


def grid_scene(H, W, seed=0, pose=IDENTITY):
    """The full grid mesh of a random depth image (two triangles per cell), its vertices on the pixels: rendered from its own pose it covers exactly the block
    [0:H-1, 0:W-1], each pixel once, with the image's depth bits; textured through atlas-convention uv (or coloured per vertex) it returns `image` there.
    -> dict(K, depth float32, image uint8, coloured mesh, textured mesh)."""
    rng = np.random.default_rng(seed)
    K = intrinsics(H, W)
    depth = (1.5 + 0.3 * rng.random((H, W))).astype(np.float32)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ii, jj = np.mgrid[0:H, 0:W]
    vertices = to_world(unproject(K, jj, ii, depth.astype(np.float64)), pose)
    idx = np.arange(H * W).reshape(H, W)
    faces = np.concatenate([np.stack([idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:]], -1).reshape(-1, 3),
                            np.stack([idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)]).astype(np.int32)
    uv = np.stack([jj.reshape(-1), ii.reshape(-1)], -1).astype(np.float64) / np.array([float(W), float(H)])
    uv[:, 1] = 1.0 - uv[:, 1]  # pack_textures_row's convention
    return {"K": K, "depth": depth, "image": image,
            "coloured": {"vertices": vertices, "faces": faces, "vertex_colors": image.reshape(-1, 3)},
            "textured": {"vertices": vertices, "faces": faces, "uv": uv, "texture": image}}


def coloured(vertices, faces, seed=1):
    rng = np.random.default_rng(seed)
    return {"vertices": np.asarray(vertices, np.float64), "faces": np.asarray(faces, np.int32),
            "vertex_colors": rng.integers(0, 256, (len(vertices), 3), dtype=np.uint8)}


def quad_scene(H, W, pose=IDENTITY):
    """Two triangles at z = 2 that reach beyond the screen on every side: every pixel covered exactly once (the shared diagonal too), depth bits of 2.0f."""
    K = intrinsics(H, W)
    corners = unproject(K, [-8.0, W + 16.0, W + 16.0, -8.0], [-8.0, -8.0, H + 12.0, H + 12.0], 2.0)
    return K, coloured(to_world(corners, pose), [[0, 1, 2], [0, 2, 3]])


def fan_scene(H, W, seed=0, spokes=17):
    """A fan of `spokes` faces around an off-grid centre: no pixel is covered twice."""
    rng = np.random.default_rng(seed)
    K = intrinsics(H, W)
    angle = np.sort(rng.random(spokes)) * 2 * np.pi
    centre = np.array([0.489 * W, 0.473 * H])
    radius = 0.375 * min(H, W) * (0.5 + rng.random(spokes))
    points = np.vstack([centre, np.c_[centre[0] + radius * np.cos(angle), centre[1] + radius * np.sin(angle)]])
    return K, coloured(unproject(K, points[:, 0], points[:, 1], 3.0), [[0, 1 + k, 1 + (k + 1) % spokes] for k in range(spokes)])


def tie_scene(H, W):
    """Three coincident faces (one with the other winding): face 0 wins everywhere."""
    K = intrinsics(H, W)
    a, b = 5.0 / 64.0 * W, 40.0 / 64.0 * min(H, W)
    return K, coloured(unproject(K, [a, b, a], [a, a, b], 2.0), [[0, 1, 2], [0, 1, 2], [2, 1, 0]])
