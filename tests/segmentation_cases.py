"""Pictures and the moving-sphere sequence of the segmentation tests.

The pictures are built from the labelling kernel's tile (read from csrc/segment_core.hpp, so that a retune moves the cases with it) and are chosen so that a
wrong merge shows: pixel pairs that touch only diagonally across a tile corner and across each tile edge, a checkerboard, one-pixel-wide serpentines and a
spiral (long equivalence chains whose root is found late), a comb whose teeth join only in the last row (the root lies in the first tile, the merge happens in
the last), and random masks up to the percolation threshold.

The sequence is the room of tests/tracking_cases.py seen from its 12-pose corner orbit at 48 x 64, with a sphere of radius 0.10 m crossing the view at 8.2 cm
per frame, composited analytically: ray-sphere intersection, live = min(room, sphere), truth = sphere < room."""
import os
import re

import numpy as np

import tracking_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_tile():
    """(SEG_TILE_H, SEG_TILE_W) of csrc/segment_core.hpp."""
    text = open(os.path.join(ROOT, "hive_amd", "csrc", "segment_core.hpp")).read()
    return tuple(int(re.search(rf"constexpr int SEG_TILE_{side} = (\d+);", text).group(1)) for side in "HW")


TILE_H, TILE_W = kernel_tile()
# 1 x 1, one row, one column, one more than a tile in both directions of the default tile's smaller side, two tiles by one, and three by two tiles with ragged edges
SIZES = [(1, 1), (1, 200), (200, 1), (33, 65), (64, 64), (97, 131)]
DENSITIES = (0.3, 0.5, 0.593)


def serpentine(h, w, transpose=False):
    """One pixel wide: every other row full, joined to the next at alternating ends."""
    if transpose:
        return np.ascontiguousarray(serpentine(w, h).T)
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for k, r in enumerate(range(1, h, 2)):
        if r + 1 < h:
            m[r, (w - 1) if k % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    """A walk one pixel wide from the top left corner inwards, turning right whenever the next pixel is outside, set, or one pixel from a set one."""
    m = np.zeros((h, w), np.uint8)
    inside = lambda v, u: 0 <= v < h and 0 <= u < w
    v, u, dv, du, turns = 0, 0, 0, 1, 0
    m[0, 0] = 1
    while turns < 2:
        nv, nu, av, au = v + dv, u + du, v + 2 * dv, u + 2 * du
        if inside(nv, nu) and not m[nv, nu] and not (inside(av, au) and m[av, au]):
            v, u, turns = nv, nu, 0
            m[v, u] = 1
        else:
            dv, du, turns = du, -dv, turns + 1
    return m


def comb(h, w):
    """Teeth in every other column from the first row down; they join in the last row alone."""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def diagonal_pairs(h, w):
    """name -> picture of two pixels that touch only diagonally: across a tile corner (both diagonals), across a horizontal and a vertical tile edge away from
    a corner, and inside the first tile; only those that fit the size.  One component under connectivity 8, two under 4."""
    th, tw = TILE_H, TILE_W
    at = {"corner \\": ((th - 1, tw - 1), (th, tw)), "corner /": ((th - 1, tw), (th, tw - 1)),
          "row edge \\": ((th - 1, tw // 2), (th, tw // 2 + 1)), "row edge /": ((th - 1, tw // 2 + 1), (th, tw // 2)),
          "column edge \\": ((th // 2, tw - 1), (th // 2 + 1, tw)), "column edge /": ((th // 2 + 1, tw - 1), (th // 2, tw)),
          "inside": ((0, 0), (1, 1))}
    out = {}
    for name, (p, q) in at.items():
        if max(p[0], q[0]) < h and max(p[1], q[1]) < w:
            m = np.zeros((h, w), np.uint8)
            m[p], m[q] = 1, 1
            out["pair " + name] = m
    return out


def pictures(h, w):
    """name -> uint8 (h, w) picture, in a fixed order."""
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}
    corners = np.zeros((h, w), np.uint8)
    corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 1
    out["corners"] = corners
    out.update(diagonal_pairs(h, w))
    v, u = np.mgrid[0:h, 0:w]
    out["checkerboard"] = ((v + u) % 2 == 0).astype(np.uint8)
    out["serpentine"] = serpentine(h, w)
    out["serpentine, columns"] = serpentine(h, w, transpose=True)
    out["spiral"] = spiral(h, w)
    out["comb"] = comb(h, w)
    rng = np.random.default_rng(20240 + 1000 * h + w)
    for density in DENSITIES:
        out[f"random {density}"] = (rng.random((h, w)) < density).astype(np.uint8) * np.uint8(3)  # (any non-zero value is set)
    return out


def border_masks(h, w):
    """Masks that touch every border, for the opening: a frame one and three pixels thick, and a full picture with a hole."""
    thin, thick, hole = (np.zeros((h, w), np.uint8) for _ in range(3))
    thin[[0, -1], :] = thin[:, [0, -1]] = 1
    thick[:3], thick[-3:], thick[:, :3], thick[:, -3:] = 1, 1, 1, 1
    hole[:] = 1
    hole[h // 2, w // 2] = 0
    return {"frame 1": thin, "frame 3": thick, "hole": hole}


# ---- the moving sphere -------------------------------------------------------------------------------------------------------------------------------------------
SEQ_H, SEQ_W, SEQ_VOXELS, SEQ_FRAMES = 48, 64, 64, 12
SPHERE_RADIUS = 0.10
# What tests/test_segmentation_cpu.py measures with the restatements over the 12 frames and prints: the most pixels of the true silhouette that one opening
# iteration (and the 1 % area filter) removes in a frame.  A recorded CPU measurement, not a tolerance of the GPU tests, which are exact against the CPU chain.
OPENING_FALSE_NEGATIVES_MAX = 2


def sphere_centre(i, n=SEQ_FRAMES):
    s = (i + 0.5) / n
    return tc.PIVOT + np.array([-0.35 + 0.7 * s, -0.05, 0.35 - 0.7 * s]) + np.array([-0.15, -0.10, -0.15])


def sphere_depth(pose, K, height, width, centre, radius=SPHERE_RADIUS):
    """z-depth float32 (H, W) of the nearer intersection of every pixel's ray with the sphere, inf where it misses (float64 arithmetic, rounded at the end)."""
    K = np.asarray(K, np.float64)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)
    c = pose[:3, :3].T @ (np.asarray(centre, np.float64) - pose[:3, 3])
    a, b = (d * d).sum(-1), d @ c
    disc = b * b - a * (c @ c - radius * radius)
    with np.errstate(invalid="ignore"):
        z = (b - np.sqrt(disc)) / a
    return np.where((disc > 0) & (z > 0), z, np.inf).astype(np.float32)


_sequence = {}


def sphere_sequence():
    """dict: K (3, 3), poses (12, 4, 4) camera-to-world, color uint8 (12, H, W, 3), room / live float32 (12, H, W), truth bool (12, H, W).  Built once."""
    if not _sequence:
        K, poses = tc.intrinsics(SEQ_H, SEQ_W), tc.corner_orbit(SEQ_FRAMES)
        color, room, live, truth = [], [], [], []
        for i, pose in enumerate(poses):
            c, r = tc.room_frame(pose, K, SEQ_H, SEQ_W, seed=i)
            s = sphere_depth(pose, K, SEQ_H, SEQ_W, sphere_centre(i))
            color.append(c), room.append(r), live.append(np.minimum(r, s).astype(np.float32)), truth.append(s < r)
        _sequence.update(K=K, poses=poses, color=np.stack(color), room=np.stack(room), live=np.stack(live), truth=np.stack(truth))
        for a in _sequence.values():
            a.setflags(write=False)
    return _sequence


def fuse_sequence(oracle):
    """The oracle volume of 64^3 with all 12 live frames fused in, nothing masked."""
    seq = sphere_sequence()
    vol = oracle.TSDFVolume(tc.bounds(), tc.VOLUME / SEQ_VOXELS)
    for i in range(SEQ_FRAMES):
        vol.integrate(seq["color"][i], seq["live"][i], seq["K"], seq["poses"][i])
    return vol


_cpu_chain = {}


def cpu_chain(oracle):
    """The CPU chain over the sequence, computed once: oracle volume -> raycast_restatement -> (model depth (12, H, W), raw masks uint8 (12, H, W))."""
    if not _cpu_chain:
        import raycast_restatement as rc
        import segmentation_restatement as sr
        seq, vol = sphere_sequence(), fuse_sequence(oracle)
        model = np.stack([rc.raycast(vol._tsdf, vol._weight, vol._color, vol._vol_origin, np.float32(vol._voxel_size), np.float32(vol._trunc_margin), SEQ_H, SEQ_W,
                                     seq["K"], pose)[0] for pose in seq["poses"]])
        _cpu_chain.update(volume=vol, model=model, raw=np.stack([sr.motion_mask(l, m, 0.05) for l, m in zip(seq["live"], model)]))
    return _cpu_chain
