"""Meshes and area tables shared by tests/test_texture_smoothing_cpu.py (the numpy restatement) and tests/test_texture_smoothing_gpu.py (the kernels)."""
import functools

import numpy as np

import texture_smoothing_restatement as SR


def grid(nx, ny, num_faces=None):
    """(faces (2 nx ny, 3) int32, vertex count) of an nx x ny grid of squares cut into two triangles each; ``num_faces``: only the first so many."""
    i, j = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v00 = (i * (nx + 1) + j).reshape(-1)
    v10, v01, v11 = v00 + 1, v00 + nx + 1, v00 + nx + 2
    faces = np.stack([np.stack([v00, v10, v01], axis=1), np.stack([v11, v01, v10], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    return (faces if num_faces is None else faces[:num_faces]), (nx + 1) * (ny + 1)


def fan(m):
    """m faces on the edge (0, 1): every face lists the m - 1 others."""
    return np.stack([np.zeros(m, np.int32), np.ones(m, np.int32), np.arange(2, m + 2, dtype=np.int32)], axis=1), m + 2


TETRAHEDRON = (np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32), 4)

NEIGHBOUR_CASES = {
    "one face": (np.array([[0, 1, 2]], np.int32), 3),
    "two faces on an edge": (np.array([[0, 1, 2], [2, 1, 3]], np.int32), 4),
    "tetrahedron": TETRAHEDRON,
    "fan of 5": fan(5),
    "fan of 64": fan(64),
    "duplicate faces": (np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 2, 3]], np.int32), 4),
    "a repeated id and an id out of range": (np.array([[0, 1, 2], [1, 1, 2], [2, 1, 3], [0, 2, 4], [3, 1, 7], [-1, 0, 1], [0, 3, 1]], np.int32), 5),
    "255 faces": grid(16, 8, 255),
    "256 faces": grid(16, 8, 256),
    "257 faces": grid(16, 9, 257),
    "32 x 32": grid(32, 32),
}

# the smoothing meshes of the GPU test: (faces, vertex count, views)
SMOOTH_MESHES = {"8 x 8": grid(8, 8) + (2,), "16 x 16": grid(16, 16) + (4,), "32 x 32": grid(32, 32) + (8,), "fan of 64": fan(64) + (3,)}
FAMILIES = ("random", "tied", "small")
SEAM_COSTS = (0, 1, 100, 10 ** 6)


def table(family, n, nf, seed=0):
    """int64 (n, nf): ``random`` areas in 1 .. 999 (one entry in twenty 0), ``tied`` one value with a unit added to view f mod n of face f, ``small`` areas in
    1 .. 3; about a tenth of the faces have no view at all."""
    rng = np.random.default_rng(1000 + seed + 17 * n + nf)
    if family == "random":
        area = rng.integers(1, 1000, (n, nf))
        area[rng.random((n, nf)) < 0.05] = 0
    elif family == "tied":
        area = np.full((n, nf), 500)
        area[np.arange(nf) % n, np.arange(nf)] += 1
    else:
        area = rng.integers(1, 4, (n, nf))
    area[:, rng.random(nf) < 0.1] = 0
    return area.astype(np.int64)


@functools.lru_cache(maxsize=None)
def adjacency(name):
    faces, nv, _ = SMOOTH_MESHES[name]
    return SR.face_neighbours(faces, nv)


@functools.lru_cache(maxsize=None)
def smoothed(name, family, seam_cost):
    """The restatement's (best, labels, stats) of one combination, computed once for all tests."""
    faces, _, n = SMOOTH_MESHES[name]
    offsets, neighbours = adjacency(name)
    return SR.smooth(table(family, n, len(faces)), offsets, neighbours, seam_cost)
