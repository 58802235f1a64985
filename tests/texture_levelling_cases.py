"""Cases shared by tests/test_texture_levelling_cpu.py (the numpy restatement) and tests/test_texture_levelling_gpu.py (the kernels): the scaled-frame room, the
hand cases of the levelling, and small meshes with given labels.  Restated results are computed once and shared."""
import functools

import numpy as np

import texture_levelling_restatement as LR
import texture_smoothing_cases as SC
import texturing_cases as C

# per-channel exposure factors of the key frames: two views (frames 0 and 2 of the room), three views (frame 1 keeps its exposure)
FACTORS = {2: ((0.85, 0.80, 0.90), (1.15, 1.20, 1.10)), 3: ((0.85, 0.80, 0.90), (1.0, 1.0, 1.0), (1.15, 1.20, 1.10))}
ROOM_FRAMES = {2: [0, 2], 3: [0, 1, 2]}


def scaled(frames, factors):
    """The frames multiplied per view and channel, rounded into bytes."""
    f = np.asarray(factors, np.float64)[:, None, None, :]
    return np.clip(np.floor(np.asarray(frames, np.float64) * f + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def room(n_views):
    """The fused room of texturing_cases with the frames of FACTORS: dict(mesh, K, poses, clean, frames, factors, all_clean, all_poses)."""
    mesh, seq, w2c = C.room()
    pick = ROOM_FRAMES[n_views]
    return dict(mesh=mesh, K=seq["K"].astype(np.float64), poses=w2c[pick], clean=seq["color"][pick], frames=scaled(seq["color"][pick], FACTORS[n_views]),
                factors=np.asarray(FACTORS[n_views]), all_clean=seq["color"], all_poses=w2c)


@functools.lru_cache(maxsize=None)
def room_restated(n_views, exposure, levelling, sweeps=64, reverse=False):
    r = room(n_views)
    order = slice(None, None, -1) if reverse else slice(None)
    return LR.texture_mesh(r["mesh"], r["frames"][order], r["K"], r["poses"][order], exposure=exposure, levelling=levelling, levelling_sweeps=sweeps)


# ---------------------------------------------------------------------------------------------------------------- levelling by hand
COLOUR_A, COLOUR_B = (40, 100, 200), (60, 80, 180)


def two_quads():
    """Two coplanar squares sharing the edge (1, 4) on z = 1 of the identity camera (screen 16 | 32 | 48 x 16 | 32), the left one labelled view 0 and the right one
    view 1; constant frames of colours A and B.  Vertices: 0 1 2 / 3 4 5."""
    faces, nv = SC.grid(2, 1)
    xs, ys = [(s - 32.0) / 32.0 for s in (16.0, 32.0, 48.0)], [(s - 24.0) / 32.0 for s in (16.0, 32.0)]
    vertices = np.array([[x, y, 1.0] for y in ys for x in xs], np.float64)
    frames = np.empty((2, C.H, C.W, 3), np.uint8)
    frames[0], frames[1] = COLOUR_A, COLOUR_B
    mesh = dict(vertices=vertices, faces=faces, vertex_colors=np.full((nv, 3), 128, np.uint8))
    return dict(mesh=mesh, labels=np.array([0, 0, 1, 1], np.int32), frames=frames, poses=np.stack([C.IDENTITY, C.IDENTITY]), q=None)


# ---------------------------------------------------------------------------------------------------------------- meshes with given labels
def _surface(faces, nv, positions, labels, n, seed):
    rng = np.random.default_rng(500 + seed)
    mesh = dict(vertices=np.asarray(positions, np.float64), faces=np.asarray(faces, np.int32), vertex_colors=rng.integers(0, 256, (nv, 3), dtype=np.uint8))
    return dict(mesh=mesh, labels=np.asarray(labels, np.int32), frames=C.frames_for(n, seed), poses=C.random_poses(n, seed),
                q=rng.integers(40000, 90000, (n, 3)).astype(np.uint32))


def _grid_positions(nx, ny):
    i, j = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    return np.stack([-0.9 + 1.8 * j / nx, -0.6 + 1.2 * i / ny, 2.0 + 0.1 * np.sin(i + j)], axis=-1).reshape(-1, 3)


def fan_of_40():
    """40 faces round vertex 0, four sectors of ten faces labelled 0, 1, 2, 0: the centre is a seam vertex of three labels."""
    m = 40
    ring = 1 + np.arange(m)
    faces = np.stack([np.zeros(m, np.int64), ring, 1 + (np.arange(m) + 1) % m], axis=1)
    angle = 2 * np.pi * np.arange(m) / m
    positions = np.concatenate([[[0.0, 0.0, 2.0]], np.stack([0.5 * np.cos(angle), 0.5 * np.sin(angle), np.full(m, 2.1)], axis=1)])
    return _surface(faces, m + 1, positions, (np.arange(m) // 10) % 3, 3, 1)


def three_on_an_edge():
    faces, nv = SC.fan(3)
    positions = [[0.0, -0.3, 2.0], [0.0, 0.3, 2.0], [0.4, 0.0, 2.0], [-0.4, 0.0, 2.0], [0.0, 0.0, 1.6]]
    return _surface(faces, nv, positions, [0, 1, 0], 2, 2)


def patched_grid():
    """12 x 12 squares (288 faces, 864 corners: more than one workgroup) in four label patches over three views."""
    faces, nv = SC.grid(12, 12)
    square = np.arange(144)
    labels = np.repeat(((square // 12 >= 6) * 2 + (square % 12 >= 6)) % 3, 2)
    return _surface(faces, nv, _grid_positions(12, 12), labels, 3, 3)


def broken_grid():
    """4 x 4 squares with a face that repeats an id, a face with an id out of range, unlabelled faces and a label no view has."""
    faces, nv = SC.grid(4, 4)
    faces = faces.copy()
    faces[5, 1] = faces[5, 0]
    faces[9, 2] = nv + 3
    rng = np.random.default_rng(77)
    labels = rng.integers(-1, 3, len(faces))
    labels[12] = 7
    return _surface(faces, nv, _grid_positions(4, 4), labels, 3, 4)


LEVEL_CASES = {"two quads": two_quads, "fan of 40": fan_of_40, "three faces on an edge": three_on_an_edge, "patched grid": patched_grid, "broken grid": broken_grid}
SWEEPS = (0, 1, 64)


@functools.lru_cache(maxsize=None)
def level_case(name):
    return LEVEL_CASES[name]()


@functools.lru_cache(maxsize=None)
def levelled(name, sweeps):
    case = level_case(name)
    return LR.level(case["mesh"], case["labels"], case["frames"], C.K, case["poses"], case["q"], sweeps)


# ---------------------------------------------------------------------------------------------------------------- sums
SUM_FACES, SUM_VIEWS = (1, 2, 3, 255, 256, 257, 513), (1, 2, 3, 33)


def sum_case(nf, n, with_masks):
    seed = nf * 5 + n
    return dict(mesh=C.soup(nf, seed), frames=C.frames_for(n, seed), poses=C.random_poses(n, seed), masks=C.masks_for(n, seed) if with_masks else None)
