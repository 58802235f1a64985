"""Cases at which the compactions of csrc/fgmesh.hip and csrc/mesh_compact.hpp scan MORE than 1024 block counts (scan_counts_kernel, scan_counts_box_kernel:
every scan thread takes a run of per > 1 counts, and the last run is ragged), and the rules they are compared against in plain numpy
(tests/test_fgmesh_cases_cpu.py proves on the CPU that the shapes reach that path; tests/test_fgmesh_gpu.py runs them).  No GPU, no library of this project."""
import numpy as np

TILE = 1024          # mesh_compact.hpp: pixels / faces / vertices per workgroup of the count and place kernels
SCAN_THREADS = 1024  # hive_internal.hpp: one workgroup of 1024 threads, thread t scans the block counts [t per, t per + per)

# hive_grid_mesh: a picture of 1026 whole tiles and ONE pixel.  Two bands (rows / columns, each at least two thick) are masked out, and the depth steps by a
# metre at one column: hive_filter_faces then drops the faces across the step
GRID_SIZE = (1025, 1025)
GRID_ROW_BAND, GRID_COL_BAND, GRID_STEP_COLUMN = (400, 403), (600, 602), 700
SMALL_SIZE = (23, 31)
SMALL_ROW_BAND, SMALL_COL_BAND, SMALL_STEP_COLUMN = (9, 11), (13, 16), 20
PASS_ALL_LIMITS = (5.0, 10.0)  # (max_pixel_distance, max_depth_distance): every face of the grid passes
STEP_LIMITS = (2.0, 0.1)       # the faces across the depth step do not

# hive_mesh_cleanup_cc: the lattice mesh of a 726 x 726 picture, fully valid but for a one-pixel ring around a 4 x 4 patch in the middle: the patch is a
# component of 18 faces, below CLEANUP_MIN_FACES; the ring's pixels are vertices that no face references
CLEANUP_SIZE = (726, 726)
CLEANUP_PATCH = (360, 364)  # rows and columns of the patch; the ring lies around it
CLEANUP_MIN_FACES = 25


def scan_shape(n_items):
    """(nb, per, scan threads with an empty run) of a scan over the tiles of n_items."""
    nb = -(-n_items // TILE)
    per = -(-nb // SCAN_THREADS)
    lo = np.minimum(np.arange(SCAN_THREADS) * per, nb)
    hi = np.minimum(lo + per, nb)
    return nb, per, np.flatnonzero(lo == hi)


def banded_scene(size, row_band, col_band, step_column):
    """(depth float32, mask bool): every pixel valid outside a band of rows and a band of columns; 2 m left of step_column, 3 m from it on."""
    H, W = size
    mask = np.ones((H, W), bool)
    mask[row_band[0]:row_band[1], :] = False
    mask[:, col_band[0]:col_band[1]] = False
    depth = np.where(np.arange(W)[None, :] < step_column, np.float32(2.0), np.float32(3.0)) * np.ones((H, 1), np.float32)
    return depth, mask


def full_block_faces(valid, pixel_ids=False):
    """The implicit triangulation where no 2 x 2 block has exactly three valid corners and no hole is bridged: (a, c, b), (b, c, d) for each fully valid
    block, blocks in raster order.  int32 (F, 3) of rows of point_cloud_from_depth (the valid pixels in raster order), or with pixel_ids of pixel numbers
    (an invalid pixel is then a vertex that no face references)."""
    vid = -np.ones(valid.shape, np.int64)
    vid[valid] = np.flatnonzero(valid.reshape(-1)) if pixel_ids else np.arange(int(valid.sum()))
    a, b, c, d = vid[:-1, :-1], vid[:-1, 1:], vid[1:, :-1], vid[1:, 1:]
    full = (a >= 0) & (b >= 0) & (c >= 0) & (d >= 0)
    return np.stack([a[full], c[full], b[full], b[full], c[full], d[full]], axis=1).reshape(-1, 3).astype(np.int32)


def cleanup_valid():
    """The 726 x 726 picture's valid pixels: all but the ring around the patch."""
    valid = np.ones(CLEANUP_SIZE, bool)
    lo, hi = CLEANUP_PATCH
    valid[lo - 1:hi + 1, lo - 1:hi + 1] = False
    valid[lo:hi, lo:hi] = True
    return valid
