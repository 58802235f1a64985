"""The premises of the long-scan tests of tests/test_fgmesh_gpu.py, on the CPU: that the three shapes of tests/fgmesh_cases.py give the two-array scans of
csrc/fgmesh.hip (scan_counts_kernel behind hive_grid_mesh and hive_filter_faces, scan_counts_box_kernel behind the compaction of mesh_compact.hpp) more than
1024 block counts, no whole number of runs, and a ragged last tile -- recomputed from the kernels' constants, restated in fgmesh_cases."""
import numpy as np

import fgmesh_cases as fc


def _grid_counts():
    depth, mask = fc.banded_scene(fc.GRID_SIZE, fc.GRID_ROW_BAND, fc.GRID_COL_BAND, fc.GRID_STEP_COLUMN)
    valid = mask & (depth > 0)
    full = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
    return valid, full


def test_grid_mesh_size_reaches_the_long_scan():
    H, W = fc.GRID_SIZE
    n = H * W
    nb, per, empty = fc.scan_shape(n)
    # 1026 whole tiles and one pixel; two block counts per scan thread, thread 513 with one only, threads 514 .. 1023 with none
    assert (nb, per) == (1027, 2) and nb > fc.SCAN_THREADS and nb % fc.SCAN_THREADS != 0 and n - (nb - 1) * fc.TILE == 1
    assert list(empty) == list(range(514, 1024)) and nb - 513 * per == 1
    valid, full = _grid_counts()
    assert valid[-1, -1], "the one pixel of the last tile is a vertex"
    # the block counts are not constant: per tile of 1024 pixels in raster order, the valid pixels and the faces (two per fully valid block, at its corner a)
    pad = nb * fc.TILE - n
    cv = np.pad(valid.reshape(-1), (0, pad)).reshape(nb, fc.TILE).sum(axis=1)
    cf = 2 * np.pad(np.pad(full, ((0, 1), (0, 1))).reshape(-1), (0, pad)).reshape(nb, fc.TILE).sum(axis=1)
    assert len(np.unique(cv)) > 3 and len(np.unique(cf)) > 3 and cv.min() == 0 and cv.max() < fc.TILE, "tiles inside the row band are empty, none is full"
    assert cv[-1] == 1 and cf[-1] == 0 and cv.sum() == valid.sum() and cf.sum() == 2 * full.sum()
    for band in (fc.GRID_ROW_BAND, fc.GRID_COL_BAND, fc.SMALL_ROW_BAND, fc.SMALL_COL_BAND):
        assert band[1] - band[0] >= 2, "a band two thick: none of its pixels has three valid 4-neighbours, so no hole is bridged"


def test_filter_faces_input_reaches_the_long_scan():
    valid, full = _grid_counts()
    n_faces = 2 * int(full.sum())
    rows = fc.GRID_SIZE[0] - 1 - (fc.GRID_ROW_BAND[1] - fc.GRID_ROW_BAND[0] + 1)
    cols = fc.GRID_SIZE[1] - 1 - (fc.GRID_COL_BAND[1] - fc.GRID_COL_BAND[0] + 1)
    assert n_faces == 2 * rows * cols == 2 * 1020 * 1021
    nb, per, empty = fc.scan_shape(n_faces)
    # (a picture of 1025 x 1025 has at most 2 * 1024^2 faces = 2048 tiles: two block counts per scan thread is what this face list can reach)
    assert (nb, per) == (2035, 2) and nb > fc.SCAN_THREADS and nb % fc.SCAN_THREADS != 0
    assert n_faces - (nb - 1) * fc.TILE == 24, "a ragged last tile"
    assert list(empty) == list(range(1018, 1024)) and nb - 1017 * per == 1
    # the depth step drops faces in every row of blocks, so in (nearly) every tile: the block column left of the step
    assert fc.GRID_COL_BAND[1] < fc.GRID_STEP_COLUMN < fc.GRID_SIZE[1] - 1 and fc.STEP_LIMITS[1] < 1.0 < fc.PASS_ALL_LIMITS[1]


def test_cleanup_mesh_reaches_the_long_scan_with_both_arrays():
    valid = fc.cleanup_valid()
    H, W = fc.CLEANUP_SIZE
    faces = fc.full_block_faces(valid, pixel_ids=True)
    lo, hi = fc.CLEANUP_PATCH
    # the ring costs the 2 x 2 blocks that touch it: the 7 x 7 blocks around the patch but for the patch's own 3 x 3
    assert len(faces) == 2 * (H - 1) * (W - 1) - 2 * (49 - 9) == 1051170
    nbf, nbv = -(-len(faces) // fc.TILE), -(-(H * W) // fc.TILE)
    assert (nbf, nbv) == (1027, 515), "face tiles and vertex tiles; both arrays are scanned over max(nbf, nbv) counts, the vertices' with a tail of zeros"
    nb, per, empty = fc.scan_shape(len(faces))
    assert (nb, per) == (1027, 2) and nb > fc.SCAN_THREADS and nb % fc.SCAN_THREADS != 0 and len(faces) - (nb - 1) * fc.TILE == 546 and (H * W) % fc.TILE != 0
    assert list(empty) == list(range(514, 1024))
    # what goes: the patch's 18 faces (a component below the limit) from the middle of the list, and the ring's 20 vertices, which no face references
    patch = np.zeros((H, W), bool)
    patch[lo:hi, lo:hi] = True
    in_patch = patch.reshape(-1)[faces].all(axis=1)
    assert in_patch.sum() == 18 < fc.CLEANUP_MIN_FACES and not patch.reshape(-1)[faces[~in_patch]].any()
    at = np.flatnonzero(in_patch)
    assert fc.TILE < at.min() and at.max() < len(faces) - fc.TILE and len(np.unique(at // fc.TILE)) >= 2
    assert (~valid).sum() == 20
