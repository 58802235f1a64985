"""The premises of tests/test_geometry_edges_gpu.py, on the CPU: that each case of tests/geometry_cases.py reaches the guarded path of csrc/geometry.hip it is
there for (recomputed from the kernels' constants, restated below), that the ties are exact ties and split the two rounding modes, and that the oracle at
these shapes is the reference's formula."""
import numpy as np
import pytest

import geometry_cases as gc
import tracking_restatement as tr

UP_TILE = 1024        # unproject_count_kernel / unproject_write_kernel: pixels per workgroup (256 threads x UP_VPT)
UP_VPT = 4            # the same kernels: consecutive pixels per thread
SCAN_THREADS = 1024   # scan_counts_kernel: one workgroup of 1024 threads, thread t scans blocks [t per, t per + per)
LANES = 256           # max_depth_batch_kernel, depth_quantize_kernel, project_kernel, image2world_kernel: threads per workgroup
WAVE = 64             # max_depth_batch_kernel: the shuffle reduction is per wave of 64
FRUSTUM_GROUPS = 1024       # hive_view_frustum: at most 1024 workgroups for one frame
FRUSTUM_BATCH_GROUPS = 64   # hive_view_frustum_batch: at most 64 workgroups per frame
F64_TOL = dict(rtol=1e-14, atol=1e-14)  # tests/test_geometry_gpu.py::test_full_resolution_checksums_and_oracle against the oracle


def _scan_shape(n):
    nb = -(-n // UP_TILE)
    per = -(-nb // SCAN_THREADS)
    lo = np.minimum(np.arange(SCAN_THREADS) * per, nb)
    hi = np.minimum(lo + per, nb)
    return nb, per, np.flatnonzero(lo == hi)


def test_unproject_sizes_reach_the_ragged_tile_and_the_long_scan():
    rows = {}
    for H, W in gc.UNPROJECT_SIZES:
        n = H * W
        nb, per, empty = _scan_shape(n)
        assert n % UP_TILE != 0, "a whole number of tiles never makes `base + j < n` false"
        rows[(H, W)] = (n, nb, per, len(empty))
    assert rows[(1, 1)] == (1, 1, 1, 1023) and rows[(5, 7)] == (35, 1, 1, 1023)
    assert 1 % UP_VPT and 35 % UP_VPT, "one thread is partly filled"
    assert rows[(37, 53)] == (1961, 2, 1, 1022) and 1961 % UP_VPT == 1 and 0 < 1961 - UP_TILE < UP_TILE
    assert rows[(33, 31)] == (UP_TILE - 1, 1, 1, 1023)
    # 1026 whole tiles and one pixel: nb = 1027, two blocks per scan thread, thread 513 with one block only, threads 514 .. 1023 with lo == hi == nb
    assert rows[(1025, 1025)] == (1050625, 1027, 2, 510) and 1025 * 1025 - 1026 * UP_TILE == 1
    assert list(_scan_shape(1025 * 1025)[2]) == list(range(514, 1024))
    # what the existing tests run: whole tiles, one block per scan thread
    for H, W in ((48, 64), (480, 640)):
        assert (H * W) % UP_TILE == 0 and _scan_shape(H * W)[1] == 1


@pytest.mark.parametrize("size", gc.UNPROJECT_SIZES)
def test_unproject_case_forces_the_pixels_a_lost_tail_would_lose(size):
    H, W = size
    c = gc.unproject_case(H, W, seed=H * 1000 + W)
    valid = (c["mask"] & (c["depth"] > 0)).reshape(-1)
    n = H * W
    assert valid[-1], "the last pixel is valid"
    if n > UP_TILE:
        last_whole = (n - 1) // UP_TILE * UP_TILE - 1
        assert valid[last_whole] and (last_whole + 1) % UP_TILE == 0 and n - (last_whole + 1) < UP_TILE
    if n >= 35:
        assert 0.75 < c["mask"].mean() <= 1.0 and 0.0 < (c["depth"] == 0).mean() < 0.25
    assert c["depth"].dtype == np.float32 and c["K"].dtype == np.float32 and c["rgb"].dtype == np.uint8
    assert c["depth"].max() <= 5.0 and c["depth"][c["depth"] > 0].min() >= 0.5
    R = c["R"]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)
    assert np.abs(R - np.eye(3)).min() > 0.05, "a general rotation: no entry is the identity's"


def test_frustum_and_quantize_sizes_reach_the_stride_and_the_tail():
    (h0, w0), (h1, w1) = gc.FRUSTUM_SIZES
    n0, n1 = h0 * w0, h1 * w1
    groups0 = min(-(-n0 // LANES), FRUSTUM_GROUPS)
    assert groups0 * LANES > n0 and (n0 - 1) // LANES == groups0 - 1, "the last pixel is in the last workgroup, which is ragged"
    wave_start = (n0 - 1) // WAVE * WAVE
    assert wave_start < n0 < wave_start + WAVE, "and in a wave that is only partly inside the image"
    assert -(-n1 // LANES) == 1026 > FRUSTUM_GROUPS and (n1 - 1) // LANES >= FRUSTUM_GROUPS, "the last pixels are reached by the stride alone"
    assert -(-(120 * 160) // LANES) == 75 <= FRUSTUM_GROUPS, "the existing single-frame tests launch a workgroup per 256 pixels"
    assert -(-n0 // LANES) <= FRUSTUM_BATCH_GROUPS < -(-n1 // LANES), "the batch form: a workgroup per 256 pixels at the first size, the stride at the second"
    for H, W in gc.FRUSTUM_SIZES:
        d = gc.frustum_case(H, W)["depth"].reshape(-1)
        assert d.argmax() == H * W - 1 and d[0] > 0 and d[0] < d[-1] and np.count_nonzero(d) == 2 and d.min() == 0
    qh, qw = gc.QUANTIZE_SIZE
    assert (qh * qw) % LANES != 0 and (48 * 64) % LANES == 0
    n_pts = gc.TIE_COUNT + gc.NON_TIES
    assert len(gc.tie_points()) == n_pts and n_pts % LANES != 0 and n_pts > LANES


def test_tie_points_are_exact_ties_and_split_the_modes(oracle_lib):
    pts = gc.tie_points()
    K, R, t = gc.TIE_K, np.eye(3), np.zeros(3)
    assert all(np.log2(K[i, i]) % 1 == 0 for i in (0, 1)) and K[0, 2] % 1 == 0 and K[1, 2] % 1 == 0
    uvf, _ = oracle_lib.project(pts, K, R, t, integer=False)
    ties = uvf[:gc.TIE_COUNT]
    halves = np.array(gc.TIE_HALVES)
    assert list(halves) == [-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5]
    assert np.array_equal(ties[:7, 0], halves) and np.all(ties[:7, 1] == 1.25)       # ==, not close
    assert np.array_equal(ties[7:14, 1], halves) and np.all(ties[7:14, 0] == 1.25)
    assert np.array_equal(ties[14:, 0], np.repeat(halves, 7)) and np.array_equal(ties[14:, 1], np.tile(halves, 7))
    rest = uvf[gc.TIE_COUNT:]
    assert np.abs(np.abs(rest % 1.0 - 0.5)).min() > 1e-9, "the other points are no ties"
    assert np.all(np.abs(rest) >= 0.7), "and none of them rounds to row or column 0"
    even, _ = oracle_lib.project(pts, K, R, t, round_mode=oracle_lib.ROUND_HALF_EVEN)
    away, _ = oracle_lib.project(pts, K, R, t, round_mode=oracle_lib.ROUND_HALF_AWAY)
    assert np.array_equal(even[gc.TIE_COUNT:], away[gc.TIE_COUNT:])
    for axis in (0, 1):
        differ = even[:, axis] != away[:, axis]
        assert (differ & (uvf[:, axis] > 0)).any() and (differ & (uvf[:, axis] < 0)).any(), "positive and negative ties, where round and rint part ways in opposite directions"
        assert np.all(away[differ, axis] - even[differ, axis] == np.sign(uvf[differ, axis]))
    # the bounding box: the tie at -0.5 is inside under half-even (-0.0 >= 0) and outside under half-away
    box_even, box_away = gc.bbox_of(even, gc.TIE_W, gc.TIE_H), gc.bbox_of(away, gc.TIE_W, gc.TIE_H)
    assert box_even[0] == 0 and box_even[2] == 0 and box_away[0] == 1 and box_away[2] == 1 and box_even[4] != box_away[4]
    # mutation: points off the ties no longer split the modes
    off = pts[:gc.TIE_COUNT] + np.array([0.003, 0.003, 0.0])
    assert np.array_equal(oracle_lib.project(off, K, R, t, round_mode=0)[0], oracle_lib.project(off, K, R, t, round_mode=1)[0])


def test_icp_tie_case_pairs_depend_on_the_mode():
    c = gc.icp_tie_case()
    H, W = c["live_v"].shape[:2]
    assert (H, W) == (5, 7)
    args = (c["K"], c["live_v"], c["live_n"], c["model_v"], c["model_n"], c["model_pose"], c["est_pose"], c["dist_thresh"], c["cos_thresh"])
    # the projections are exact ties: su = 1 * (u / 1) + 0.5
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    V = c["live_v"].astype(np.float64)
    assert np.array_equal(1.0 * (V[..., 0] / V[..., 2]) + 0.5, u + 0.5) and np.array_equal(1.0 * (V[..., 1] / V[..., 2]) + 0.5, v + 0.5)
    masks = {}
    for mode in (tr.HALF_EVEN, tr.HALF_AWAY):
        terms, mask = tr.icp_terms(*args, round_mode=mode)
        sums, pairs = tr.icp_sums(terms)
        assert 0 < pairs == int(mask.sum()) < H * W and np.abs(sums).sum() > 0
        masks[mode] = mask
    assert not np.array_equal(masks[tr.HALF_EVEN], masks[tr.HALF_AWAY])
    assert not masks[tr.HALF_AWAY][-1].any() and not masks[tr.HALF_AWAY][:, -1].any(), "half-away leaves the image in the last row and column"
    # the distance gate is not what decides: every candidate is inside it
    for mode in (tr.HALF_EVEN, tr.HALF_AWAY):
        assert np.array_equal(tr.icp_terms(*args[:7], 100.0, args[8], round_mode=mode)[1], masks[mode])


@pytest.fixture(scope="module")
def unproject_oracle(oracle_lib):
    """size -> (case, oracle points, oracle colours), computed once."""
    out = {}
    for H, W in gc.UNPROJECT_SIZES:
        c = gc.unproject_case(H, W, seed=H * 1000 + W)
        out[(H, W)] = (c,) + oracle_lib.unproject(c["depth"], c["mask"], gc.kinv(c["K"]), c["R"], c["t"], rgb=c["rgb"])
    return out


@pytest.mark.parametrize("size", gc.UNPROJECT_SIZES)
def test_oracle_unproject_and_project_are_the_reference_formulas(oracle_lib, unproject_oracle, size):
    c, pts, col = unproject_oracle[size]
    want, want_col = gc.unproject_formula(c["depth"], c["mask"], c["K"], c["R"], c["t"], rgb=c["rgb"])
    assert len(pts) == len(want) == int((c["mask"] & (c["depth"] > 0)).sum()) > 0
    assert np.array_equal(col, want_col)
    rows = np.arange(len(pts)) if len(pts) <= 20000 else np.unique(np.concatenate([np.random.default_rng(3).integers(0, len(pts), 20000), [0, len(pts) - 1]]))
    np.testing.assert_allclose(pts[rows], want[rows], **F64_TOL)
    np.testing.assert_allclose(pts.sum(axis=0), want.sum(axis=0), rtol=1e-12)
    assert np.array_equal(pts[-1], oracle_lib.unproject(c["depth"], None, gc.kinv(c["K"]), c["R"], c["t"])[0][-1]), "mask = None keeps the (valid) last pixel"
    # back into another camera: pixels exact in both modes, float pixels and depth inside the float64 tolerance
    sample = pts[rows]
    R2, t2 = gc.rotation([0.1, 0.7, -0.2], 0.05) @ c["R"], c["t"] + np.array([[0.02], [-0.01], [0.03]])
    K64 = c["K"].astype(np.float64)
    for mode in (gc.HALF_EVEN, gc.HALF_AWAY):
        uv, dep = oracle_lib.project(sample, K64, R2, t2, round_mode=mode)
        w_uv, w_dep = gc.project_formula(sample, K64, R2, t2, round_mode=mode)
        uvf, _ = oracle_lib.project(sample, K64, R2, t2, integer=False)
        near_tie = np.abs(np.abs(uvf % 1.0) - 0.5).min(axis=1) < 1e-9  # (a random point is never one; a different last bit could flip it)
        assert np.array_equal(uv[~near_tie], w_uv[~near_tie]) and near_tie.sum() == 0
        np.testing.assert_allclose(dep, w_dep, **F64_TOL)
    np.testing.assert_allclose(uvf, gc.project_formula(sample, K64, R2, t2, integer=False)[0], rtol=1e-11, atol=1e-10)
    tie_even = oracle_lib.project(gc.tie_points(), gc.TIE_K, np.eye(3), np.zeros(3), round_mode=0)[0]
    tie_away = oracle_lib.project(gc.tie_points(), gc.TIE_K, np.eye(3), np.zeros(3), round_mode=1)[0]
    assert np.array_equal(tie_even, gc.project_formula(gc.tie_points(), gc.TIE_K, np.eye(3), np.zeros((3, 1)), round_mode=0)[0])
    assert np.array_equal(tie_away, gc.project_formula(gc.tie_points(), gc.TIE_K, np.eye(3), np.zeros((3, 1)), round_mode=1)[0])


def test_oracle_image2world_is_unproject_on_a_dense_grid(oracle_lib, unproject_oracle):
    """The oracle has no image2world of its own: with the scale factor folded into half-pixel coordinates, the formula on the valid pixels of a depth map
    is its unproject."""
    c, pts, _ = unproject_oracle[(37, 53)]
    valid = c["mask"] & (c["depth"] > 0)
    V, U = valid.nonzero()
    got = gc.image2world_formula(np.array([U, V]).T / 2.0, c["depth"][valid].astype(np.float64), c["K"], c["R"], c["t"], scale_factor=2.0)
    np.testing.assert_allclose(got, pts, **F64_TOL)


@pytest.mark.parametrize("size", gc.FRUSTUM_SIZES)
def test_oracle_view_frustum_is_the_reference_formula(oracle_lib, size):
    c = gc.frustum_case(*size)
    got = oracle_lib.view_frustum(c["depth"], c["K"], c["pose"])
    np.testing.assert_allclose(got, gc.view_frustum_formula(c["depth"], c["K"], c["pose"]), **F64_TOL)
    assert np.array_equal(got[:, 0], c["pose"][:3, 3]), "the apex is the camera centre"
    zeros = oracle_lib.view_frustum(np.zeros(size, np.float32), c["K"], c["pose"])
    assert np.array_equal(zeros, np.repeat(c["pose"][:3, 3:], 5, axis=1)), "an empty frame: five times the camera centre"
    lost = c["depth"].copy()
    lost[-1, -1] = 0.0
    assert not np.array_equal(oracle_lib.view_frustum(lost, c["K"], c["pose"]), got), "losing the last pixel changes the frustum"


def test_oracle_depth_quantize_is_the_reference_formula(oracle_lib):
    c = gc.quantize_case(*gc.QUANTIZE_SIZE)
    d = c["depth"]
    assert d.dtype == np.float32 and d.min() < -0.9 and d.max() > 69.0
    flat = d.reshape(-1)
    assert np.array_equal(flat[:len(gc.QUANTIZE_PLANTED)], np.array(gc.QUANTIZE_PLANTED, np.float32)) and np.signbit(flat[0]) and flat[-1] == 66.0
    on_boundary = np.isin(flat, (np.arange(-1000, 70001) / 1000.0).astype(np.float32))
    assert 0.45 < on_boundary.mean() < 0.6
    for mask in (None, c["mask"]):
        mm, m = oracle_lib.depth_quantize(d, mask=mask)
        w_mm, w_m = gc.depth_quantize_formula(d, mask=mask)
        assert np.array_equal(mm, w_mm) and np.array_equal(m.view(np.uint32), w_m.view(np.uint32))
    mm, m = oracle_lib.depth_quantize(d, mask=c["mask"])
    inside = (d * np.float32(1000.0) >= 0) & (d * np.float32(1000.0) <= 65535)
    assert np.array_equal(mm[inside], (d * np.float32(1000.0))[inside].astype(np.uint16)), "inside the range: the reference's astype, literally"
    assert list(mm.reshape(-1)[:9]) == [0, 0, 1, 9999, 10000, 10000, 65535, 65535, 65535]
    assert ((mm == 65535) & (d > 65.536)).any(), "saturated"
    assert ((d < 0) & (mm == 0)).any() and not (mm[d < 0]).any(), "negative depth is clamped to 0"
    assert ((mm > 0) & (m == 0) & ~c["mask"]).any() and ((m > 0) & (m <= 10.0)).any(), "zeroed by max_depth, and kept below it"
    assert (m[c["mask"]] == 0).all() and 0.1 < c["mask"].mean() < 0.3
