"""csrc/geometry.hip where its guards and branches actually run: ragged tiles and the long scan of the unprojection, the capacity contract, device memory,
both rounding modes (projection, bounding box, ICP association), the grid-stride loop of the frusta and the tail and saturation of the depth hand-off.
The cases and what each reaches: tests/geometry_cases.py, proven on the CPU by tests/test_geometry_cases_cpu.py.  Every comparison is against the CPU oracle
or the tracking restatement; float64 coordinates within rtol = atol = 1e-14, everything integral exactly."""
import ctypes

import numpy as np
import pytest

import geometry_cases as gc
import tracking_restatement as tr

pytestmark = pytest.mark.gpu
F64_TOL = dict(rtol=1e-14, atol=1e-14)  # test_geometry_gpu.py::test_full_resolution_checksums_and_oracle against the oracle
SENTINEL = -7777.25                     # fills every output before a call; the guard rows behind an output must still hold it afterwards
SENTINEL_U8, SENTINEL_I16 = 0xA5, 0x5A5A
GUARD_ROWS = 64


def _seed(size):
    return size[0] * 1000 + size[1]


@pytest.fixture(scope="module")
def unproject_oracle(oracle_lib):
    """size -> (case, oracle points, oracle colours); computed on first use, shared, never written to."""
    cache = {}

    def get(size):
        if size not in cache:
            c = gc.unproject_case(*size, seed=_seed(size))
            pts, col = oracle_lib.unproject(c["depth"], c["mask"], gc.kinv(c["K"]), c["R"], c["t"], rgb=c["rgb"])
            pts.setflags(write=False), col.setflags(write=False)
            cache[size] = (c, pts, col)
        return cache[size]
    return get


def _unproject_abi(ctx, c, mem, capacity, rows=None, with_mask=True, with_rgb=True):
    """hive_unproject straight through the C ABI.  Outputs of ``rows`` rows (None: NULL outputs), filled with the sentinel.
    -> (return code, n_out, xyz, rgba, last error)."""
    import torch
    from hive_amd._lib import MEM_DEVICE, ptr
    H, W = c["depth"].shape
    ins = [np.ascontiguousarray(c["depth"], np.float32), np.ascontiguousarray(c["mask"], np.uint8) if with_mask else None,
           np.ascontiguousarray(c["rgb"], np.uint8) if with_rgb else None]
    xyz = rgba = None
    if rows is not None:
        xyz = np.full((rows, 3), SENTINEL, np.float64)
        rgba = np.full((rows, 4), SENTINEL_U8, np.uint8) if with_rgb else None
    if mem == MEM_DEVICE:
        ins = [None if a is None else torch.from_numpy(a).cuda() for a in ins]
        xyz, rgba = (None if a is None else torch.from_numpy(a).cuda() for a in (xyz, rgba))
    n = ctypes.c_int64(-1)
    rc = ctx.lib.hive_unproject(ctx.handle, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), H, W, ptr(gc.kinv(c["K"])), ptr(np.ascontiguousarray(c["R"], np.float64)),
                                ptr(np.ascontiguousarray(c["t"], np.float64).reshape(3)), mem, ptr(xyz), ptr(rgba), capacity, ctypes.byref(n))
    message = (ctx.lib.hive_last_error(ctx.handle) or b"").decode()
    if mem == MEM_DEVICE:
        torch.cuda.synchronize()
        xyz, rgba = (None if a is None else a.cpu().numpy() for a in (xyz, rgba))
    return rc, int(n.value), xyz, rgba, message


def _is_sentinel(a):
    return bool(np.all(a == (SENTINEL if a.dtype == np.float64 else SENTINEL_U8)))


# ---- 1. the unprojection ladder ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", gc.UNPROJECT_SIZES)
def test_unprojection_ladder(gpu_ctx, oracle_lib, unproject_oracle, size):
    from hive_amd._lib import MEM_HOST, OK
    from hive_amd.geometric import point_cloud_from_depth, point_cloud_from_rgbd
    c, want, want_col = unproject_oracle(size)
    pts = point_cloud_from_depth(c["depth"], c["mask"], c["K"], c["R"], c["t"])
    assert pts.dtype == np.float64 and pts.shape == want.shape, (pts.shape, want.shape)  # the count: a lost ragged tail loses the (valid) last pixel
    np.testing.assert_allclose(pts, want, **F64_TOL)
    pts2, col = point_cloud_from_rgbd(c["rgb"], c["depth"], c["mask"], c["K"], c["R"], c["t"])
    assert pts2.shape == want.shape and col.dtype == np.uint8
    np.testing.assert_allclose(pts2, want, **F64_TOL)
    assert np.array_equal(col, want_col)
    # mask = NULL through the C ABI
    n_px = size[0] * size[1]
    all_pts, _ = oracle_lib.unproject(c["depth"], None, gc.kinv(c["K"]), c["R"], c["t"])
    rc, n, xyz, _, message = _unproject_abi(gpu_ctx, c, MEM_HOST, n_px, rows=n_px + GUARD_ROWS, with_mask=False, with_rgb=False)
    assert rc == OK, message
    assert n == len(all_pts) == int((c["depth"] > 0).sum()) >= len(want)
    np.testing.assert_allclose(xyz[:n], all_pts, **F64_TOL)
    assert _is_sentinel(xyz[n:])


# ---- 2. device memory and the capacity contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 53), (1025, 1025)])
def test_unproject_device_path_and_capacity(gpu_ctx, unproject_oracle, size):
    from hive_amd._lib import ERR_INVALID, MEM_DEVICE, MEM_HOST, OK
    c, want, want_col = unproject_oracle(size)
    total = len(want)
    rows = total + GUARD_ROWS
    rc, n, h_xyz, h_rgba, message = _unproject_abi(gpu_ctx, c, MEM_HOST, total, rows=rows)
    assert rc == OK and n == total, message
    np.testing.assert_allclose(h_xyz[:total], want, **F64_TOL)
    assert np.array_equal(h_rgba[:total], want_col) and _is_sentinel(h_xyz[total:]) and _is_sentinel(h_rgba[total:])
    # full capacity from and into device memory: the host call's bits (the one comparison of two GPU results here; the host call is checked above)
    rc, n, d_xyz, d_rgba, message = _unproject_abi(gpu_ctx, c, MEM_DEVICE, total, rows=rows)
    assert rc == OK and n == total, message
    assert np.array_equal(d_xyz[:total].view(np.uint64), h_xyz[:total].view(np.uint64)) and np.array_equal(d_rgba[:total], h_rgba[:total])
    assert _is_sentinel(d_xyz[total:]) and _is_sentinel(d_rgba[total:]), "the guard rows behind the last point"
    # capacity 0 and no outputs: a count query
    rc, n, _, _, message = _unproject_abi(gpu_ctx, c, MEM_DEVICE, 0, rows=None, with_rgb=False)
    assert rc == OK and n == total, message
    # five rows short: refused, the true total reported, the first `capacity` rows written and nothing behind them
    capacity = total - 5
    rc, n, d_xyz, d_rgba, message = _unproject_abi(gpu_ctx, c, MEM_DEVICE, capacity, rows=rows)
    assert rc == ERR_INVALID and n == total
    assert str(total) in message and str(capacity) in message, message
    np.testing.assert_allclose(d_xyz[:capacity], want[:capacity], **F64_TOL)
    assert np.array_equal(d_rgba[:capacity], want_col[:capacity])
    assert _is_sentinel(d_xyz[capacity:]) and _is_sentinel(d_rgba[capacity:])
    # and the context goes on working
    rc, n, d_xyz, _, message = _unproject_abi(gpu_ctx, c, MEM_DEVICE, total, rows=rows, with_rgb=False)
    assert rc == OK and n == total, message
    np.testing.assert_allclose(d_xyz[:total], want, **F64_TOL)


# ---- 3. + 4. projection and its bounding box in both rounding modes ---------------------------------------------------------------------------------------
def _project_abi(ctx, pts, mem, integer, scale=1.0):
    import torch
    from hive_amd._lib import MEM_DEVICE, ptr
    n = len(pts)
    K, R, t = np.ascontiguousarray(gc.TIE_K), np.eye(3), np.zeros(3)
    uv = np.full((n, 2), -77, np.int32) if integer else np.full((n, 2), SENTINEL, np.float64)
    dep = np.full(n, SENTINEL, np.float64)
    pts = np.ascontiguousarray(pts, np.float64)
    if mem == MEM_DEVICE:
        pts, uv, dep = (torch.from_numpy(a).cuda() for a in (pts, uv, dep))
    ctx.check(ctx.lib.hive_project(ctx.handle, ptr(pts), n, ptr(K), ptr(R), ptr(t), float(scale), mem, ptr(uv) if integer else None,
                                   None if integer else ptr(uv), ptr(dep)))
    if mem == MEM_DEVICE:
        torch.cuda.synchronize()
        uv, dep = uv.cpu().numpy(), dep.cpu().numpy()
    return uv, dep


def _bbox_abi(ctx, pts, mem):
    import torch
    from hive_amd._lib import MEM_DEVICE, ptr
    pts = np.ascontiguousarray(pts, np.float64)
    if mem == MEM_DEVICE:
        pts = torch.from_numpy(pts).cuda()
    box = np.zeros(5, np.int32)
    ctx.check(ctx.lib.hive_project_bbox(ctx.handle, ptr(pts), len(pts), ptr(np.ascontiguousarray(gc.TIE_K)), ptr(np.eye(3)), ptr(np.zeros(3)), gc.TIE_W, gc.TIE_H,
                                        mem, ptr(box)))
    return [int(v) for v in box]


@pytest.fixture(scope="module")
def tie_oracle(oracle_lib):
    """mode -> (int32 pixels, depth) of the oracle on the tie points, and "f64" -> its unrounded pixels."""
    pts = gc.tie_points()
    out = {mode: oracle_lib.project(pts, gc.TIE_K, np.eye(3), np.zeros(3), round_mode=mode) for mode in (gc.HALF_EVEN, gc.HALF_AWAY)}
    out["f64"] = oracle_lib.project(pts, gc.TIE_K, np.eye(3), np.zeros(3), integer=False)[0]
    return pts, out


def test_projection_in_both_rounding_modes(tie_oracle):
    """A context of its own: the session's shared one keeps its mode."""
    from hive_amd import _lib
    pts, want = tie_oracle
    assert len(pts) % 256 != 0 and len(pts) > 256
    ctx = _lib.Context(0)
    got = {}
    try:
        for mode, set_it in ((gc.HALF_EVEN, False), (gc.HALF_AWAY, True), (gc.HALF_EVEN, True)):  # the default, then set, then set back
            if set_it:
                ctx.set_round_mode(_lib.ROUND_HALF_AWAY if mode == gc.HALF_AWAY else _lib.ROUND_HALF_EVEN)
            for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
                uv, dep = _project_abi(ctx, pts, mem, integer=True)
                assert uv.dtype == np.int32 and np.array_equal(uv, want[mode][0]), (mode, mem, np.flatnonzero((uv != want[mode][0]).any(axis=1)))
                np.testing.assert_allclose(dep, want[mode][1], **F64_TOL)
                uv1, dep1 = _project_abi(ctx, pts[2:3], mem, integer=True)  # n = 1: the tie at u = -0.5
                assert np.array_equal(uv1, want[mode][0][2:3]) and dep1[0] == want[mode][1][2]
                uvf, depf = _project_abi(ctx, pts, mem, integer=False)
                np.testing.assert_allclose(uvf, want["f64"], rtol=1e-11, atol=1e-10)  # test_world2image_matches_reference's
                np.testing.assert_allclose(depf, want[mode][1], **F64_TOL)
                got[(mode, mem)] = uv
    finally:
        ctx.close()
    assert not np.array_equal(got[(gc.HALF_EVEN, _lib.MEM_HOST)], got[(gc.HALF_AWAY, _lib.MEM_HOST)])
    assert not np.array_equal(got[(gc.HALF_EVEN, _lib.MEM_DEVICE)], got[(gc.HALF_AWAY, _lib.MEM_DEVICE)])


def test_bounding_box_follows_the_contexts_rounding(tie_oracle):
    """hive_project_bbox is the box of hive_project's pixels in either mode.  The tie at u = -0.5 (v = -0.5) rounds to -0.0 under half-even, inside the image,
    and to -1 under half-away, outside: count and minima differ.  (A kernel that always rounds half-to-even returns the half-even box in both modes.)"""
    from hive_amd import _lib
    pts, want = tie_oracle
    boxes = {}
    ctx = _lib.Context(0)
    try:
        for mode in (gc.HALF_EVEN, gc.HALF_AWAY):
            if mode == gc.HALF_AWAY:
                ctx.set_round_mode(_lib.ROUND_HALF_AWAY)
            expect = gc.bbox_of(want[mode][0], gc.TIE_W, gc.TIE_H)
            for mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
                assert _bbox_abi(ctx, pts, mem) == expect, (mode, mem)
                assert _bbox_abi(ctx, pts[:gc.TIE_COUNT], mem) == gc.bbox_of(want[mode][0][:gc.TIE_COUNT], gc.TIE_W, gc.TIE_H), (mode, mem, "ties alone")
            boxes[mode] = expect
    finally:
        ctx.close()
    even, away = boxes[gc.HALF_EVEN], boxes[gc.HALF_AWAY]
    assert even[0] == 0 and even[2] == 0 and away[0] == 1 and away[2] == 1 and even[4] != away[4], (even, away)


# ---- 5. image2world from device memory ----------------------------------------------------------------------------------------------------------------------
def _image2world_abi(ctx, uv, depth, c, scale, mem):
    import torch
    from hive_amd._lib import MEM_DEVICE, ptr
    n = len(uv)
    uv, depth = np.ascontiguousarray(uv, np.float64), np.ascontiguousarray(depth, np.float64)
    out = np.full((n + GUARD_ROWS, 3), SENTINEL, np.float64)
    if mem == MEM_DEVICE:
        uv, depth, out = (torch.from_numpy(a).cuda() for a in (uv, depth, out))
    ctx.check(ctx.lib.hive_image2world(ctx.handle, ptr(uv), ptr(depth), n, ptr(gc.kinv(c["K"])), ptr(np.ascontiguousarray(c["R"], np.float64)),
                                       ptr(np.ascontiguousarray(c["t"], np.float64).reshape(3)), float(scale), mem, ptr(out)))
    if mem == MEM_DEVICE:
        torch.cuda.synchronize()
        out = out.cpu().numpy()
    assert _is_sentinel(out[n:])
    return out[:n]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_image2world_from_device_memory(gpu_ctx, unproject_oracle, n):
    from hive_amd._lib import MEM_DEVICE, MEM_HOST
    c, want, _ = unproject_oracle((37, 53))
    # the first n valid pixels at half their coordinates and scale factor 2: the arithmetic of the unprojection, so the oracle's rows
    V, U = (c["mask"] & (c["depth"] > 0)).nonzero()
    uv, depth = np.array([U, V]).T[:n] / 2.0, c["depth"][V[:n], U[:n]].astype(np.float64)
    host = _image2world_abi(gpu_ctx, uv, depth, c, 2.0, MEM_HOST)
    dev = _image2world_abi(gpu_ctx, uv, depth, c, 2.0, MEM_DEVICE)
    np.testing.assert_allclose(host, want[:n], **F64_TOL)
    np.testing.assert_allclose(host, gc.image2world_formula(uv, depth, c["K"], c["R"], c["t"], 2.0), **F64_TOL)
    assert np.array_equal(dev.view(np.uint64), host.view(np.uint64)), "device memory: the host path's bits (host path checked against the oracle above)"
    # pixel coordinates off the grid, float64 depth: the reference's formula
    rng = np.random.default_rng(n)
    uv, depth = rng.uniform(-3.0, 30.0, (n, 2)), rng.uniform(0.5, 5.0, n)
    formula = gc.image2world_formula(uv, depth, c["K"], c["R"], c["t"], 2.0)
    host = _image2world_abi(gpu_ctx, uv, depth, c, 2.0, MEM_HOST)
    dev = _image2world_abi(gpu_ctx, uv, depth, c, 2.0, MEM_DEVICE)
    np.testing.assert_allclose(host, formula, **F64_TOL)
    assert np.array_equal(dev.view(np.uint64), host.view(np.uint64))


# ---- 6. frusta ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", gc.FRUSTUM_SIZES)
def test_frusta_ragged_wave_and_grid_stride(gpu_ctx, oracle_lib, size):
    import torch
    from hive_amd.fusion import get_view_frustum, view_frusta
    c = gc.frustum_case(*size)
    want = oracle_lib.view_frustum(c["depth"], c["K"], c["pose"])
    assert not np.array_equal(want, oracle_lib.view_frustum(np.where(c["depth"] == c["depth"].max(), 0, c["depth"]), c["K"], c["pose"]))  # the last pixel decides
    got = get_view_frustum(c["depth"], c["K"], c["pose"], ctx=gpu_ctx)
    assert got.shape == (3, 5) and np.array_equal(got, want)
    assert np.array_equal(get_view_frustum(torch.from_numpy(c["depth"]).cuda(), c["K"], c["pose"], ctx=gpu_ctx), want)
    # three frames: the case, an empty frame (a maximum that leaks across frames shows in it), the case at half its depth
    depths = np.stack([c["depth"], np.zeros_like(c["depth"]), c["depth"] * np.float32(0.5)])
    poses = np.stack([c["pose"], np.eye(4), c["pose"]])
    poses[2, :3, 3] += [0.25, 0.5, -0.125]
    want3 = np.stack([oracle_lib.view_frustum(depths[i], c["K"], poses[i]) for i in range(3)])
    assert np.array_equal(want3[1], np.zeros((3, 5))) and not np.array_equal(want3[0], want3[2])
    assert np.array_equal(view_frusta(depths, c["K"], poses, ctx=gpu_ctx), want3)
    assert np.array_equal(view_frusta(torch.from_numpy(depths).cuda(), c["K"], poses, ctx=gpu_ctx), want3)


# ---- 7. the depth hand-off ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
def test_depth_hand_off_tail_saturation_and_argument_forms(gpu_ctx, oracle_lib, dtype_name):
    import torch
    from hive_amd import _lib
    H, W = gc.QUANTIZE_SIZE
    n, pad = H * W, 256
    c = gc.quantize_case(H, W)
    dtype, code = {"float32": (torch.float32, _lib.F32), "float16": (torch.float16, _lib.F16), "bfloat16": (torch.bfloat16, _lib.BF16)}[dtype_name]
    dd = torch.from_numpy(c["depth"]).cuda().to(dtype)
    as_f32 = dd.float().cpu().numpy()  # the values the kernel sees, after the conversion to the type
    mk = torch.from_numpy(c["mask"].astype(np.uint8)).cuda()
    for mask in (None, c["mask"]):
        e_mm, e_m = oracle_lib.depth_quantize(as_f32, mask=mask)
        # the case has what it is for, in this type too
        assert (e_mm == 65535).sum() > 10 and ((as_f32 < 0) & (e_mm == 0)).sum() > 5, "saturated; negative depth clamped to 0"
        unmasked = np.ones((H, W), bool) if mask is None else ~mask
        assert ((e_mm > 0) & (e_m == 0) & unmasked).any() and ((e_m > 0) & (e_m <= 10.0)).any(), "zeroed by max_depth; kept below it"
        for want_mm, want_m in ((True, True), (True, False), (False, True)):
            mm = torch.full((n + pad,), SENTINEL_I16, dtype=torch.int16, device="cuda")
            m = torch.full((n + pad,), SENTINEL, dtype=torch.float32, device="cuda")
            gpu_ctx.check(gpu_ctx.lib.hive_depth_quantize(gpu_ctx.handle, dd.data_ptr(), code, H, W, 1.0 / 1000.0, 10.0, None if mask is None else mk.data_ptr(),
                                                          mm.data_ptr() if want_mm else None, m.data_ptr() if want_m else None))
            torch.cuda.synchronize()
            mm, m = mm.cpu().numpy(), m.cpu().numpy()
            form = (dtype_name, mask is not None, want_mm, want_m)
            if want_mm:
                assert np.array_equal(mm[:n].view(np.uint16).reshape(H, W), e_mm), form
            if want_m:
                assert np.array_equal(m[:n].view(np.uint32).reshape(H, W), e_m.view(np.uint32)), form
            assert np.all(mm[n if want_mm else 0:] == SENTINEL_I16) and np.all(m[n if want_m else 0:] == np.float32(SENTINEL)), form  # the guard, and an output not asked for


# ---- 8. ICP association in both rounding modes ----------------------------------------------------------------------------------------------------------------
def test_icp_association_follows_the_contexts_rounding():
    import torch
    from hive_amd import _lib, tracking
    c = gc.icp_tie_case()
    H, W = c["live_v"].shape[:2]
    dev = [torch.from_numpy(c[k]).cuda() for k in ("live_v", "live_n", "model_v", "model_n")]
    masks = {}
    for mode, lib_mode in ((tr.HALF_EVEN, _lib.ROUND_HALF_EVEN), (tr.HALF_AWAY, _lib.ROUND_HALF_AWAY)):
        terms, mask = tr.icp_terms(c["K"], c["live_v"], c["live_n"], c["model_v"], c["model_n"], c["model_pose"], c["est_pose"], c["dist_thresh"], c["cos_thresh"],
                                   round_mode=mode)
        want, want_pairs = tr.icp_sums(terms)
        ctx = _lib.Context(0)
        try:
            if mode == tr.HALF_AWAY:
                ctx.set_round_mode(lib_mode)
            got_mask = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
            got, pairs = tracking.icp_step(ctx, c["K"], *dev, c["model_pose"], c["est_pose"], c["dist_thresh"], c["cos_thresh"], pair_mask=got_mask)
            torch.cuda.synchronize()
        finally:
            ctx.close()
        masks[mode] = got_mask.cpu().numpy()
        assert np.array_equal(masks[mode], mask.astype(np.uint8)), mode
        assert 0 < pairs == want_pairs == int(mask.sum()) < H * W
        bound = terms.shape[0] * 2.0 ** -52 * np.abs(terms[:, :28]).sum(axis=0)  # test_icp_step_sums_and_pairs': n 2^-52 sum |term|
        assert np.all(np.abs(got - want) <= bound) and np.abs(want).sum() > 0
    assert not np.array_equal(masks[tr.HALF_EVEN], masks[tr.HALF_AWAY])
