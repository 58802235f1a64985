"""Billboards on the GPU (csrc/billboard.hip hive_fg_billboard, foreground.billboard, the ``billboard`` keyword of frame_mesh / process_frame) against numpy:
the exact median, the map in its stated operation order (bit for bit) and in the reference's literal matrix form (within rounding), the frame path against
the separate calls, and the default path against itself."""
import numpy as np
import pytest

import fts_restatement as F

pytestmark = pytest.mark.gpu


def gpu_median(ctx, values):
    """The median kernel alone: with R = I and t = 0 the camera-space depth of (0, 0, z) is z itself."""
    from hive_amd import foreground
    vertices = np.zeros((len(values), 3), np.float64)
    vertices[:, 2] = values
    _, median = foreground.billboard(vertices, np.eye(3), np.zeros((3, 1)), ctx=ctx, return_median=True)
    return np.float64(median)


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


SIZES = sorted(set(list(range(1, 71)) + [2 ** k + d for k in range(7, 12) for d in (-1, 0, 1)]))


def _value_families(n, rng):
    tiny = np.float64(5e-324)
    yield "normal", rng.standard_normal(n) * 3.0 + 2.5
    yield "all equal", np.full(n, 1.2345678901234567)
    yield "two values", rng.choice([0.75, 3.5], size=n)
    yield "negative", -np.abs(rng.standard_normal(n)) - 0.5
    yield "mixed sign, wide range", rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, size=n)
    yield "denormals", rng.integers(-1000, 1000, size=n).astype(np.float64) * tiny + tiny
    ties = rng.standard_normal(n)
    ties[rng.permutation(n)[: max(1, (2 * n) // 3)]] = 0.5  # two thirds of the values tie at what becomes the middle
    yield "ties at the middle", ties


def test_median_is_numpys_bit_for_bit(gpu_ctx):
    """Every V up to 70, powers of two +- 1 up to 2049, odd and even; value families without a mixed pair of zeros: the same bits as np.median."""
    rng = np.random.default_rng(2024)
    checked = 0
    for n in SIZES:
        for name, values in _value_families(n, rng):
            values = np.ascontiguousarray(values, np.float64)
            assert not (np.any(np.signbit(values) & (values == 0)) and np.any(~np.signbit(values) & (values == 0)))
            got, want = gpu_median(gpu_ctx, values), np.median(values)
            assert same_bits(got, want), (n, name, float(got), float(want))
            checked += 1
    assert checked == len(SIZES) * 7


@pytest.mark.parametrize("n", [307_200, 2_073_600, 2_073_601])
def test_median_at_frame_sizes(gpu_ctx, n):
    """V = H W at VGA and 1080p (many workgroups share the histogram), and an odd neighbour; twice, for determinism."""
    rng = np.random.default_rng(n)
    for values in (rng.standard_normal(n) + 2.0, np.round(rng.standard_normal(n), 2), -rng.random(n)):
        want = np.median(values)
        assert same_bits(gpu_median(gpu_ctx, values), want) and same_bits(gpu_median(gpu_ctx, values), want)


def test_median_with_both_zeros_is_compared_by_value(gpu_ctx):
    """numpy's partition does not order -0 and +0, the integer keys do (-0 first): such arrays agree by value, not necessarily by sign bit."""
    for n in (2, 3, 8, 9, 64, 129):
        values = np.zeros(n)
        values[::2] = -0.0
        assert gpu_median(gpu_ctx, values) == np.median(values) == 0.0
        values[0], values[-1] = -1.0, 1.0
        assert gpu_median(gpu_ctx, values) == np.median(values)


def _poses():
    from scipy.spatial.transform import Rotation
    yield "identity", np.eye(3), np.zeros((3, 1))
    yield "identity, t != 0", np.eye(3), np.array([[0.3], [-1.2], [2.0]])
    yield "general", Rotation.from_euler("xyz", [0.31, -0.52, 1.1]).as_matrix(), np.array([[-2.56], [1.7], [0.45]])
    yield "looking backwards", Rotation.from_euler("y", 2.9).as_matrix(), np.array([[0.5], [0.25], [-4.0]])  # negative depths through the quirk


@pytest.mark.parametrize("n", [1, 2, 9, 1000, 76_801])
def test_billboard_equals_ordered_restatement_bit_for_bit(gpu_ctx, n):
    """foreground.billboard == the numpy restatement in the stated operation order, every coordinate bit for bit, numpy arrays and device tensors (in place);
    and == the reference's literal `R @ (...)` lines within 16 * 2^-53 * M, M = max_i |p_i + t| + |t|: BLAS may fuse and reorder the 3-term dot products, each
    is then off by at most 3 * 2^-53 * sqrt(3) * M ~ 5.2 * 2^-53 * M, the forward error passes through the back rotation once and the back product and the
    subtraction add theirs, about 12 * 2^-53 * M in all."""
    import torch
    from hive_amd import foreground
    rng = np.random.default_rng(n)
    vertices = rng.standard_normal((n, 3)) * [1.5, 1.0, 0.8] + [0.2, -0.1, 3.0]
    for name, R, t in _poses():
        want, want_m = F.billboard_ordered(vertices, R, t)
        got, got_m = foreground.billboard(vertices, R, t, ctx=gpu_ctx, return_median=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert same_bits(got_m, want_m), name
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        dev = torch.from_numpy(vertices.copy()).cuda()
        out = foreground.billboard(dev, R, t, ctx=gpu_ctx)
        assert out.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy().view(np.uint64), want.view(np.uint64)), name
        literal = F.billboard_literal(vertices, R, t)
        bound = F.literal_bound(vertices, t)
        worst = np.abs(got - literal).max()
        print(f"V = {n}, {name}: |kernel - literal| = {worst:.3g}, bound {bound:.3g}")
        assert worst <= bound, name
        # flat: ONE restated camera-space depth for all vertices, up to the rounding of the way back and forth (it is the median itself only where R t = t:
        # R (R^T (c - t) + t) = c - t + R t)
        z = F.camera_z_ordered(got, R, t.reshape(3))
        assert np.abs(z - np.median(z)).max() <= bound


def test_billboard_is_not_the_inverse_of_world2image_for_nonzero_translation(gpu_ctx):
    """The quirk is kept: R (p + t), not R p + t -- an object whose vertices already share one depth under world2image's camera still moves when t != 0 and R != I."""
    from hive_amd import foreground
    _, R, t = list(_poses())[2]
    cam = np.random.default_rng(5).standard_normal((50, 3))
    cam[:, 2] = 2.0  # flat in the camera of world2image: c = R p + t
    world = (R.T @ (cam.T - t)).T
    got = foreground.billboard(world, R, t, ctx=gpu_ctx)
    assert np.abs(got - world).max() > 1e-3
    assert np.array_equal(got, F.billboard_ordered(world, R, t)[0])


def test_billboard_without_vertices_is_a_no_op(gpu_ctx):
    import torch
    from hive_amd import foreground
    out, median = foreground.billboard(np.zeros((0, 3)), np.eye(3), np.zeros((3, 1)), ctx=gpu_ctx, return_median=True)
    assert out.shape == (0, 3) and median == 0.0
    dev = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    assert foreground.billboard(dev, np.eye(3), np.zeros((3, 1)), ctx=gpu_ctx).shape == (0, 3)


def _object_frame(h=240, w=320):
    """One frame of the synthetic room with three ellipse objects and a camera whose rotation is a few degrees off the identity with t != 0 -- the billboard's
    quirk then shifts every object by |t - R^T t|, a few centimetres: enough to differ from the proper inverse, small enough to stay in the image."""
    from scipy.spatial.transform import Rotation
    from hive_amd import synthetic
    seq = synthetic.make_sequence(num_frames=1, height=h, width=w, yaw_step_deg=2.4)
    masks = synthetic.ellipse_masks(1, h, w, num_objects=3, seed=3)[0]
    R = Rotation.from_euler("xyz", [0.01, 0.03, -0.02]).as_matrix()
    t = np.array([[-0.8], [0.3], [0.5]])
    return seq, masks, R, t


def _projected_box(vertices, K, R, t):
    """Bounding box of the rounded pixel coordinates of K (R p + t) on the CPU (world2image's map)."""
    cam = np.asarray(K, np.float64) @ (R @ vertices.T + t)
    uv = np.round(cam[:2] / cam[2])
    return uv[0].min(), uv[1].min(), uv[0].max(), uv[1].max()


@pytest.mark.parametrize("decimate", [False, True])
@pytest.mark.parametrize("enable_cc", [False, True])
def test_frame_mesh_with_billboard_equals_separate_steps(gpu_ctx, enable_cc, decimate):
    """frame_mesh(billboard=True) == the call without it, then foreground.billboard, then get_mesh_texture_and_uv on the result: vertices, faces, uv, bbox and
    texture bit for bit, with and without the clean-up and the decimation.  The inputs are chosen so that every flattened object projects inside the image
    (checked here on the CPU), where the reference's texture step works too."""
    import torch
    from hive_amd import foreground
    from hive_amd.options import MeshDecimationOptions
    seq, masks, R, t = _object_frame()
    K, rgb = seq["K"], seq["color"][0]
    h, w = masks.shape
    depth, img = torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(rgb).cuda()
    dec = MeshDecimationOptions(num_faces_object=500) if decimate else None
    seen = 0
    for object_id in range(1, int(masks.max()) + 1):
        mask = torch.from_numpy(masks == object_id).cuda()
        plain = foreground.frame_mesh(depth, mask, img, K, R, t, ctx=gpu_ctx, enable_cc_analysis=enable_cc, decimation_options=dec)
        pv, pf = plain["vertices"].clone(), plain["faces"].clone()
        if pv.shape[0] == 0:
            continue
        seen += 1
        flat = foreground.billboard(pv.clone(), R, t, ctx=gpu_ctx).cpu().numpy()
        lo_u, lo_v, hi_u, hi_v = _projected_box(flat, K, R, t)
        assert 0 <= lo_u and 0 <= lo_v and hi_u < w and hi_v < h, "pick inputs whose flattened box stays inside the image"
        tex, uv, bbox = foreground.get_mesh_texture_and_uv(flat, rgb, K, R, t, ctx=gpu_ctx, return_bbox=True)
        got = foreground.frame_mesh(depth, mask, img, K, R, t, ctx=gpu_ctx, enable_cc_analysis=enable_cc, decimation_options=dec, billboard=True)
        assert np.array_equal(got["vertices"].cpu().numpy().view(np.uint64), flat.view(np.uint64))
        assert torch.equal(got["faces"], pf)
        assert np.array_equal(got["uv"].cpu().numpy(), uv) and got["bbox"] == bbox and np.array_equal(got["texture"].cpu().numpy(), tex)
        assert not np.array_equal(flat, pv.cpu().numpy()), "the object was not flat before"
        # all flattened vertices share one restated camera-space depth (up to the rounding of the way back: tests above)
        z = F.camera_z_ordered(flat, R, t.reshape(3))
        assert np.abs(z - np.median(z)).max() <= F.literal_bound(flat, t)
        for key in ("before", "decimated", "decimation_stats"):
            assert got.get(key) == plain.get(key)
    assert seen == 3


@pytest.mark.parametrize("decimate", [False, True])
@pytest.mark.parametrize("enable_cc", [False, True])
def test_process_frame_with_billboard_equals_separate_steps(gpu_ctx, enable_cc, decimate):
    """process_frame(billboard=True) == per object: frame_mesh without it, foreground.billboard, get_mesh_texture_and_uv; stacked and packed as process_frame does."""
    import torch
    from hive_amd import foreground
    from hive_amd.options import MaskDilationOptions, MeshDecimationOptions, MeshFilteringOptions
    from test_fgmesh_gpu import _reference_pack_textures
    seq, masks, R, t = _object_frame()
    K, rgb, depth = seq["K"], seq["color"][0], seq["depth"][0]
    ids = masks.copy()
    ids[depth == 0] = 0
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3:4] = R, t
    dil, flt = MaskDilationOptions(num_iterations=0), MeshFilteringOptions()
    dec = MeshDecimationOptions(num_faces_object=500) if decimate else None
    d, img = torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda()
    verts, faces, texs, uvs, count = [], [], [], [], 0
    for object_id in range(1, int(ids.max()) + 1):
        mask = torch.from_numpy(ids == object_id).cuda()
        plain = foreground.frame_mesh(d, mask, img, K, R, t, flt, ctx=gpu_ctx, enable_cc_analysis=enable_cc, min_components=flt.min_num_components,
                                      decimation_options=dec)
        f = plain["faces"].cpu().numpy().astype(np.int64)
        flat = foreground.billboard(plain["vertices"].clone(), R, t, ctx=gpu_ctx).cpu().numpy()
        tex, uv = foreground.get_mesh_texture_and_uv(flat, rgb, K, R, t, ctx=gpu_ctx)
        verts.append(flat), faces.append(f + count), texs.append(tex), uvs.append(uv)
        count += len(flat)
    want_atlas, want_uv = _reference_pack_textures(texs, uvs)
    got = foreground.process_frame(img, d, torch.from_numpy(ids).cuda(), K, pose, dil, flt, ctx=gpu_ctx, enable_cc_analysis=enable_cc, decimation_options=dec,
                                   billboard=True)
    assert got["objects"] == [1, 2, 3]
    assert np.array_equal(got["vertices"].cpu().numpy().view(np.uint64), np.vstack(verts).view(np.uint64))
    assert np.array_equal(got["faces"].cpu().numpy(), np.vstack(faces))
    assert np.array_equal(got["texture"].cpu().numpy(), want_atlas) and np.array_equal(got["uv"].cpu().numpy(), want_uv)


def test_billboard_off_is_todays_output(gpu_ctx):
    """billboard=False == the call that omits the keyword, bit for bit: frame_mesh and process_frame, with the clean-up and the decimation too."""
    import torch
    from hive_amd import foreground
    from hive_amd.options import MaskDilationOptions, MeshDecimationOptions, MeshFilteringOptions
    seq, masks, R, t = _object_frame()
    K, rgb = seq["K"], seq["color"][0]
    depth, img = torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(rgb).cuda()
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3:4] = R, t
    for kwargs in ({}, {"enable_cc_analysis": True}, {"enable_cc_analysis": True, "decimation_options": MeshDecimationOptions(num_faces_object=500)}):
        mask = torch.from_numpy(masks == 1).cuda()
        a = foreground.frame_mesh(depth, mask, img, K, R, t, ctx=gpu_ctx, **kwargs)
        a = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in a.items()}
        b = foreground.frame_mesh(depth, mask, img, K, R, t, ctx=gpu_ctx, billboard=False, **kwargs)
        assert a.keys() == b.keys()
        for key in a:
            assert torch.equal(a[key], b[key]) if hasattr(a[key], "shape") else a[key] == b[key], key
        ids = torch.from_numpy(masks).cuda()
        dil, flt = MaskDilationOptions(num_iterations=0), MeshFilteringOptions()
        pa = foreground.process_frame(img, depth, ids, K, pose, dil, flt, ctx=gpu_ctx, **kwargs)
        pb = foreground.process_frame(img, depth, ids, K, pose, dil, flt, ctx=gpu_ctx, billboard=False, **kwargs)
        assert pa.keys() == pb.keys()
        for key in pa:
            assert torch.equal(pa[key], pb[key]) if hasattr(pa[key], "shape") else pa[key] == pb[key], key


def test_object_at_the_image_border_does_not_raise(gpu_ctx):
    """Flattened vertices may project outside the frame (the reference's TODO at this spot, where its texture step breaks): here the crop is clamped to the
    image.  Nothing raises and the shapes are consistent."""
    import torch
    from scipy.spatial.transform import Rotation
    from hive_amd import foreground, synthetic
    h, w = 240, 320
    seq = synthetic.make_sequence(num_frames=1, height=h, width=w, yaw_step_deg=2.4)
    mask = np.zeros((h, w), bool)
    mask[:60, :80] = True  # the top left corner
    R = Rotation.from_euler("xyz", [0.02, 0.06, -0.02]).as_matrix()
    t = np.array([[-1.5], [0.8], [0.5]])
    got = foreground.frame_mesh(torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(seq["color"][0]).cuda(), seq["K"], R, t,
                                ctx=gpu_ctx, enable_cc_analysis=True, billboard=True)
    nv = got["vertices"].shape[0]
    assert nv > 1000 and got["uv"].shape == (nv, 2) and got["faces"].shape[1] == 3 and int(got["faces"].max()) < nv
    min_u, min_v, max_u, max_v = got["bbox"]
    assert min_u <= max_u and min_v <= max_v
    tex = got["texture"]
    assert tex.dim() == 3 and tex.shape[2] == 3
    assert tex.shape[0] == max(0, min(max_v, h) - max(min_v, 0)) and tex.shape[1] == max(0, min(max_u, w) - max(min_u, 0))
