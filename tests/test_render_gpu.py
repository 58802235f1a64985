"""The rasteriser on the GPU (csrc/render.hip behind hive_amd.render.render_mesh) against the numpy restatement of its rules (tests/render_restatement.py) and
against known answers: every comparison is exact -- winning face, depth bits, colour."""
import numpy as np
import pytest

import render_cases as C
import render_restatement as RR

pytestmark = pytest.mark.gpu


def _as_dict(mesh):
    if mesh is None or isinstance(mesh, dict):
        return mesh
    return {"vertices": mesh.vertices, "faces": mesh.faces, "vertex_colors": mesh.visual.vertex_colors}


def _host(mesh):
    """A process_frame dict on the host."""
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in mesh.items()}


def _gpu(meshes, K, pose, H, W, **kw):
    from hive_amd.render import render_mesh
    out = render_mesh(K, pose, *meshes, size=(H, W), return_depth=True, return_faces=True, **kw)
    return tuple(x.cpu().numpy() for x in out)


def _same(got, want):
    assert np.array_equal(got[2], want[2]), f"winning faces differ at {int((got[2] != want[2]).sum())} pixels"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "depth bits differ"
    assert np.array_equal(got[0], want[0]), f"colours differ at {int((got[0] != want[0]).any(-1).sum())} pixels"


def _check(meshes, K, pose, H, W, **kw):
    """render_mesh == the restatement; returns the restatement's (colour, depth, face, cover)."""
    want = RR.render([_as_dict(m) for m in meshes], K, pose[:3, :3], pose[:3, 3], H, W, **kw)
    _same(_gpu(meshes, K, pose, H, W, **kw), want)
    return want


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (24, 32), (47, 63), (48, 64)])
def test_screen_size_ladder(gpu_ctx, H, W):
    """The CPU known answers at every size (wave tails of the pixel and the vertex kernels): grid round trip at two poses, quad and reversed winding, fan, ties."""
    for pose in (C.IDENTITY, C.general_pose()):
        s = C.grid_scene(H, W, pose=pose)
        for name in ("textured", "coloured") if pose is C.IDENTITY else ("textured",):
            color, depth, face, cover = _check([s[name]], s["K"], pose, H, W)
            block = np.zeros((H, W), bool)
            block[:H - 1, :W - 1] = True
            assert np.array_equal(cover, block.astype(np.int32))
            assert np.array_equal(depth[block].view(np.uint32), s["depth"][block].view(np.uint32)) and np.array_equal(color[block], s["image"][block])
    K, quad = C.quad_scene(H, W)
    _, depth, _, cover = _check([quad], K, C.IDENTITY, H, W)
    assert (cover == 1).all() and (depth.view(np.uint32) == np.float32(2.0).view(np.uint32)).all()
    _check([dict(quad, faces=np.ascontiguousarray(quad["faces"][:, ::-1]))], K, C.IDENTITY, H, W)
    K, quad = C.quad_scene(H, W, pose=C.general_pose())
    assert (_check([quad], K, C.general_pose(), H, W)[3] == 1).all()
    K, fan = C.fan_scene(H, W)
    assert _check([fan], K, C.IDENTITY, H, W)[3].max() <= 1
    K, tie = C.tie_scene(H, W)
    assert _check([tie], K, C.IDENTITY, H, W)[2].max() <= 0


# ------------------------------------------------------------------------------------------------ 2
def test_triangle_size_ladder_runs_both_raster_paths(gpu_ctx):
    """Isolated right triangles with legs of 1 .. 40 pixels at random sub-pixel offsets on 48 x 64.  A face whose clipped box holds more than 64 pixels is drawn by a
    workgroup, the others by one thread: legs up to 6 (a box of at most 7 x 7) take the one path, legs from 9 (at least 9 x 9) the other."""
    from hive_amd.render import RenderBuffers, render_mesh
    H, W = 48, 64
    K = C.intrinsics(H, W)
    rng = np.random.default_rng(5)
    buffers = RenderBuffers(H, W)
    for leg in range(1, 41):
        u0, v0 = 3.0 + rng.random(), 3.0 + rng.random()
        mesh = C.coloured(C.unproject(K, [u0, u0 + leg, u0], [v0, v0, v0 + leg], 1.0 + rng.random(3)), [[0, 1, 2]], seed=leg)
        want = RR.render([mesh], K, np.eye(3), np.zeros(3), H, W)
        got = render_mesh(K, C.IDENTITY, mesh, size=(H, W), return_depth=True, return_faces=True, buffers=buffers)
        _same(tuple(x.cpu().numpy() for x in got), want)
        assert want[3].sum() >= leg * (leg - 1) // 2
        small, large = buffers.path_counts()
        assert small + large == 1
        if leg <= 6:
            assert (small, large) == (1, 0)
        if leg >= 9:
            assert (small, large) == (0, 1)


# ------------------------------------------------------------------------------------------------ 3
def _soup(K, H, W, n, rng, integer):
    """n random triangles in screen space with a random depth per vertex; the first faces are the special ones."""
    centre = np.stack([rng.uniform(-6, W + 6, n), rng.uniform(-6, H + 6, n)], -1)
    reach = rng.choice([1.5, 4.0, 12.0], size=(n, 1, 1))
    pts = centre[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 2)) * reach
    if integer:
        pts = np.round(pts)  # vertices on samples, edges through samples
    z = rng.uniform(1.0, 4.0, (n, 3))
    if integer:
        z = np.round(z * 4) / 4  # many equal depths: ties
    z[0] = -2.0                                   # behind the camera
    z[1] = [2.0, 2.0, -0.5]                       # straddling the camera plane
    z[2] = [2.0, 0.01, 2.0]                       # straddling near
    z[3] = [0.05, 0.05, 0.05]                     # exactly at near: kept
    pts[4] = [[-300.0, 5.0], [-280.0, 5.0], [-300.0, 30.0]]      # off screen
    pts[5] = [[W + 50.0, H + 50.0], [W + 90.0, H + 50.0], [W + 50.0, H + 99.0]]
    pts[6] = [[10.0, 10.0], [20.0, 20.0], [30.0, 30.0]]          # zero area
    pts[7] = [[12.5, 7.25], [12.5, 7.25], [40.0, 9.0]]           # two vertices on one point
    pts[8] = [[70000.0, 10.0], [10.0, 10.0], [10.0, 30.0]]       # beyond the guard band
    pts[9] = [[10.0, -65536.0], [10.0, 10.0], [30.0, 10.0]]      # on it
    pts[10] = [[-20.0, -20.0], [W + 40.0, -20.0], [-20.0, H + 60.0]]  # a large face behind most
    z[10] = 3.9
    vertices = C.unproject(K, pts[..., 0].reshape(-1), pts[..., 1].reshape(-1), z.reshape(-1))
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    faces[11] = [33, 34, 34]                      # a repeated vertex
    return vertices, faces


@pytest.mark.parametrize("integer", [False, True], ids=["subpixel", "integer"])
def test_soup(gpu_ctx, integer):
    """2,000 random triangles on 48 x 64, the rejected kinds among them, with vertex colours and with a texture; permuting the faces leaves the depth unchanged."""
    H, W = 48, 64
    K = C.intrinsics(H, W)
    rng = np.random.default_rng(11 + integer)
    vertices, faces = _soup(K, H, W, 2000, rng, integer)
    col = {"vertices": vertices, "faces": faces, "vertex_colors": rng.integers(0, 256, (len(vertices), 3), dtype=np.uint8)}
    tex = {"vertices": vertices, "faces": faces, "uv": rng.uniform(-0.1, 1.1, (len(vertices), 2)), "texture": rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)}
    for pose in (C.IDENTITY, C.general_pose()):
        moved = C.to_world(vertices, pose)
        want = _check([dict(col, vertices=moved)], K, pose, H, W)
        assert want[3].max() > 3 and (want[2] >= 0).mean() > 0.9
        want_tex = _check([dict(tex, vertices=moved)], K, pose, H, W)
        assert np.array_equal(want_tex[1].view(np.uint32), want[1].view(np.uint32))
        order = rng.permutation(len(faces))
        got = _gpu([dict(col, vertices=moved, faces=np.ascontiguousarray(faces[order]))], K, pose, H, W)
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4
def test_ties_and_several_meshes(gpu_ctx):
    H, W = 48, 64
    K, tie = C.tie_scene(H, W)
    assert set(np.unique(_check([tie], K, C.IDENTITY, H, W)[2])) == {-1, 0}  # duplicated faces inside one mesh
    a = dict(tie, faces=tie["faces"][:1])
    b = dict(a, vertex_colors=255 - a["vertex_colors"])
    for first, second in ((a, b), (b, a)):  # the same triangle in two meshes: the lower global index wins, so the first argument's colours show
        color, _, face, _ = _check([first, second], K, C.IDENTITY, H, W)
        assert set(np.unique(face)) == {-1, 0}
        assert np.array_equal(color, _check([first], K, C.IDENTITY, H, W)[0])
    # None and empty meshes take no face numbers
    empty = {"vertices": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int32), "vertex_colors": np.zeros((0, 3), np.uint8)}
    _same(_gpu([None, a, empty, b], K, C.IDENTITY, H, W), RR.render([a, b], K, np.eye(3), np.zeros(3), H, W))
    # a vertex-colour quad cutting through a textured grid
    s = C.grid_scene(H, W, seed=3)
    cut = C.coloured(C.unproject(s["K"], [2.0, W - 3.5, W - 3.5, 2.0], [1.5, 1.5, H - 2.0, H - 2.0], [1.2, 2.2, 2.2, 1.2]), [[0, 1, 2], [0, 2, 3]])
    for meshes in ([s["textured"], cut], [cut, s["textured"]]):
        face = _check(meshes, s["K"], C.IDENTITY, H, W)[2]
        n_grid = len(s["textured"]["faces"])
        grid_won = (face >= 0) & ((face < n_grid) if meshes[0] is not cut else (face >= 2))
        assert grid_won.sum() > 300 and ((face >= 0) & ~grid_won).sum() > 300


# ------------------------------------------------------------------------------------------------ 5
@pytest.fixture(scope="module")
def small_frames():
    from hive_amd import synthetic
    return synthetic.make_sequence(num_frames=2, height=48, width=64, yaw_step_deg=25.0)


def test_fused_background_mesh(gpu_ctx, small_frames):
    """TSDFVolume.get_mesh() of a 32^3 volume fused from two 48 x 64 frames, from both frames' poses and from one moved into the room."""
    from hive_amd import fusion, synthetic
    from hive_amd.mesh import Mesh
    seq = small_frames
    vol = fusion.TSDFVolume(synthetic.room_bounds(), 0.16, ctx=gpu_ctx)
    for i in range(2):
        vol.integrate(seq["color"][i], seq["depth"][i], seq["K"], seq["poses"][i])
    verts, faces, norms, colors = vol.get_mesh()
    assert len(faces) > 200
    lo, hi = verts.min(0), verts.max(0)
    mesh = Mesh(verts, faces, vertex_colors=colors, vertex_normals=norms)
    inside = seq["poses"][1].copy()
    inside[:3, 3] = (lo.astype(np.float64) + hi) / 2  # the middle of the surface's bounding box: faces all around, some nearer than `near`
    K = np.asarray(seq["K"], np.float64)
    for c2w in (seq["poses"][0], seq["poses"][1], inside):
        want = _check([mesh], K, np.linalg.inv(c2w), 48, 64)
        assert (want[2] >= 0).mean() > (0.3 if c2w is not inside else 0.0)


def test_foreground_frame_mesh(gpu_ctx, small_frames):
    """A process_frame mesh of a 48 x 64 frame (device tensors, textured through the atlas uv) from its own pose and from a shifted one; from its own pose every
    vertex is back on its pixel, so the picture there is the frame."""
    import torch
    from hive_amd import foreground, synthetic
    from hive_amd.options import MaskDilationOptions
    seq = small_frames
    ids = synthetic.ellipse_masks(1, 48, 64, num_objects=2, seed=3)[0].copy()
    ids[seq["depth"][0] == 0] = 0
    pose = np.linalg.inv(seq["poses"][0])
    mesh = foreground.process_frame(torch.from_numpy(seq["color"][0]).cuda(), torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(ids).cuda(), seq["K"], pose,
                                    MaskDilationOptions(num_iterations=0), ctx=gpu_ctx, disable_coverage_constraint=True)
    assert mesh is not None and mesh["faces"].shape[0] > 50
    K = np.asarray(seq["K"], np.float64)
    shifted = pose.copy()
    shifted[:3, 3] += [0.07, -0.04, 0.1]
    host = _host(mesh)
    for p in (pose, shifted):
        want = RR.render([host], K, p[:3, :3], p[:3, 3], 48, 64)
        _same(_gpu([mesh], K, p, 48, 64), want)
        assert (want[2] >= 0).sum() > 50
    own = RR.render([host], K, pose[:3, :3], pose[:3, 3], 48, 64)
    hit = own[2] >= 0
    assert np.array_equal(own[0][hit], seq["color"][0][hit])


# ------------------------------------------------------------------------------------------------ 6
def test_known_answers_at_640x480(gpu_ctx):
    """The workload's size without the restatement: the grid round trip (small faces) and the screen-filling quad (the large-face path)."""
    from hive_amd.render import RenderBuffers, render_mesh
    H, W = 480, 640
    s = C.grid_scene(H, W, seed=2)
    block = np.zeros((H, W), bool)
    block[:H - 1, :W - 1] = True
    buffers = RenderBuffers(H, W)
    for name in ("textured", "coloured"):
        color, depth, face = (x.cpu().numpy() for x in render_mesh(s["K"], C.IDENTITY, s[name], size=(H, W), return_depth=True, return_faces=True, buffers=buffers))
        assert np.array_equal(face >= 0, block)
        assert np.array_equal(depth[block].view(np.uint32), s["depth"][block].view(np.uint32)) and (depth[~block] == 0).all()
        assert np.array_equal(color[block], s["image"][block]) and (color[~block] == 255).all()
        assert buffers.path_counts() == (len(s[name]["faces"]), 0)
    K, quad = C.quad_scene(H, W)
    color, depth, face = (x.cpu().numpy() for x in render_mesh(K, C.IDENTITY, quad, size=(H, W), return_depth=True, return_faces=True, buffers=buffers))
    assert buffers.path_counts() == (0, 2)
    assert (depth.view(np.uint32) == np.float32(2.0).view(np.uint32)).all()
    ii, jj = np.mgrid[0:H, 0:W]
    # the diagonal from (-8, -8) to (W + 16, H + 12): face 0 = [0, 1, 2] holds the samples above it, and by the top-left rule none on it belongs to both
    side = (jj + 8.0) * (H + 20.0) - (ii + 8.0) * (W + 24.0)
    assert (face[side > 0] == 0).all() and (face[side < 0] == 1).all() and set(np.unique(face)) == {0, 1}
    flat = RR.render([quad], K, np.eye(3), np.zeros(3), 8, 8)[0]  # (the colours of a corner, from the restatement at a size it is quick at)
    assert np.array_equal(color[:8, :8], flat)


# ------------------------------------------------------------------------------------------------ 7
def test_plumbing(gpu_ctx):
    import torch
    from hive_amd.geometric import CameraMatrix, pose_mat2vec
    from hive_amd.render import RenderBuffers, render_mesh
    H, W = 24, 32
    pose = C.general_pose()
    s = C.grid_scene(H, W, pose=pose)
    K = s["K"]
    host = [s["textured"], dict(s["coloured"], vertices=s["coloured"]["vertices"] + [0.0, 0.0, 0.01])]
    kept = [{k: np.array(v, copy=True) for k, v in m.items()} for m in host]
    dev = [{k: torch.from_numpy(v).cuda() for k, v in m.items()} for m in host]
    dev_kept = [{k: v.clone() for k, v in m.items()} for m in dev]
    a = _gpu(host, K, pose, H, W)
    b = _gpu(dev, K, pose, H, W)
    c = _gpu(dev, torch.from_numpy(K), torch.from_numpy(pose), H, W, buffers=RenderBuffers(H, W))
    for other in (b, c, _gpu(host, K, pose, H, W)):
        _same(other, a)
    for m, k in list(zip(host, kept)) + [({n: v.cpu().numpy() for n, v in m.items()}, {n: v.cpu().numpy() for n, v in k.items()}) for m, k in zip(dev, dev_kept)]:
        assert all(np.array_equal(m[n], k[n]) for n in m)
    # the camera as a CameraMatrix and a 7-vector, the flags one by one
    cam = CameraMatrix.from_matrix(K, (H, W))
    only = render_mesh(cam, pose_mat2vec(pose), *host)
    assert only.dtype == torch.uint8 and tuple(only.shape) == (H, W, 3) and only.is_cuda
    color, depth = render_mesh(cam, pose, *host, return_depth=True)
    color2, face = render_mesh(cam, pose, *host, return_faces=True)
    assert depth.dtype == torch.float32 and face.dtype == torch.int32
    assert np.array_equal(color.cpu().numpy(), a[0]) and np.array_equal(color2.cpu().numpy(), a[0])
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), a[1].view(np.uint32)) and np.array_equal(face.cpu().numpy(), a[2])
    # nothing to draw: the background, depth 0, face -1
    empty = {"vertices": np.zeros((0, 3)), "faces": np.zeros((0, 3), np.int32), "vertex_colors": np.zeros((0, 3), np.uint8)}
    for meshes in ([], [None], [empty, None]):
        color, depth, face = _gpu(meshes, K, pose, H, W, background=(1, 2, 3))
        assert (color == [1, 2, 3]).all() and (depth == 0).all() and (face == -1).all()
    assert (_gpu([], K, pose, H, W)[0] == 255).all()
    # errors
    with pytest.raises(ValueError):
        render_mesh(K, pose, host[0], size=(H, W), near=0.0)
    with pytest.raises(ValueError):
        render_mesh(K, pose, host[0], size=(H, 0))
    for bad in (-1, H * W):
        faces = s["coloured"]["faces"].copy()
        faces[7, 1] = bad
        with pytest.raises(ValueError):
            render_mesh(K, pose, dict(s["coloured"], faces=faces), size=(H, W))
