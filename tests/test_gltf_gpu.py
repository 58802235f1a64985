"""glTF export on the GPU: ``hive_gltf_pack`` (csrc/gltf.hip) bit for bit against the numpy restatement (tests/gltf_restatement.py), the quantisation's edge
cases and error bound, batch independence, the failures that name a mesh, ``write_glb`` / ``read_glb`` round trips through the renderer, and
``Pipeline.run(export_gltf=True)`` end to end."""
import ctypes
import json
import os

import numpy as np
import pytest

import gltf_restatement as R

pytestmark = pytest.mark.gpu


def _mesh(rng, V, F, wide_vertices, wide_faces, uv=False, channels=0):
    mesh = {"vertices": (rng.normal(size=(V, 3)) * [3.0, 0.5, 40.0] + [0.0, -7.0, 100.0]).astype(np.float64 if wide_vertices else np.float32),
            "faces": rng.integers(0, V, (F, 3)).astype(np.int64 if wide_faces else np.int32)}
    if uv:
        mesh["uv"] = rng.random((V, 2))
    if channels:
        mesh["colors"] = rng.integers(0, 256, (V, channels), dtype=np.uint8)
    return mesh


def _batches():
    """Seven meshes for ONE call and two for a second one.  A pack workgroup takes 256 elements of the concatenated ranges (V per vertex attribute, F for the
    indices): mesh 0 ends ON a workgroup boundary (1 + 1 + 254 = 256), mesh 1 one element BEFORE the next (256 + 63 + 63 + 129 = 511), mesh 2 one AFTER the one
    after it (511 + 64 + 64 + 130 = 769).  V = 65535 / 65536 switch the quantised index type; 270000 vertices give the bounds' final stage more chunks (264) than
    it has threads.  Odd F: uint16 indices that end off a 4-byte boundary."""
    rng = np.random.default_rng(2024)
    first = [_mesh(rng, 1, 254, True, True, uv=True), _mesh(rng, 63, 129, False, False, channels=3), _mesh(rng, 64, 130, True, False, channels=4),
             _mesh(rng, 65, 77, False, True, uv=True), _mesh(rng, 256, 301, True, True, channels=3), _mesh(rng, 257, 500, False, False, uv=True),
             _mesh(rng, 65535, 70001, True, True, uv=True)]
    second = [_mesh(rng, 65536, 70001, True, False, channels=4), _mesh(rng, 270000, 1001, False, True, channels=3)]
    first[6]["faces"][:2] = [[65534, 0, 65534], [0, 65534, 1]]
    second[0]["faces"][0] = [65535, 0, 65535]
    return first, second


BATCHES = _batches()
LUT = (255 * np.power(np.arange(256) / 255, 2.2)).astype(np.uint8)
_REFERENCE = {}


def reference(which, quantize):
    """The restatement's (bytes, bounds, views) of a batch, computed once."""
    key = (which, bool(quantize))
    if key not in _REFERENCE:
        meshes = BATCHES[which]
        data, bounds = R.pack(meshes, quantize, LUT)
        _REFERENCE[key] = (data, bounds, R.layout(meshes, quantize)[0])
    return _REFERENCE[key]


def native_pack(ctx, meshes, quantize, lut=None, out_bytes=None):
    """hive_gltf_layout + hive_gltf_pack of host meshes (uploaded as they are) -> (bytes, bounds, views).  The output buffer has 64 guard bytes behind it."""
    import torch
    from hive_amd import _lib
    lib = ctx.lib
    keep, table = [], (_lib.GltfMesh * len(meshes))()
    for row, mesh in zip(table, meshes):
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mesh.items()}
        keep.append(dev)
        row.vertices, row.faces = dev["vertices"].data_ptr(), dev["faces"].data_ptr()
        row.n_vertices, row.n_faces = mesh["vertices"].shape[0], mesh["faces"].shape[0]
        row.vertex_dtype = _lib.GLTF_F64 if mesh["vertices"].dtype == np.float64 else _lib.GLTF_F32
        row.face_dtype = _lib.GLTF_I64 if mesh["faces"].dtype == np.int64 else _lib.GLTF_I32
        if "uv" in mesh:
            row.uv = dev["uv"].data_ptr()
        if "colors" in mesh:
            row.colors, row.color_channels = dev["colors"].data_ptr(), mesh["colors"].shape[1]
    views = (_lib.GltfView * (4 * len(meshes)))()
    total = ctypes.c_int64(0)
    _lib.check(lib.hive_gltf_layout(table, len(meshes), int(quantize), views, total))
    out = torch.full((total.value + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    bounds = np.full((len(meshes), 2, 3), np.nan)
    lut = None if lut is None else np.ascontiguousarray(lut, np.uint8)
    ctx.check(lib.hive_gltf_pack(ctx.handle, table, len(meshes), int(quantize), _lib.ptr(lut), out.data_ptr(), total.value if out_bytes is None else out_bytes,
                                 _lib.ptr(bounds)))
    data = out.cpu().numpy()
    assert np.all(data[total.value:] == 0xAB), "nothing is written behind the layout's total"
    return data[:total.value].tobytes(), bounds, [[(v.offset, v.length) for v in views[4 * k:4 * k + 4]] for k in range(len(meshes))]


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_packed_bytes_and_bounds_equal_the_restatement(gpu_ctx, which, quantize):
    want, want_bounds, want_views = reference(which, quantize)
    got, bounds, views = native_pack(gpu_ctx, BATCHES[which], quantize, LUT)
    assert views == want_views
    assert np.array_equal(bounds, want_bounds)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.nonzero(a != b)[0][0])
        owner = [(k, kind) for k, row in enumerate(views) for kind, (offset, length) in enumerate(row) if offset <= at < offset + max(length, 1)]
        pytest.fail(f"first difference at byte {at} of {len(b)} (mesh, view) = {owner}: {a[at:at + 8]} != {b[at:at + 8]}")
    if quantize:  # the index type switches between 65535 and 65536 vertices
        V, F, row = len(BATCHES[which][-1 if which == 0 else 0]["vertices"]), 70001, views[-1 if which == 0 else 0]
        assert row[R.INDICES][1] == F * 3 * (2 if V <= 65535 else 4)


def test_a_mesh_alone_equals_the_mesh_in_the_batch_and_runs_repeat(gpu_ctx):
    for quantize in (False, True):
        whole, bounds, views = native_pack(gpu_ctx, BATCHES[0], quantize, LUT)
        again, _, _ = native_pack(gpu_ctx, BATCHES[0], quantize, LUT)
        assert whole == again, "two runs give the same bytes"
        for k in (0, 1, 2, 5, 6):
            alone, alone_bounds, alone_views = native_pack(gpu_ctx, [BATCHES[0][k]], quantize, LUT)
            assert np.array_equal(alone_bounds[0], bounds[k])
            for (o0, n0), (o1, n1) in zip(alone_views[0], views[k]):
                assert n0 == n1 and alone[o0:o0 + n0] == whole[o1:o1 + n1], (k, quantize)


def test_quantisation_ties_flat_axis_and_clamped_uv(gpu_ctx):
    """Integers with lo = 0 and hi = 131070 give s = 2 exactly: every odd coordinate x = 2 k + 1 is the tie k + 0.5 and must round to the EVEN neighbour.  z is flat
    (hi == lo): s = 1, q = 0.  uv below 0 and above 1 clamp to 0 and 65535 (v is flipped first: v' = 1 - v)."""
    k = np.array([0, 1, 2, 3, 16382, 16383, 32767, 32768, 65533], np.float64)
    odd = 2.0 * k + 1.0
    vertices = np.zeros((len(odd) + 2, 3))
    vertices[:len(odd), 0], vertices[:len(odd), 1] = odd, odd[::-1]
    vertices[len(odd)] = [0.0, 131070.0, 0.0]
    vertices[len(odd) + 1] = [131070.0, 0.0, 0.0]
    vertices[:, 2] = 7.25
    V = len(vertices)
    uv = np.linspace(0.0, 1.0, 2 * V).reshape(V, 2)
    uv[0], uv[1], uv[2], uv[3] = [-0.5, 1.5], [1.5, -0.5], [-1e-300, 1.0 + 1e-16], [0.5, 0.5]
    mesh = {"vertices": vertices, "faces": np.array([[0, 1, 2], [2, 3, V - 1], [V - 1, V - 2, 0]], np.int32), "uv": uv}
    data, bounds, views = native_pack(gpu_ctx, [mesh], True)
    assert np.array_equal(bounds[0], [[0, 0, 7.25], [131070, 131070, 7.25]])
    q = np.frombuffer(data, "<u2", 4 * V, views[0][R.POSITION][0]).reshape(V, 4)
    even = np.where(k % 2 == 0, k, k + 1)  # k + 0.5 -> the even one of k, k + 1
    assert np.array_equal(q[:len(odd), 0], even) and np.array_equal(q[:len(odd), 1], even[::-1])
    assert np.array_equal(q[len(odd):, :2], [[0, 65535], [65535, 0]])
    assert not q[:, 2].any() and not q[:, 3].any(), "a flat axis gives q = 0; the stride's last two bytes are 0"
    t = np.frombuffer(data, "<u2", 2 * V, views[0][R.TEXCOORD][0]).reshape(V, 2)
    assert np.array_equal(t[:3], [[0, 0], [65535, 65535], [0, 0]])
    assert np.array_equal(t[3], [32768, 32768]), "0.5 * 65535 = 32767.5 is a tie -> the even 32768"
    assert data == R.pack([mesh], True)[0]
    idx = np.frombuffer(data, "<u2", 9, views[0][R.INDICES][0])
    assert np.array_equal(idx.reshape(3, 3), mesh["faces"]) and data[views[0][R.INDICES][0] + 18:] == b"\0\0", "9 uint16 indices and 2 bytes of padding"


def test_decoded_positions_are_within_half_a_step(gpu_ctx):
    """|x' - x| <= s / 2 + 4 ulp(larger bound): x' = q s + lo in float64.  The four ulps are for the rule's one division, one multiplication and two additions
    (x - lo, q s + lo), each rounded once at the magnitude of the larger bound at most."""
    for mesh in (BATCHES[0][4], BATCHES[0][6], BATCHES[0][5]):
        data, bounds, views = native_pack(gpu_ctx, [mesh], True)
        V = len(mesh["vertices"])
        q = np.frombuffer(data, "<u2", 4 * V, views[0][R.POSITION][0]).reshape(V, 4)[:, :3].astype(np.float64)
        lo, hi = bounds[0]
        s = R.step_of(lo, hi)
        decoded = q * s + lo
        error = np.abs(decoded - mesh["vertices"].astype(np.float64))
        bound = s / 2 + 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        print("largest error / bound per axis:", (error / bound).max(axis=0))
        assert np.all(error <= bound)
        assert q.min() == 0 and q.max() == 65535


def test_failures_name_the_mesh(gpu_ctx):
    from hive_amd import _lib
    rng = np.random.default_rng(5)
    good = lambda: _mesh(rng, 40, 30, True, True, channels=3)
    bad_index = good()
    bad_index["faces"][17, 1] = 40  # == V
    with pytest.raises(_lib.HiveError, match=r"mesh 1 has a face index outside \[0, 40\)"):
        native_pack(gpu_ctx, [good(), bad_index, good()], False)
    negative = good()
    negative["faces"][3, 0] = -1
    with pytest.raises(_lib.HiveError, match="mesh 0 has a face index outside"):
        native_pack(gpu_ctx, [negative, bad_index], True)
    for value in (np.nan, np.inf):
        bad_vertex = good()
        bad_vertex["vertices"][39, 2] = value
        with pytest.raises(_lib.HiveError, match="mesh 2 has a vertex that is not finite"):
            native_pack(gpu_ctx, [good(), good(), bad_vertex, bad_vertex], False)
    no_faces = good()
    no_faces["faces"] = np.zeros((0, 3), np.int64)
    with pytest.raises(_lib.HiveError, match="mesh 1 has n_faces == 0"):
        native_pack(gpu_ctx, [good(), no_faces], False)
    meshes = [good(), good()]
    _, total = R.layout(meshes, False)
    with pytest.raises(_lib.HiveError, match=rf"out_bytes = {total - 4} is too small for mesh 1"):
        native_pack(gpu_ctx, meshes, False, out_bytes=total - 4)
    with pytest.raises(_lib.HiveError, match="is too small for mesh 0"):
        native_pack(gpu_ctx, meshes, False, out_bytes=8)
    native_pack(gpu_ctx, meshes, False)  # the context still works


@pytest.fixture(scope="module")
def frame_meshes(gpu_ctx):
    """A ``process_frame`` dict (two ellipse objects of a 240 x 320 frame, device-resident) and a coloured ``Mesh`` beside it, with the camera that saw them."""
    import torch
    from hive_amd import foreground, synthetic
    from hive_amd.mesh import Mesh
    from hive_amd.options import MaskDilationOptions, MeshFilteringOptions
    H, W = 240, 320
    seq = synthetic.make_sequence(num_frames=1, height=H, width=W)
    ids = synthetic.ellipse_masks(1, H, W, num_objects=2, seed=3)[0].copy()
    ids[seq["depth"][0] == 0] = 0
    pose = np.linalg.inv(seq["poses"][0])
    frame = foreground.process_frame(torch.from_numpy(seq["color"][0]).cuda(), torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(ids).cuda(), seq["K"], pose,
                                     MaskDilationOptions(num_iterations=0), MeshFilteringOptions(), ctx=gpu_ctx, enable_cc_analysis=True)
    frame = {key: frame[key] for key in ("vertices", "faces", "uv", "texture")}
    assert frame["vertices"].dtype == torch.float64 and frame["faces"].shape[0] > 100
    rng = np.random.default_rng(8)
    v = frame["vertices"].cpu().numpy() + (seq["poses"][0][:3, :3] @ np.array([0.4, 0.0, 0.1]))
    coloured = Mesh(v, frame["faces"].cpu().numpy().astype(np.int32), rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
    return frame, coloured, seq["K"], pose, (H, W)


@pytest.mark.parametrize("quantize", [False, True])
def test_write_then_read_round_trip(gpu_ctx, tmp_path, frame_meshes, quantize):
    from hive_amd import gltf, render
    frame, coloured, K, pose, size = frame_meshes
    scene = gltf.Scene(camera=dict(resolution=(size[1], size[0]), focal=(K[0, 0], K[1, 1])))
    scene.add_geometry(frame, node_name="000000")
    scene.add_geometry(coloured, node_name="static")
    scene.add_geometry({"vertices": frame["vertices"], "faces": frame["faces"][:0], "uv": frame["uv"], "texture": frame["texture"]}, node_name="no_faces")
    path = str(tmp_path / "scene.glb")
    sizes = gltf.write_glb(path, scene, quantize=quantize, lut=LUT)
    with open(path, "rb") as f:
        blob = f.read()
    doc, binary = R.check_container(blob)
    assert sizes["total"] == len(blob) and sizes["geometry"] + sizes["images"] <= len(binary)
    assert [doc["nodes"][c]["name"] for c in doc["nodes"][0]["children"]] == ["000000", "static"], "the node without faces is left out"
    assert doc["nodes"][0]["name"] == "world" and doc["nodes"][0]["matrix"] == [float(v) for v in np.eye(4).ravel()]
    assert ("extensionsRequired" in doc) == quantize and len(doc["images"]) == len(doc["textures"]) == len(doc["materials"]) == 1
    back = gltf.read_glb(path)
    a, b = back.meshes()
    v, f, uv = frame["vertices"].cpu().numpy(), frame["faces"].cpu().numpy(), frame["uv"].cpu().numpy()
    assert np.array_equal(a["faces"], f) and np.array_equal(b.faces, coloured.faces)
    assert np.array_equal(a["texture"], frame["texture"].cpu().numpy()[:, :, :3])
    assert np.array_equal(b.visual.vertex_colors[:, :3], LUT[coloured.visual.vertex_colors[:, :3]]) and np.all(b.visual.vertex_colors[:, 3] == 255)
    if quantize:
        for got, original in ((a["vertices"], v), (b.vertices, coloured.vertices)):
            lo, hi = original.min(axis=0), original.max(axis=0)
            assert np.all(np.abs(got - original) <= R.step_of(lo, hi) / 2 + 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi))))
        assert np.all(np.abs(a["uv"] - uv) <= 0.5 / 65535.0 + 2 * np.spacing(1.0))
        return
    assert np.array_equal(a["vertices"], v.astype(np.float32).astype(np.float64)), "vertices equal to float32 of the originals"
    assert np.array_equal(b.vertices, coloured.vertices.astype(np.float32).astype(np.float64))
    # uv equal in float32: what the file stores is float32 of (u, 1 - v); read_glb flips v back in float64
    stored = R.texcoords(uv).astype(np.float32)
    assert np.array_equal(a["uv"], np.stack([stored[:, 0].astype(np.float64), 1.0 - stored[:, 1].astype(np.float64)], axis=1))
    assert np.array_equal(R.texcoords(a["uv"]).astype(np.float32), stored)
    # the renderer sees the same picture: read-back meshes == originals with their vertices rounded to float32 (the coloured one with the table applied)
    from hive_amd.mesh import Mesh
    rounded = dict(frame, vertices=frame["vertices"].float().double())
    rounded_coloured = Mesh(coloured.vertices.astype(np.float32).astype(np.float64), coloured.faces, LUT[coloured.visual.vertex_colors[:, :3]])
    want = render.render_mesh(K, pose, rounded, rounded_coloured, size=size, ctx=gpu_ctx)
    got = render.render_mesh(K, pose, *back.meshes(apply_transform=False), size=size, ctx=gpu_ctx)
    assert (want.cpu().numpy() != 255).any(axis=2).mean() > 0.02, "the meshes are in view"
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_pipeline_run_exports_gltf(gpu_ctx, tmp_path):
    """``run(export_gltf=True)`` on the TUM-layout fixture with three ellipse masks: the three files in mesh/ and in the export folder; the fg nodes are the frames
    that have a PLY; bg.glb's colours are the PLY's, i.e. the sRGB table of the fused mesh's (the table is applied once, on the device, as the reference applies it
    once to the static mesh); every PLY and PNG byte-identical to a run without the flag, which writes nothing new; the compression record holds the two file sizes;
    a second export into the same folder fails without ``overwrite_ok``."""
    from PIL import Image
    from hive_amd import gltf, synthetic
    from hive_amd.dataset_adaptors import get_dataset
    from hive_amd.options import BackgroundMeshOptions, PipelineOptions, StorageOptions, WebXROptions
    from hive_amd.pipeline import Pipeline
    from test_fgclean_gpu import read_ply
    from tum_fixture import write_tum_sequence
    tum, hive = str(tmp_path / "tum"), str(tmp_path / "hive")
    n = 3
    write_tum_sequence(tum, num_frames=n, yaw_step_deg=10.0)
    ds = get_dataset(tum, hive)
    masks = synthetic.ellipse_masks(n, ds.frame_height, ds.frame_width, num_objects=3, seed=5)
    for name, m in zip(sorted(os.listdir(os.path.join(hive, "mask"))), masks):
        Image.fromarray(m).save(os.path.join(hive, "mask", name))
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.04, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)
    webxr = WebXROptions(webxr_path=str(tmp_path / "player" / "video"))

    plain = Pipeline(options=PipelineOptions(num_frames=n), background_mesh_options=bg_options, webxr_options=webxr)
    plain.run(hive, str(tmp_path / "plain"))
    listing = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    plain_files = listing(tmp_path / "plain")
    assert not any(f.endswith((".glb", "metadata.json")) for f in plain_files) and not (tmp_path / "player").exists()
    assert "mesh_compression" not in plain.profiling and "scene_centering" not in plain.profiling["timing"]

    pipe = Pipeline(options=PipelineOptions(num_frames=n), background_mesh_options=bg_options, webxr_options=webxr)
    static_mesh = pipe.run(hive, str(tmp_path / "export"), export_gltf=True)
    mesh_dir, export_dir = tmp_path / "export" / "mesh", tmp_path / "player" / "video" / "hive"
    assert listing(tmp_path / "export") == sorted(plain_files + [os.path.join("mesh", f) for f in ("fg.glb", "bg.glb", "metadata.json")])
    for name in plain_files:
        with open(tmp_path / "plain" / name, "rb") as a, open(tmp_path / "export" / name, "rb") as b:
            assert a.read() == b.read(), name
    assert sorted(os.listdir(export_dir)) == ["bg.glb", "fg.glb", "metadata.json"]
    for name in ("bg.glb", "fg.glb", "metadata.json"):
        with open(mesh_dir / name, "rb") as a, open(export_dir / name, "rb") as b:
            assert a.read() == b.read(), name
    with open(mesh_dir / "metadata.json") as f:
        assert json.load(f) == dict(fps=ds.fps, fov_y=int(np.rad2deg(2 * np.arctan2(ds.frame_height, 2 * float(ds.camera_matrix[1, 1])))), num_frames=n,
                                    use_vertex_colour_for_bg=True, add_ground_plane=False, add_sky_box=False)
    for name in ("fg.glb", "bg.glb"):
        with open(mesh_dir / name, "rb") as f:
            doc, _ = R.check_container(f.read())
        assert doc["extensionsRequired"] == ["KHR_mesh_quantization"], "compress=True (the default) leaves the quantised files"
    fg, bg = gltf.read_glb(str(mesh_dir / "fg.glb")), gltf.read_glb(str(mesh_dir / "bg.glb"))
    assert list(fg.geometry) == sorted(f[:-4] for f in os.listdir(mesh_dir / "fg") if f.endswith(".ply")) and len(fg.geometry) > 0
    assert list(bg.geometry) == ["000000"]
    for name, node in fg.geometry.items():  # every frame's node is that frame's PLY and PNG: half a quantisation step, + 1e-6 for the PLY's own float32 rounding (half an ulp is 4.8e-7 below 8 m)
        _, v, f = read_ply(str(mesh_dir / "fg" / f"{name}.ply"))
        xyz = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float64)
        assert np.array_equal(node["faces"], f) and np.array_equal(node["texture"], np.asarray(Image.open(mesh_dir / "fg" / f"{name}.png")))
        assert np.all(np.abs(node["vertices"] - xyz) <= R.step_of(xyz.min(axis=0), xyz.max(axis=0)) / 2 + 1e-6), name
        assert np.all(np.abs(node["uv"] - np.stack([v["texture_u"], v["texture_v"]], axis=1)) <= 0.5 / 65535 + 1e-6), name
    assert np.array_equal(fg.transform, bg.transform) and np.array_equal(fg.transform[:3, :3], np.diag([-1.0, -1.0, 1.0]))
    assert np.array_equal(fg.transform[:3, 3], fg.transform[:3, 3].astype(np.float32)), "the offset is a float32"
    _, ply_v, ply_f = read_ply(str(mesh_dir / "bg.ply"))
    ply_colours = np.stack([ply_v["red"], ply_v["green"], ply_v["blue"]], axis=1)
    glb_mesh = bg.meshes()[0]
    assert np.array_equal(glb_mesh.visual.vertex_colors[:, :3], ply_colours)
    assert np.array_equal(ply_colours, LUT[np.asarray(static_mesh.visual.vertex_colors)[:, :3]])
    assert np.array_equal(glb_mesh.faces, ply_f)
    xyz = np.stack([ply_v["x"], ply_v["y"], ply_v["z"]], axis=1).astype(np.float64)
    assert np.all(np.abs(glb_mesh.vertices - xyz) <= R.step_of(xyz.min(axis=0), xyz.max(axis=0)) / 2 + 1e-6)
    # centred: the joint bounds sit on y = 0 and z = 0 and are centred in x (to the quantisation step and the float32 offset)
    joint = Pipeline._get_scene_bounds(fg, bg)
    assert abs(joint[0, 0] + joint[1, 0]) < 1e-3 and abs(joint[0, 1]) < 1e-3 and abs(joint[0, 2]) < 1e-3
    record = pipe.profiling["mesh_compression"]
    for key, name in (("foreground", "fg.glb"), ("background", "bg.glb")):
        assert set(record[key]) == {"uncompressed_file_size", "compressed_file_size", "data_saving", "compression_ratio"}
        assert record[key]["compressed_file_size"] == os.path.getsize(mesh_dir / name) < record[key]["uncompressed_file_size"]
        assert record[key]["compression_ratio"] == record[key]["uncompressed_file_size"] / record[key]["compressed_file_size"]
    timing = pipe.profiling["timing"]
    assert timing["scene_centering"] >= 0 and timing["mesh_export"] > 0 and timing["webxr_export"] > 0
    assert set(timing["mesh_compression"]) == {"total", "foreground", "background"}
    with open(os.path.join(hive, "profiling.json")) as f:
        assert "mesh_compression" in json.load(f)
    # compress=False leaves the plain files; a second export into the same folder fails unless overwrite_ok
    again = Pipeline(options=PipelineOptions(num_frames=n, background_only=True), background_mesh_options=bg_options, webxr_options=webxr)
    with pytest.raises(FileExistsError):
        again.run(hive, str(tmp_path / "again"), export_gltf=True)
    again.storage_options = StorageOptions(hive, str(tmp_path / "again"), overwrite_ok=True)
    again.run(compress=False, export_gltf=True)
    with open(tmp_path / "again" / "mesh" / "bg.glb", "rb") as f:
        doc, _ = R.check_container(f.read())
    assert "extensionsRequired" not in doc and len(doc["nodes"]) == 2
    empty = gltf.read_glb(str(tmp_path / "again" / "mesh" / "fg.glb"))
    assert empty.is_empty
    # the command line: --export_gltf
    from hive_amd.pipeline import main
    main(["--dataset_path", hive, "--output_path", str(tmp_path / "cli"), "--export_gltf", "--overwrite_ok", "--background_only", "--num_frames", str(n),
          "--sdf_voxel_size", "0.04", "--sdf_max_voxels", "1000000", "--key_frame_threshold", "0.9", "--key_frame_step", "2", "--webxr_path",
          str(tmp_path / "player" / "video")])
    assert {"fg.glb", "bg.glb", "metadata.json"} <= set(os.listdir(tmp_path / "cli" / "mesh"))
    with open(tmp_path / "cli" / "mesh" / "bg.glb", "rb") as a, open(export_dir / "bg.glb", "rb") as b:
        blob = a.read()
        assert blob == b.read(), "the export folder now holds this run's file"
    assert R.check_container(blob)[0]["extensionsRequired"] == ["KHR_mesh_quantization"]
    assert os.path.getsize(tmp_path / "again" / "mesh" / "bg.glb") == record["background"]["uncompressed_file_size"], "the plain file of the same background"
