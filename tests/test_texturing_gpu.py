"""csrc/texture.hip against tests/texturing_restatement.py, bit for bit: labels, unwelded geometry, uv and every atlas byte, on the CPU file's known answers,
random triangle soups, and the fused 32^3 room; the renderer and the glTF writer take the result; the pipeline switch."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gltf_restatement as GR  # noqa: E402
import render_restatement as RR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("vertices", "faces", "uv", "texture", "views")


def native(ctx, mesh, frames, poses, masks=None, device_inputs=False, **kw):
    import torch
    from hive_amd import texturing
    if device_inputs:
        mesh = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mesh.items()}
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        masks = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    out = texturing.texture_mesh(mesh, frames, C.K, poses, masks=masks, ctx=ctx, return_views=True, **kw)
    assert out["vertices"].dtype == torch.float64 and out["faces"].dtype == torch.int32 and out["uv"].dtype == torch.float64 and out["texture"].dtype == torch.uint8
    assert all(out[k].is_cuda for k in KEYS)
    return {k: out[k].cpu().numpy() for k in KEYS}


def same(got, want, what=""):
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k} differs"


def check_case(ctx, mesh, frames, poses, masks=None, ties=False, **kw):
    """Alone, on a second run, with host and device inputs, and with the views passed in reverse order; returns the restatement's result.  ``ties``: two views
    see a face with the same area, so the lower index wins and a reversal legitimately moves the label: the reversed run is compared with the restatement of
    the reversed inputs instead."""
    want = TR.texture_mesh(mesh, frames, C.K, poses, masks=masks, **kw)
    same(native(ctx, mesh, frames, poses, masks, **kw), want, "first run")
    same(native(ctx, mesh, frames, poses, masks, **kw), want, "second run")
    same(native(ctx, mesh, frames, poses, masks, device_inputs=True, **kw), want, "device inputs")
    n = len(poses)
    if n > 1:
        back = native(ctx, mesh, frames[::-1], poses[::-1], None if masks is None else masks[::-1], **kw)
        if ties:
            same(back, TR.texture_mesh(mesh, frames[::-1], C.K, poses[::-1], masks=None if masks is None else masks[::-1], **kw), "reversed inputs")
            return want
        assert np.array_equal(C.reverse_labels(back["views"], n), want["views"]), "the labels map through the reversal"
        assert np.array_equal(back["texture"], want["texture"]) and np.array_equal(back["uv"], want["uv"])
    return want


@pytest.mark.parametrize("S", [6, 7, 9, 13])
def test_the_closed_form_quad(gpu_ctx, S):
    want = check_case(gpu_ctx, C.quad(*C.QUAD_CORNERS), C.ramp_frame()[None], C.IDENTITY[None], cell=S)
    assert want["views"].tolist() == [0, 0]


@pytest.mark.parametrize("gap, labels", C.TWO_QUAD_LABELS)
def test_selection_two_parallel_quads(gpu_ctx, gap, labels):
    mesh, poses = C.two_quads(gap)
    want = check_case(gpu_ctx, mesh, C.frames_for(2), poses, depth_tolerance=C.TOLERANCE)
    assert want["views"].tolist() == labels, "the labels worked out by hand"


def test_selection_ties_masks_near_and_screen(gpu_ctx):
    mesh, frames = C.quad(*C.QUAD_CORNERS), C.frames_for(2, 1)
    two = np.stack([C.IDENTITY, C.IDENTITY])
    assert native(gpu_ctx, mesh, frames, two)["views"].tolist() == [0, 0], "identical poses: the lower index"
    masks = np.zeros((2, C.H, C.W), np.uint8)
    masks[0, 22, 31] = 7
    assert check_case(gpu_ctx, mesh, frames, two, masks, ties=True)["views"].tolist() == [1, 0]
    behind = C.quad(*C.QUAD_CORNERS)
    behind["vertices"][0, 2] = 0.01
    assert check_case(gpu_ctx, behind, frames[:1], C.IDENTITY[None])["views"].tolist() == [-1, 0]
    assert check_case(gpu_ctx, C.quad(60.0, 63.6, 10.0, 14.0), frames[:1], C.IDENTITY[None])["views"].tolist() == [-1, -1]
    assert check_case(gpu_ctx, C.quad(60.0, 63.4, 10.0, 14.0), frames[:1], C.IDENTITY[None])["views"].tolist() == [0, 0]


def test_a_mesh_no_view_sees_takes_its_vertex_colours(gpu_ctx):
    away = np.diag([-1.0, 1.0, -1.0, 1.0])
    mesh = C.quad(*C.QUAD_CORNERS, colour=(10, 200, 90))
    got = native(gpu_ctx, mesh, C.ramp_frame()[None], away[None])
    assert got["views"].tolist() == [-1, -1] and (got["texture"] == np.array([10, 200, 90], np.uint8)).all()
    mesh["vertex_colors"] = np.array([[0, 0, 0, 255], [255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], np.uint8)  # (alpha is dropped)
    check_case(gpu_ctx, dict(mesh, faces=mesh["faces"][:1]), C.ramp_frame()[None], away[None])


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("n", C.SOUP_VIEWS)
@pytest.mark.parametrize("cell", C.SOUP_CELLS)
@pytest.mark.parametrize("nf", C.SOUP_FACES)
def test_triangle_soups(gpu_ctx, nf, cell, n, with_masks):
    case = C.soup_case(nf, cell, n, with_masks)
    want = check_case(gpu_ctx, case["mesh"], case["frames"], case["poses"], case["masks"], cell=cell)
    if nf >= 255:
        assert (want["views"] >= 0).any() and (want["views"] < 0).any(), "both fills are exercised"


@pytest.fixture(scope="module")
def textured_room(gpu_ctx):
    mesh, seq, w2c = C.room()
    frames, poses = seq["color"][[0, 2]], w2c[[0, 2]]
    want = TR.texture_mesh(mesh, frames, seq["K"].astype(np.float64), poses)
    return mesh, seq, w2c, frames, poses, want


def test_the_fused_room(gpu_ctx, textured_room):
    import torch
    from hive_amd import texturing
    mesh, seq, w2c, frames, poses, want = textured_room
    for k in range(2):
        out = texturing.texture_mesh(mesh, frames, seq["K"], poses, ctx=gpu_ctx, return_views=True)
        same({key: out[key].cpu().numpy() for key in KEYS}, want, f"run {k}")
    back = texturing.texture_mesh({k: torch.from_numpy(v).cuda() for k, v in mesh.items()}, torch.from_numpy(frames[::-1].copy()).cuda(), seq["K"], poses[::-1],
                                  ctx=gpu_ctx, return_views=True)
    assert np.array_equal(C.reverse_labels(back["views"].cpu().numpy(), 2), want["views"]) and np.array_equal(back["texture"].cpu().numpy(), want["texture"])
    assert (want["views"] >= 0).mean() > 0.5
    assert set(texturing.texture_mesh(mesh, frames, seq["K"], poses, ctx=gpu_ctx)) == {"vertices", "faces", "uv", "texture"}


def test_render_mesh_takes_the_result(gpu_ctx, textured_room):
    from hive_amd import render, texturing
    mesh, seq, w2c, frames, poses, want = textured_room
    out = texturing.texture_mesh(mesh, frames, seq["K"], poses, ctx=gpu_ctx)
    K = seq["K"].astype(np.float64)
    picture, depth, face = render.render_mesh(K, w2c[1], out, size=(C.H, C.W), return_depth=True, return_faces=True, ctx=gpu_ctx)
    color, d, f, _ = RR.render([{k: want[k] for k in ("vertices", "faces", "uv", "texture")}], K, w2c[1][:3, :3], w2c[1][:3, 3], C.H, C.W)
    assert (f >= 0).mean() > 0.8
    assert np.array_equal(picture.cpu().numpy(), color) and np.array_equal(depth.cpu().numpy(), d) and np.array_equal(face.cpu().numpy(), f)


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("wide", [False, True])
def test_write_then_read_glb(gpu_ctx, tmp_path, textured_room, quantize, wide):
    """Plain and quantised, with 3 nf <= 65535 (the room: uint16 indices when quantised) and above (a soup of 22 000 faces: uint32 indices either way)."""
    from hive_amd import gltf, texturing
    if wide:
        mesh = C.soup(22000, 5)
        out = texturing.texture_mesh(mesh, C.frames_for(1, 5), C.K, C.IDENTITY[None], cell=6, ctx=gpu_ctx)
    else:
        mesh, seq, w2c, frames, poses, want = textured_room
        out = texturing.texture_mesh(mesh, frames, seq["K"], poses, ctx=gpu_ctx)
    V = out["vertices"].shape[0]
    assert (V > 65535) == wide and V == 3 * len(mesh["faces"])
    scene = gltf.Scene()
    scene.add_geometry(out, node_name="000000")
    path = str(tmp_path / "bg.glb")
    gltf.write_glb(path, scene, quantize=quantize)
    with open(path, "rb") as f:
        doc, _ = GR.check_container(f.read())
    primitive = doc["meshes"][0]["primitives"][0]
    assert set(primitive["attributes"]) == {"POSITION", "TEXCOORD_0"} and len(doc["images"]) == 1 and doc["images"][0]["mimeType"] == "image/png"
    assert doc["accessors"][primitive["indices"]]["componentType"] == (gltf.UNSIGNED_SHORT if quantize and not wide else gltf.UNSIGNED_INT)
    assert doc["accessors"][primitive["attributes"]["POSITION"]]["count"] == V
    back = gltf.read_glb(path).meshes()[0]
    v, uv = out["vertices"].cpu().numpy(), out["uv"].cpu().numpy()
    assert np.array_equal(back["faces"], out["faces"].cpu().numpy()) and np.array_equal(back["texture"], out["texture"].cpu().numpy())
    if quantize:
        lo, hi = v.min(axis=0), v.max(axis=0)
        assert np.all(np.abs(back["vertices"] - v) <= GR.step_of(lo, hi) / 2 + 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi))))
        assert np.all(np.abs(back["uv"] - uv) <= 0.5 / 65535.0 + 2 * np.spacing(1.0))
    else:
        assert np.array_equal(back["vertices"], v.astype(np.float32).astype(np.float64))
        stored = GR.texcoords(uv).astype(np.float32)
        assert np.array_equal(back["uv"], np.stack([stored[:, 0].astype(np.float64), 1.0 - stored[:, 1].astype(np.float64)], axis=1))
    # either way every corner still lands on its own texel under the renderer's nearest-texel rule
    ht, wt = back["texture"].shape[:2]
    nearest = lambda a: (np.clip(np.floor(a[:, 0] * wt + 0.5), 0, wt - 1), np.clip(np.floor((1.0 - a[:, 1]) * ht + 0.5), 0, ht - 1))
    assert np.array_equal(nearest(back["uv"])[0], nearest(uv)[0]) and np.array_equal(nearest(back["uv"])[1], nearest(uv)[1])


def test_pipeline_switch(gpu_ctx, tmp_path):
    """``run(export_gltf=True)`` with ``texture_background``: bg.glb's one mesh has uv and one image and no colours, metadata says so, bg.ply and the foreground
    are untouched; two runs with the switch off write the same bytes, with the structure tests/test_gltf_gpu.py expects of the vertex-coloured file."""
    from PIL import Image
    from hive_amd import gltf, synthetic
    from hive_amd.dataset_adaptors import get_dataset
    from hive_amd.options import BackgroundMeshOptions, PipelineOptions, WebXROptions
    from hive_amd.pipeline import Pipeline
    from tum_fixture import write_tum_sequence
    tum, hive = str(tmp_path / "tum"), str(tmp_path / "hive")
    n = 3
    write_tum_sequence(tum, num_frames=n, yaw_step_deg=10.0)
    ds = get_dataset(tum, hive)
    masks = synthetic.ellipse_masks(n, ds.frame_height, ds.frame_width, num_objects=3, seed=5)
    for name, m in zip(sorted(os.listdir(os.path.join(hive, "mask"))), masks):
        Image.fromarray(m).save(os.path.join(hive, "mask", name))
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.08, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)

    def run(name, compress=True, **switch):
        webxr = WebXROptions(webxr_path=str(tmp_path / f"player_{name}"))
        pipe = Pipeline(options=PipelineOptions(num_frames=n, **switch), background_mesh_options=bg_options, webxr_options=webxr)
        pipe.run(hive, str(tmp_path / name), compress, export_gltf=True)
        files = {}
        for f in ("bg.glb", "fg.glb", "metadata.json", "bg.ply"):
            with open(tmp_path / name / "mesh" / f, "rb") as handle:
                files[f] = handle.read()
        return pipe, files
    _, off_a = run("off_a")
    _, off_b = run("off_b")
    assert off_a == off_b, "the off path is deterministic"
    doc, _ = GR.check_container(off_a["bg.glb"])
    primitive = doc["meshes"][0]["primitives"][0]
    assert set(primitive["attributes"]) == {"POSITION", "COLOR_0"} and "images" not in doc and doc["extensionsRequired"] == ["KHR_mesh_quantization"]
    assert [doc["nodes"][c]["name"] for c in doc["nodes"][0]["children"]] == ["000000"]
    assert json.loads(off_a["metadata.json"])["use_vertex_colour_for_bg"] is True

    for compress in (True, False):
        pipe, on = run(f"on_{int(compress)}", compress, texture_background=True, texture_cell=6)
        assert on["bg.ply"] == off_a["bg.ply"] and (on["fg.glb"] == off_a["fg.glb"]) == compress, "bg.ply and the foreground are untouched"
        assert json.loads(on["metadata.json"]) == dict(json.loads(off_a["metadata.json"]), use_vertex_colour_for_bg=False)
        doc, _ = GR.check_container(on["bg.glb"])
        primitive = doc["meshes"][0]["primitives"][0]
        assert len(doc["meshes"]) == 1 and set(primitive["attributes"]) == {"POSITION", "TEXCOORD_0"} and len(doc["images"]) == 1 and "material" in primitive
        assert ("extensionsRequired" in doc) == compress
        record = pipe.profiling["background_texturing"]
        print(f"background texturing: {record}")
        # (how many faces find a view depends on the masks, the key frames and the 5 cm tolerance on an 8 cm mesh: an independent numpy emulation of this room
        # gives 41 % from frame 0 alone and 75 % from frames 0 and 2; no share is asserted, only that the frames were used at all)
        assert 0 < record["faces_with_a_view"] <= record["faces"] and 1 <= len(record["key_frames"]) <= 32
        back = gltf.read_glb(str(tmp_path / f"on_{int(compress)}" / "mesh" / "bg.glb"))
        mesh = back.meshes()[0]
        assert list(back.geometry) == ["000000"] and len(mesh["vertices"]) == 3 * len(mesh["faces"]) == 3 * record["faces"]
        assert mesh["texture"].shape[:2] == (record["atlas"][1], record["atlas"][0]) and mesh["texture"].any()
