"""Baseline JPEG on the GPU: ``hive_amd.jpeg.encode`` (csrc/jpeg.hip) byte for byte against the numpy restatement (tests/jpeg_restatement.py, which
tests/test_jpeg_cpu.py pins against Pillow) over every size, quality, content and subsampling of tests/jpeg_cases.py; batches, repeats and row-pitched views;
the bounds of the output buffer; ``write_glb(texture_format="jpeg")`` and ``Pipeline.run`` with it.  No test here provokes a fault: what is refused is refused on
the host, before any launch."""
import io
import json
import os
import warnings

import numpy as np
import pytest

import jpeg_cases as C
import jpeg_restatement as R

pytestmark = pytest.mark.gpu


def _device(picture):
    import torch
    return torch.from_numpy(np.array(picture)).cuda()


def _opens_without_warning(data, height, width):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(data))
        image.load()
    assert image.format == "JPEG" and image.size == (width, height) and image.mode == "RGB"
    return np.array(image)


@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", C.QUALITIES)
def test_bytes_equal_the_restatement(gpu_ctx, quality, subsampling):
    """Every picture alone.  16 x 2064: 129 MCUs in one interval; 1040 x 16: 65 or 130 intervals; at quality 90 one 480 x 640 picture more (several workgroups of
    every kernel, the scan over 30 or 60 intervals).  Pillow opens every file without a warning (its only use here)."""
    from hive_amd import jpeg
    for height, width, content in C.cases(with_large=quality == 90):
        want = C.restated(height, width, content, quality, subsampling)[0]
        got = jpeg.encode(_device(C.picture(height, width, content)), quality, subsampling, ctx=gpu_ctx)
        assert isinstance(got, bytes) and got == want, (height, width, content, quality, subsampling, len(got), len(want))
        _opens_without_warning(got, height, width)


@pytest.mark.parametrize("case", C.LONG)
def test_bytes_equal_the_restatement_past_256_intervals(gpu_ctx, case):
    """257 MCU rows: the picture scan's second chunk of 256 intervals, alone and as the middle picture of three (its first interval is not the call's first)."""
    from hive_amd import jpeg
    quality, subsampling = case[3:]
    want = C.restated(*case)[0]
    long = _device(C.picture(*case[:3]))
    assert jpeg.encode(long, quality, subsampling, ctx=gpu_ctx) == want
    around = [(9, 17, "noise"), (24, 40, "gradient_noise")]
    batch = jpeg.encode([_device(C.picture(*around[0])), long, _device(C.picture(*around[1]))], quality, subsampling, ctx=gpu_ctx)
    assert batch == [C.restated(*around[0], quality, subsampling)[0], want, C.restated(*around[1], quality, subsampling)[0]]


@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
def test_a_batch_equals_each_alone_in_either_order_and_runs_repeat(gpu_ctx, subsampling):
    from hive_amd import jpeg
    cases = [(h, w, C.CONTENTS[k % len(C.CONTENTS)]) for k, (h, w) in enumerate(C.SIZES + (C.LARGE,))]
    pictures = [_device(C.picture(*case)) for case in cases]
    alone = [jpeg.encode(p, 90, subsampling, ctx=gpu_ctx) for p in pictures]
    assert alone == [C.restated(*case, 90, subsampling)[0] for case in cases]
    batch = jpeg.encode(pictures, 90, subsampling, ctx=gpu_ctx)
    assert isinstance(batch, list) and batch == alone
    assert jpeg.encode(pictures[::-1], 90, subsampling, ctx=gpu_ctx) == alone[::-1]
    assert jpeg.encode(pictures, 90, subsampling, ctx=gpu_ctx) == alone, "a second run"
    # host arrays are uploaded as they are
    assert jpeg.encode([np.array(C.picture(*case)) for case in cases[:4]], 90, subsampling, ctx=gpu_ctx) == alone[:4]


def test_a_row_pitched_view_equals_its_contiguous_copy(gpu_ctx):
    import torch
    from hive_amd import jpeg
    big = _device(C.picture(100, 150, "noise"))
    view = big[5:62, 7:138]  # 57 x 131 inside 100 x 150: rows 450 bytes apart, the first pixel 5 * 450 + 21 bytes in
    assert not view.is_contiguous() and view.stride() == (450, 3, 1)
    packed, offsets, sizes = jpeg.encode_to_device([view, big], 90, "4:2:0", ctx=gpu_ctx)
    got = bytes(packed[offsets[0]:offsets[0] + sizes[0]].cpu().numpy())
    assert got == jpeg.encode(view.contiguous(), 90, "4:2:0", ctx=gpu_ctx) == R.encode(view.cpu().numpy(), 90, "4:2:0")
    assert bytes(packed[offsets[1]:offsets[1] + sizes[1]].cpu().numpy()) == C.restated(100, 150, "noise", 90, "4:2:0")[0]
    # a view whose pixels are not contiguous (one channel dropped from RGBA) is copied, not misread
    rgba = torch.cat([big, big[:, :, :1]], dim=2)
    assert jpeg.encode(rgba[:, :, :3], 90, "4:4:4", ctx=gpu_ctx) == C.restated(100, 150, "noise", 90, "4:4:4")[0]


def test_the_output_buffer_is_respected(gpu_ctx):
    """64 guard bytes behind the layout's total stay as they were; a buffer one byte short is refused on the host, naming the size needed, and nothing is written."""
    import torch
    from hive_amd import _lib, jpeg
    cases = [(37, 61, "noise"), (16, 2064, "noise"), (1040, 16, "blocks")]
    pictures = [_device(C.picture(*case)) for case in cases]
    table = (_lib.JpegImage * len(pictures))()
    for row, p in zip(table, pictures):
        row.data, row.height, row.width, row.pitch = p.data_ptr(), p.shape[0], p.shape[1], p.stride(0)
    host_sizes = np.zeros(len(pictures), np.int64)
    for subsampling in C.SUBSAMPLINGS:
        offsets, total = jpeg.layout([p.shape[:2] for p in pictures], subsampling)
        packed = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        gpu_ctx.check(gpu_ctx.lib.hive_jpeg_encode(gpu_ctx.handle, table, len(pictures), 100, _lib.JPEG_SUBSAMPLING[subsampling], packed.data_ptr(), total,
                                                   _lib.ptr(host_sizes)))
        assert bool((packed[total:] == 0xA5).all()), "the guard bytes behind out_bytes"
        for case, offset, size in zip(cases, offsets, host_sizes):
            assert bytes(packed[offset:offset + size].cpu().numpy()) == C.restated(*case, 100, subsampling)[0]
    offsets, total = jpeg.layout([p.shape[:2] for p in pictures], "4:2:0")
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    host_sizes[:] = 0
    with pytest.raises(_lib.HiveError, match=rf"out_bytes = {total - 1} is too small: hive_jpeg_layout asks for {total} bytes"):
        gpu_ctx.check(gpu_ctx.lib.hive_jpeg_encode(gpu_ctx.handle, table, len(pictures), 100, 2, out.data_ptr(), total - 1, _lib.ptr(host_sizes)))
    assert bool((out == 0xA5).all()) and not host_sizes.any()
    for quality, code, word in ((0, 0, "quality 0 outside"), (101, 2, "quality 101 outside"), (90, 1, "unknown subsampling 1")):
        with pytest.raises(_lib.HiveError, match=word):
            gpu_ctx.check(gpu_ctx.lib.hive_jpeg_encode(gpu_ctx.handle, table, len(pictures), quality, code, out.data_ptr(), total, _lib.ptr(host_sizes)))
    table[1].pitch = 3 * 2064 - 1
    with pytest.raises(_lib.HiveError, match="picture 1: a row pitch"):
        gpu_ctx.check(gpu_ctx.lib.hive_jpeg_encode(gpu_ctx.handle, table, len(pictures), 90, 2, out.data_ptr(), total, _lib.ptr(host_sizes)))
    assert bool((out == 0xA5).all())
    assert jpeg.encode(pictures[0], 100, "4:4:4", ctx=gpu_ctx) == C.restated(*cases[0], 100, "4:4:4")[0], "the context still works"


@pytest.fixture(scope="module")
def textured_scene(gpu_ctx):
    """Two textured meshes (a ``process_frame`` dict of a 240 x 320 frame and a shifted copy with another atlas) and a coloured ``Mesh``, with their camera."""
    import torch
    from hive_amd import foreground, gltf, synthetic
    from hive_amd.mesh import Mesh
    from hive_amd.options import MaskDilationOptions, MeshFilteringOptions
    H, W = 240, 320
    seq = synthetic.make_sequence(num_frames=1, height=H, width=W)
    ids = synthetic.ellipse_masks(1, H, W, num_objects=2, seed=3)[0].copy()
    ids[seq["depth"][0] == 0] = 0
    pose = np.linalg.inv(seq["poses"][0])
    frame = foreground.process_frame(torch.from_numpy(seq["color"][0]).cuda(), torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(ids).cuda(), seq["K"], pose,
                                     MaskDilationOptions(num_iterations=0), MeshFilteringOptions(), ctx=gpu_ctx, enable_cc_analysis=True)
    first = {key: frame[key] for key in ("vertices", "faces", "uv", "texture")}
    second = dict(first, vertices=first["vertices"] + torch.tensor([0.0, 0.3, 0.0], dtype=first["vertices"].dtype, device="cuda"),
                  texture=torch.flip(first["texture"], dims=(0,))[: first["texture"].shape[0] - 3, : first["texture"].shape[1] - 5].contiguous())
    rng = np.random.default_rng(8)
    v = first["vertices"].cpu().numpy() + (seq["poses"][0][:3, :3] @ np.array([0.4, 0.0, 0.1]))
    coloured = Mesh(v, first["faces"].cpu().numpy().astype(np.int32), rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
    scene = gltf.Scene(camera=dict(resolution=(W, H), focal=(seq["K"][0, 0], seq["K"][1, 1])))
    scene.add_geometry(first, node_name="000000")
    scene.add_geometry(coloured, node_name="static")
    scene.add_geometry(second, node_name="000001")
    return scene, (first, second), seq["K"], pose, (H, W)


def _image_views(doc, binary):
    return [(image["mimeType"], binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]) for image in doc.get("images", [])
            for view in [doc["bufferViews"][image["bufferView"]]]]


@pytest.mark.parametrize("quantize", [False, True])
def test_write_glb_with_jpeg_textures(gpu_ctx, tmp_path, textured_scene, quantize):
    from PIL import Image
    from hive_amd import gltf, jpeg, render
    scene, textured, K, pose, size = textured_scene
    png_path, jpeg_path = str(tmp_path / "png.glb"), str(tmp_path / "jpeg.glb")
    timings = {}
    png_sizes = gltf.write_glb(png_path, scene, quantize=quantize)
    jpeg_sizes = gltf.write_glb(jpeg_path, scene, quantize=quantize, texture_format="jpeg", jpeg_quality=75, jpeg_subsampling="4:4:4", timings=timings)
    assert "jpeg" in timings and "png" not in timings
    with open(png_path, "rb") as f:
        png_doc, png_binary = gltf.split_glb(f.read())
    with open(jpeg_path, "rb") as f:
        blob = f.read()
        doc, binary = gltf.split_glb(blob)
    assert jpeg_sizes["total"] == len(blob) and jpeg_sizes["geometry"] == png_sizes["geometry"]
    # the image views hold exactly the encoder's files, which are the restatement's
    atlases = [m["texture"][:, :, :3].contiguous() for m in textured]
    files = jpeg.encode(atlases, 75, "4:4:4", ctx=gpu_ctx)
    assert files == [R.encode(a.cpu().numpy(), 75, "4:4:4") for a in atlases]
    assert _image_views(doc, binary) == [("image/jpeg", f) for f in files]
    assert [mime for mime, _ in _image_views(png_doc, png_binary)] == ["image/png"] * 2
    assert all(doc["bufferViews"][image["bufferView"]]["byteOffset"] % 4 == 0 for image in doc["images"])
    # everything but the images is the PNG file's: geometry bytes, accessors (with their bounds), nodes, meshes, materials, the geometry's views
    n = png_sizes["geometry"]
    assert binary[:n] == png_binary[:n]
    for key in ("accessors", "nodes", "meshes", "materials", "textures", "cameras", "scenes", "asset"):
        assert doc[key] == png_doc[key], key
    assert doc.get("extensionsRequired") == png_doc.get("extensionsRequired") == (["KHR_mesh_quantization"] if quantize else None)
    geometry_views = len(doc["bufferViews"]) - len(doc["images"])
    assert doc["bufferViews"][:geometry_views] == png_doc["bufferViews"][:geometry_views]
    # read back: the textures are Pillow's decode of the restatement's bytes, and the scene renders
    back = gltf.read_glb(jpeg_path)
    assert list(back.geometry) == ["000000", "static", "000001"]
    meshes = back.meshes()
    for mesh, data, atlas in zip((meshes[0], meshes[2]), files, atlases):
        assert np.array_equal(mesh["texture"], np.array(Image.open(io.BytesIO(data)).convert("RGB")))
        assert mesh["texture"].shape == tuple(atlas.shape)
    picture = render.render_mesh(K, pose, *back.meshes(apply_transform=False), size=size, ctx=gpu_ctx)
    assert tuple(picture.shape[:2]) == size and (picture.cpu().numpy() != 255).any(axis=2).mean() > 0.02, "the meshes are in view"
    # the default is today's file
    default_path = str(tmp_path / "default.glb")
    gltf.write_glb(default_path, scene, quantize=quantize)
    with open(default_path, "rb") as a, open(png_path, "rb") as b:
        assert a.read() == b.read()


def test_pipeline_run_exports_jpeg_textures(gpu_ctx, tmp_path):
    """``run(export_gltf=True)`` with ``texture_format="jpeg"`` on the TUM-layout fixture (built as tests/test_gltf_gpu.py builds it): every image of fg.glb is a
    JPEG that is the encoder's file of that frame's atlas, the quantised rewrite keeps the format, bg.glb (no texture) is byte for byte the PNG run's, node names
    and metadata.json are unchanged, the per-frame PNG files stay PNG."""
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
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.04, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)
    docs = {}
    for fmt in ("png", "jpeg"):
        webxr = WebXROptions(webxr_path=str(tmp_path / f"player_{fmt}" / "video"))
        options = PipelineOptions(num_frames=n, texture_format=fmt, jpeg_quality=80) if fmt == "jpeg" else PipelineOptions(num_frames=n)
        pipe = Pipeline(options=options, background_mesh_options=bg_options, webxr_options=webxr)
        pipe.run(hive, str(tmp_path / fmt), export_gltf=True)
        with open(tmp_path / fmt / "mesh" / "fg.glb", "rb") as f:
            docs[fmt] = gltf.split_glb(f.read())
        assert pipe.profiling["mesh_compression"]["foreground"]["compressed_file_size"] == os.path.getsize(tmp_path / fmt / "mesh" / "fg.glb")
    (png_doc, png_binary), (doc, binary) = docs["png"], docs["jpeg"]
    assert doc["extensionsRequired"] == ["KHR_mesh_quantization"], "the quantised rewrite replaced the plain file and kept image/jpeg"
    views, png_views = _image_views(doc, binary), _image_views(png_doc, png_binary)
    assert len(views) == len(png_views) > 0 and all(mime == "image/jpeg" and data[:3] == b"\xFF\xD8\xFF" for mime, data in views)
    assert all(mime == "image/png" for mime, _ in png_views)
    names = [doc["nodes"][c]["name"] for c in doc["nodes"][0]["children"]]
    assert names == [png_doc["nodes"][c]["name"] for c in png_doc["nodes"][0]["children"]] and doc["nodes"] == png_doc["nodes"] and doc["accessors"] == png_doc["accessors"]
    for name, (_, data) in zip(names, views):  # a frame's image is the file of that frame's PNG atlas at the pipeline's settings
        atlas = np.asarray(Image.open(tmp_path / "jpeg" / "mesh" / "fg" / f"{name}.png").convert("RGB"))
        assert data == R.encode(atlas, 80, "4:2:0"), name
    for name in ("bg.glb", "metadata.json"):
        with open(tmp_path / "png" / "mesh" / name, "rb") as a, open(tmp_path / "jpeg" / "mesh" / name, "rb") as b:
            assert a.read() == b.read(), name
    with open(tmp_path / "jpeg" / "mesh" / "metadata.json") as f:
        assert set(json.load(f)) == {"fps", "fov_y", "num_frames", "use_vertex_colour_for_bg", "add_ground_plane", "add_sky_box"}
    for name in sorted(os.listdir(tmp_path / "jpeg" / "mesh" / "fg")):
        with open(tmp_path / "png" / "mesh" / "fg" / name, "rb") as a, open(tmp_path / "jpeg" / "mesh" / "fg" / name, "rb") as b:
            data = b.read()
            assert a.read() == data and (not name.endswith(".png") or data[:8] == b"\x89PNG\r\n\x1a\n"), name
    back = gltf.read_glb(str(tmp_path / "jpeg" / "mesh" / "fg.glb"))
    assert list(back.geometry) == names and all(m["texture"].ndim == 3 for m in back.meshes())
    with open(tmp_path / "player_jpeg" / "video" / "hive" / "fg.glb", "rb") as a, open(tmp_path / "jpeg" / "mesh" / "fg.glb", "rb") as b:
        assert a.read() == b.read(), "the exported file is the JPEG-textured one"
