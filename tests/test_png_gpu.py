"""PNG on the GPU: ``hive_amd.png.encode`` (csrc/png.hip) byte for byte against the numpy restatement (tests/png_restatement.py, which tests/test_png_cpu.py
reads back with zlib and Pillow) on every case of tests/png_cases.py; batches of mixed kinds in either order, repeats and row-pitched views; the bounds of
the output buffer; and the three callers with ``png_encoder="gpu"`` against their default.  No test here provokes a fault: what is refused is refused on the
host, before any launch."""
import io
import os

import numpy as np
import pytest

import png_cases as C
import png_restatement as R

pytestmark = pytest.mark.gpu


def _device(picture):
    import torch
    return torch.from_numpy(np.array(picture)).cuda()


def _decoded(data):
    from PIL import Image
    image = Image.open(io.BytesIO(data))
    image.load()
    return image.mode, np.array(image)


def test_bytes_equal_the_restatement(gpu_ctx):
    """Every case alone, the 480 x 640 depth map among them (76 segments, 300 sort tiles)."""
    from hive_amd import png
    for content, kind in C.cases():
        want = C.restated(content, kind)[0]
        got = png.encode(_device(C.picture(content, kind)), ctx=gpu_ctx)
        assert isinstance(got, bytes) and len(got) == len(want) and got == want, (content, kind, len(got), len(want))


def test_the_long_picture_is_the_recorded_file(gpu_ctx):
    """257 segments and 1025 sort tiles in one picture: the second chunk of the picture's scan and of the sort's.  The restatement's file is recorded
    (tests/png_cases.py, checked on the CPU); a wrong segment offset, CRC or Adler sum also fails the decode.  Alone, and behind a 1 x 7 (first_seg = 1)."""
    import hashlib
    from hive_amd import png
    picture = C.long_picture()
    long = _device(picture)
    alone = png.encode(long, ctx=gpu_ctx)
    small, second = png.encode([_device(C.picture("1x7", "gray8")), long], ctx=gpu_ctx)
    assert small == C.restated("1x7", "gray8")[0]
    for data in (alone, second):
        assert {"length": len(data), "sha256": hashlib.sha256(data).hexdigest()} == C.LONG_RECORD
        mode, pixels = _decoded(data)
        assert mode == "L" and np.array_equal(pixels, picture)


def test_a_mixed_batch_equals_each_alone_in_either_order_and_runs_repeat(gpu_ctx):
    from hive_amd import png
    cases = C.cases(with_large=False)
    pictures = [_device(C.picture(*case)) for case in cases]
    want = [C.restated(*case)[0] for case in cases]
    batch = png.encode(pictures, ctx=gpu_ctx)
    assert isinstance(batch, list) and batch == want
    assert png.encode(pictures[::-1], ctx=gpu_ctx) == want[::-1]
    assert png.encode(pictures, ctx=gpu_ctx) == want, "a second run"
    # host arrays are uploaded as they are
    assert png.encode([np.array(C.picture(*case)) for case in cases[:9]], ctx=gpu_ctx) == want[:9]


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_row_pitched_view_equals_its_contiguous_copy(gpu_ctx, kind):
    from hive_amd import png
    host = np.array(C.picture("noise", kind))
    host[3:30, 5:105] = C.picture("ramp", kind)[10:37, 20:120]   # a compressible patch inside the noise
    big = _device(host)
    view = big[2:33, 4:150]
    assert not view.is_contiguous() and view.stride(0) == big.stride(0)
    packed, offsets, sizes = png.encode_to_device([view, big], ctx=gpu_ctx)
    got = bytes(packed[offsets[0]:offsets[0] + sizes[0]].cpu().numpy())
    assert got == png.encode(view.contiguous(), ctx=gpu_ctx) == R.encode(view.cpu().numpy())
    assert bytes(packed[offsets[1]:offsets[1] + sizes[1]].cpu().numpy()) == R.encode(big.cpu().numpy())
    if kind == "rgb8":  # a view whose pixels are not contiguous (one channel dropped from RGBA) is copied, not misread
        import torch
        rgba = torch.cat([big, big[:, :, :1]], dim=2)
        assert png.encode(rgba[:, :, :3], ctx=gpu_ctx) == R.encode(big.cpu().numpy())


def test_the_output_buffer_is_respected(gpu_ctx):
    """64 guard bytes behind the layout's total stay as they were; a buffer one byte short is refused on the host, naming the size needed, and nothing is written."""
    import torch
    from hive_amd import _lib, png
    cases = [("noise", "gray16"), ("S+1", "gray8"), ("all_bytes", "gray8"), ("ramp", "rgb8")]
    pictures = [_device(C.picture(*case)) for case in cases]
    table = (_lib.PngImage * len(pictures))()
    for row, p, (_, kind) in zip(table, pictures, cases):
        row.pixels, row.height, row.width, row.pitch, row.kind = p.data_ptr(), p.shape[0], p.shape[1], p.stride(0) * p.element_size(), _lib.PNG_KIND[kind]
    host_sizes = np.zeros(len(pictures), np.int64)
    offsets, total = png.layout([(p.shape[:2], kind) for p, (_, kind) in zip(pictures, cases)])
    packed = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    gpu_ctx.check(gpu_ctx.lib.hive_png_encode(gpu_ctx.handle, table, len(pictures), packed.data_ptr(), total, _lib.ptr(host_sizes)))
    assert bool((packed[total:] == 0xA5).all()), "the guard bytes behind out_bytes"
    for case, offset, size in zip(cases, offsets, host_sizes):
        assert bytes(packed[offset:offset + size].cpu().numpy()) == C.restated(*case)[0]
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    host_sizes[:] = 0
    with pytest.raises(_lib.HiveError, match=rf"out_bytes = {total - 1} is too small: hive_png_layout asks for {total} bytes"):
        gpu_ctx.check(gpu_ctx.lib.hive_png_encode(gpu_ctx.handle, table, len(pictures), out.data_ptr(), total - 1, _lib.ptr(host_sizes)))
    table[1].pitch = pictures[1].shape[1] - 1
    with pytest.raises(_lib.HiveError, match="picture 1: a row pitch"):
        gpu_ctx.check(gpu_ctx.lib.hive_png_encode(gpu_ctx.handle, table, len(pictures), out.data_ptr(), total, _lib.ptr(host_sizes)))
    assert bool((out == 0xA5).all()) and not host_sizes.any()
    with pytest.raises(ValueError, match="picture 0"):
        png.encode(torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"), ctx=gpu_ctx)
    assert png.encode(pictures[0], ctx=gpu_ctx) == C.restated(*cases[0])[0], "the context still works"


def test_write_depth_pngs_files_read_back_as_the_host_encoders(gpu_ctx, tmp_path):
    """Three depth maps as ``forward_frames`` leaves them (the int16 view of uint16 millimetres, values past 32767 among them): the files of
    ``write_depth_pngs`` and of ``_write_png16`` give the dataset loader the same arrays, and are the restatement's bytes."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from hive_amd import depth
    from hive_amd.io import ImageFolderDataset
    maps = np.stack([np.array(C.picture("ramp_noise", "gray16")) + np.uint16(20000 * k) for k in range(3)])
    assert maps.dtype == np.uint16 and maps.max() > 40000
    gpu_dir, host_dir = tmp_path / "gpu", tmp_path / "host"
    os.makedirs(gpu_dir), os.makedirs(host_dir)
    names = [f"{k:06d}.png" for k in range(3)]
    on_device = torch.from_numpy(maps.view(np.int16)).cuda()
    assert depth.write_depth_pngs(on_device[:2], [str(gpu_dir / n) for n in names[:2]], ctx=gpu_ctx) == []
    with ThreadPoolExecutor(max_workers=2) as writers:
        for done in depth.write_depth_pngs(on_device[2:].view(torch.uint16), [str(gpu_dir / names[2])], ctx=gpu_ctx, writers=writers):
            done.result()
    for k, name in enumerate(names):
        depth._write_png16(str(host_dir / name), maps[k])
        with open(gpu_dir / name, "rb") as f:
            assert f.read() == R.encode(maps[k])
    ours, theirs = ImageFolderDataset(str(gpu_dir)), ImageFolderDataset(str(host_dir))
    assert len(ours) == len(theirs) == 3
    for k in range(3):
        a, b = np.asarray(ours[k]), np.asarray(theirs[k])
        assert a.dtype == b.dtype and np.array_equal(a, b) and np.array_equal(a, maps[k])
    with pytest.raises(ValueError, match="2 paths for 3 depth maps"):
        depth.write_depth_pngs(on_device, ["a", "b"], ctx=gpu_ctx)
    with pytest.raises(ValueError, match="png_encoder 'fast'"):
        depth.estimate_depth_dpt([], str(tmp_path / "none"), png_encoder="fast")


def _textured_scene():
    """Two textured quads with different atlases (one RGBA) and a coloured triangle, all on the host."""
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    quad = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1.5], [0, 1, 1.5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    first = np.array(C.picture("ramp", "rgb8"))
    second = np.dstack([np.array(C.picture("ramp_noise", "rgb8")), np.full((48, 64, 1), 255, np.uint8)])
    scene = gltf.Scene(camera=dict(resolution=(64, 48), focal=(60.0, 60.0)))
    scene.add_geometry({"vertices": quad, "faces": faces, "uv": uv, "texture": first}, node_name="000000")
    scene.add_geometry(Mesh(quad[:3] + np.float32(2.0), faces[:1], np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)), node_name="static")
    scene.add_geometry({"vertices": quad + np.float32(1.0), "faces": faces, "uv": uv, "texture": second}, node_name="000001")
    return scene, (first, second[:, :, :3])


@pytest.mark.parametrize("quantize", [False, True])
def test_write_glb_with_png_textures_from_the_gpu(gpu_ctx, tmp_path, quantize):
    from hive_amd import gltf
    scene, atlases = _textured_scene()
    host_path, gpu_path = str(tmp_path / "host.glb"), str(tmp_path / "gpu.glb")
    timings = {}
    host_sizes = gltf.write_glb(host_path, scene, quantize=quantize, ctx=gpu_ctx)
    gpu_sizes = gltf.write_glb(gpu_path, scene, quantize=quantize, png_encoder="gpu", ctx=gpu_ctx, timings=timings)
    assert "png" in timings and gpu_sizes["geometry"] == host_sizes["geometry"]
    with open(host_path, "rb") as f:
        host_doc, host_binary = gltf.split_glb(f.read())
    with open(gpu_path, "rb") as f:
        doc, binary = gltf.split_glb(f.read())
    n = host_sizes["geometry"]
    assert binary[:n] == host_binary[:n], "the geometry bytes"
    for key in ("accessors", "nodes", "meshes", "materials", "textures", "cameras", "scenes", "asset"):
        assert doc[key] == host_doc[key], key
    views = [binary[v["byteOffset"]:v["byteOffset"] + v["byteLength"]] for image in doc["images"] for v in [doc["bufferViews"][image["bufferView"]]]]
    assert [image["mimeType"] for image in doc["images"]] == ["image/png"] * 2 and views == [R.encode(a) for a in atlases]
    back, host_back = gltf.read_glb(gpu_path).meshes(), gltf.read_glb(host_path).meshes()
    for k, atlas in ((0, atlases[0]), (2, atlases[1])):
        assert np.array_equal(back[k]["texture"], atlas) and np.array_equal(host_back[k]["texture"], atlas)
        assert np.array_equal(back[k]["vertices"], host_back[k]["vertices"]) and np.array_equal(back[k]["faces"], host_back[k]["faces"])
    # the default is today's file
    default_path = str(tmp_path / "default.glb")
    gltf.write_glb(default_path, scene, quantize=quantize, ctx=gpu_ctx)
    with open(default_path, "rb") as a, open(host_path, "rb") as b:
        assert a.read() == b.read()
    with pytest.raises(ValueError, match="png_encoder 'device'"):
        gltf.write_glb(default_path, scene, png_encoder="device")


def _write_hive_folder(path, color, depth_mm, masks, K, poses_c2w):
    from PIL import Image
    from hive_amd import synthetic
    from hive_amd.io import DatasetMetadata, HiveDataset
    n, H, W = masks.shape
    for folder in HiveDataset.required_folders:
        os.makedirs(os.path.join(path, folder))
    for i in range(n):
        for folder, array in (("rgb", color[i]), ("depth", depth_mm[i]), ("mask", masks[i])):
            Image.fromarray(array).save(os.path.join(path, folder, f"{i:06d}.png"))
    DatasetMetadata(num_frames=n, fps=30.0, width=W, height=H).save(os.path.join(path, HiveDataset.metadata_filename))
    np.savetxt(os.path.join(path, HiveDataset.camera_matrix_filename), K)
    np.savetxt(os.path.join(path, HiveDataset.camera_trajectory_filename), synthetic.trajectory_rows_world_to_cam(poses_c2w))


def test_inpaint_frame_data_with_the_gpu_encoder_decodes_to_the_default(gpu_ctx, tmp_path):
    """The 48 x 64 folder of tests/test_inpaint_gpu.py (its first 5 frames, batches of 3 + 2): every file of the three inpainted folders decodes to the default
    run's pixels and mode, and is the restatement's file of those pixels."""
    import shutil
    from hive_amd import synthetic
    from hive_amd.dataset_adaptors import inpaint_frame_data
    from hive_amd.options import InpaintingMode
    seq = synthetic.make_sequence(num_frames=5, height=48, width=64, yaw_step_deg=20.0)
    masks = synthetic.ellipse_masks(5, 48, 64, num_objects=2)
    host, gpu = str(tmp_path / "host"), str(tmp_path / "gpu")
    _write_hive_folder(host, seq["color"], (seq["depth"] * 1000.0).astype(np.uint16), masks, seq["K"], seq["poses"])
    shutil.copytree(host, gpu)
    inpaint_frame_data(host, InpaintingMode.CV2_Image_Depth, batch_size=3)
    inpaint_frame_data(gpu, InpaintingMode.CV2_Image_Depth, batch_size=3, png_encoder="gpu")
    for folder in ("rgb_inpainted", "depth_inpainted", "mask_inpainted"):
        names = sorted(os.listdir(os.path.join(host, folder)))
        assert names == sorted(os.listdir(os.path.join(gpu, folder))) and len(names) == 5
        for name in names:
            with open(os.path.join(host, folder, name), "rb") as a, open(os.path.join(gpu, folder, name), "rb") as b:
                (host_mode, host_pixels), data = _decoded(a.read()), b.read()
            mode, pixels = _decoded(data)
            assert mode == host_mode and pixels.dtype == host_pixels.dtype and np.array_equal(pixels, host_pixels), (folder, name)
            assert data == R.encode(host_pixels.astype(np.uint16) if mode == "I;16" else host_pixels), (folder, name)
    with pytest.raises(ValueError, match="png_encoder 'pillow'"):
        inpaint_frame_data(gpu, InpaintingMode.CV2_Image_Depth, png_encoder="pillow")
