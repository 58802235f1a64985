"""hive_inpaint_telea / hive_inpaint_frames against the numpy restatement of the header's specification (tests/inpaint_restatement.py),
bit for bit: image types, hole shapes at and away from the border, radii, both memory kinds, batching, the entry points, the errors, and
``inpaint_frame_data`` end to end."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def one_pixel(H=5, W=7):
    m = np.zeros((H, W), np.uint8)
    m[2, 4] = 1
    return m


def row_1x9():
    return np.array([[0, 1, 1, 0, 0, 1, 1, 1, 1]], np.uint8)  # the last run touches the border


def tiles_70x133():
    """More than one 64-wide tile each way, not a multiple: a large disc across the tile seams, a strip along the right border, a corner."""
    m = R.disc(70, 133, 36, 62, 17)
    m[5:20, 125:] = 1
    m[60:, 0:30] = 1
    m[3:6, 64:67] = 1
    return m


HOLES = {
    "interior": R.interior_holes,
    "border": R.border_holes,
    "one_pixel": one_pixel,
    "1x9": row_1x9,
    "9x1": lambda: np.ascontiguousarray(row_1x9().T),
    "all_borders": R.all_border_holes,
    "tiles": tiles_70x133,
}
KINDS = {"u8": (np.uint8, 1), "u8x3": (np.uint8, 3), "u16": (np.uint16, 1)}


@functools.lru_cache(maxsize=None)
def case(holes, kind, radius):
    """(image, mask, the restatement's result, its info), computed once per case and shared; nobody writes to them."""
    mask = HOLES[holes]()
    dtype, C = KINDS[kind]
    image = R.random_image(mask.shape[0], mask.shape[1], dtype, C, seed=len(holes) + radius)
    if kind == "u16":  # a depth map: a fifth of it has no reading
        image[np.random.default_rng(9).random(mask.shape) < 0.2] = 0
    info = {}
    expect = R.inpaint(image, mask, radius, info)
    for a in (image, mask, expect):
        a.setflags(write=False)
    return image, mask, expect, info


def run_both(image, mask, radius):
    """The host call and the device call."""
    import torch
    from hive_amd.image_processing import inpaint_telea
    host = inpaint_telea(image, mask, radius)
    device = inpaint_telea(torch.from_numpy(np.array(image)).cuda(), torch.from_numpy(np.array(mask)).cuda(), radius)
    assert isinstance(host, np.ndarray) and host.dtype == image.dtype and host.shape == image.shape
    return host, device.cpu().numpy()


# radius 30 clips the window at every border of a 48 x 64 image: one colour and one depth case
CASES = [(h, k, r) for h in HOLES for k in KINDS for r in (2, 5)] + [("interior", "u8x3", 30), ("border", "u16", 30)]


@pytest.mark.parametrize("holes,kind,radius", CASES)
def test_inpaint_telea_matches_restatement(gpu_ctx, holes, kind, radius):
    image, mask, expect, info = case(holes, kind, radius)
    assert info["min_weight_sum"] > 0.0
    host, device = run_both(image, mask, radius)
    for got in (host, device):
        differ = np.nonzero(got != expect)
        assert len(differ[0]) == 0, f"{len(differ[0])} values differ, first at {[int(d[0]) for d in differ]}: {got[differ][:4]} != {expect[differ][:4]}"
        assert np.array_equal(got[mask == 0], image[mask == 0])


@pytest.mark.parametrize("radius", [2, 5, 30])
def test_constant_and_ramp_come_back_exactly(gpu_ctx, radius):
    """The specification's fixed points, from the kernel's own output: on holes away from the border a constant and a non-wrapping integer ramp
    come back exactly, u8 and u16."""
    mask = R.interior_holes()
    for image in (R.ramp(48, 64, np.uint8), R.ramp(48, 64, np.uint8, 3), R.ramp(48, 64, np.uint16), np.full((48, 64), 201, np.uint8),
                  np.full((48, 64), 54321, np.uint16), np.zeros((48, 64), np.uint16)):
        host, device = run_both(image, mask, radius)
        assert np.array_equal(host, image) and np.array_equal(device, image)


def test_no_hole_is_a_copy(gpu_ctx):
    image = R.random_image(37, 53, np.uint8, 3, seed=2)
    host, device = run_both(image, np.zeros((37, 53), np.uint8), 5)
    assert np.array_equal(host, image) and np.array_equal(device, image)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def batch_frames():
    """Three 48 x 64 frames with 0, 12 and 23 levels, colour + depth."""
    masks = np.stack([np.zeros((48, 64), np.uint8), R.disc(48, 64, 24, 30, 11), R.disc(48, 64, 24, 31, 22)])
    rgb = np.stack([R.random_image(48, 64, np.uint8, 3, seed=20 + f) for f in range(3)])
    depth = np.stack([R.random_image(48, 64, np.uint16, seed=30 + f) for f in range(3)])
    depth[:, ::7, ::5] = 0
    return rgb, depth, masks


def test_batch_equals_single_calls_and_restatement(gpu_ctx):
    """One call over the batch == its frames one by one == two hive_inpaint_telea calls per frame == the restatement; levels_out too."""
    import torch
    from hive_amd.image_processing import inpaint_frames, inpaint_telea
    rgb, depth, masks = batch_frames()
    t_rgb, t_depth, t_masks = (torch.from_numpy(a).cuda() for a in (rgb, depth, masks))
    out_rgb, out_depth, levels = inpaint_frames(t_rgb, t_depth, t_masks, dilation=(5, 5, 0), radius=5, return_levels=True)
    info = {}
    expect_rgb, expect_depth = R.inpaint_batch([rgb, depth], masks, 5, info)
    assert levels.tolist() == info["level_count"].tolist() == [0, 12, 23]
    assert np.array_equal(out_rgb.cpu().numpy(), expect_rgb) and np.array_equal(out_depth.cpu().numpy(), expect_depth)
    for f in range(3):
        one_rgb, one_depth, one_levels = inpaint_frames(t_rgb[f:f + 1], t_depth[f:f + 1], t_masks[f:f + 1], dilation=(5, 5, 0), radius=5, return_levels=True)
        assert same(one_rgb[0], out_rgb[f]) and same(one_depth[0], out_depth[f]) and one_levels[0] == levels[f]
        assert same(inpaint_telea(t_rgb[f], t_masks[f], 5), out_rgb[f])
        assert same(inpaint_telea(t_depth[f], t_masks[f], 5), out_depth[f])
    # either image alone
    only_rgb, none = inpaint_frames(t_rgb, None, t_masks, dilation=(5, 5, 0), radius=5)
    assert none is None and same(only_rgb, out_rgb)
    none, only_depth = inpaint_frames(None, t_depth, t_masks, dilation=(5, 5, 0), radius=5)
    assert none is None and same(only_depth, out_depth)


def test_dilation_inside_frames_equals_dilate_then_plain_call(gpu_ctx):
    import torch
    from hive_amd.image_processing import dilate_mask, inpaint_frames, inpaint_telea
    from hive_amd.options import MaskDilationOptions
    rgb = np.stack([R.random_image(70, 133, np.uint8, 3, seed=40 + f) for f in range(2)])
    depth = np.stack([R.random_image(70, 133, np.uint16, seed=50 + f) for f in range(2)])
    masks = np.zeros((2, 70, 133), np.uint8)
    masks[0, 30:33, 60:70] = 3   # instance ids, not 0 / 1
    masks[0, 0, 0] = 1           # grows into the corner
    masks[1, 66:, 100:104] = 2
    t_rgb, t_depth, t_masks = (torch.from_numpy(a).cuda() for a in (rgb, depth, masks))
    for kh, kw, iterations in ((5, 5, 2), (3, 5, 1)):
        out_rgb, out_depth = inpaint_frames(t_rgb, t_depth, t_masks, dilation=(kh, kw, iterations), radius=5)
        for f in range(2):
            grown = dilate_mask(masks[f], MaskDilationOptions(num_iterations=iterations, dilation_filter=np.ones((kh, kw), np.uint8)))
            assert np.array_equal(grown, R.dilate_box(masks[f], kh, kw, iterations) != 0)
            assert np.array_equal(out_rgb[f].cpu().numpy(), inpaint_telea(rgb[f], grown, 5))
            assert np.array_equal(out_depth[f].cpu().numpy(), inpaint_telea(depth[f], grown, 5))


def test_errors_leave_the_context_usable(gpu_ctx):
    import torch
    from hive_amd import _lib
    from hive_amd.image_processing import inpaint_frames, inpaint_telea
    image, mask, expect, _ = case("one_pixel", "u8", 2)
    for radius, holes in ((1, mask), (65, mask), (5, np.ones_like(mask))):
        with pytest.raises(_lib.HiveError) as err:
            inpaint_telea(image, holes, radius)
        assert err.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.HiveError) as err:
            inpaint_telea(torch.from_numpy(np.array(image)).cuda(), torch.from_numpy(np.array(holes)).cuda(), radius)
        assert err.value.code == _lib.ERR_INVALID
    rgb, depth, masks = batch_frames()
    masks[1] = 1  # one frame of the batch without a known pixel
    with pytest.raises(_lib.HiveError) as err:
        inpaint_frames(torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda(), torch.from_numpy(masks).cuda(), dilation=(5, 5, 0), radius=5)
    assert err.value.code == _lib.ERR_INVALID and "frame 1" in str(err.value)
    assert np.array_equal(inpaint_telea(image, mask, 2), expect)


def write_hive_folder(path, color, depth_mm, masks, K, poses_c2w):
    from PIL import Image
    from hive_amd import synthetic
    from hive_amd.io import DatasetMetadata, HiveDataset
    n, H, W = masks.shape
    for folder in HiveDataset.required_folders:
        os.makedirs(os.path.join(path, folder))
    for i in range(n):
        name = f"{i:06d}.png"
        Image.fromarray(color[i]).save(os.path.join(path, "rgb", name))
        Image.fromarray(depth_mm[i]).save(os.path.join(path, "depth", name))
        Image.fromarray(masks[i]).save(os.path.join(path, "mask", name))
    DatasetMetadata(num_frames=n, fps=30.0, width=W, height=H).save(os.path.join(path, HiveDataset.metadata_filename))
    np.savetxt(os.path.join(path, HiveDataset.camera_matrix_filename), K)
    np.savetxt(os.path.join(path, HiveDataset.camera_trajectory_filename), synthetic.trajectory_rows_world_to_cam(poses_c2w))


def test_inpaint_frame_data_end_to_end(gpu_ctx, tmp_path):
    """An 8-frame 48 x 64 HIVE folder with drifting ellipses: ``inpaint_frame_data`` writes the three folders with the restatement's bits
    (masks dilated 5 x 5 x 5, radius 30), the dataset then serves them, and ``tsdf_fusion`` on it equals ``tsdf_fusion`` on a copy whose
    ``*_inpainted`` folders were written from the restatement."""
    import shutil
    from PIL import Image
    from hive_amd import synthetic
    from hive_amd.dataset_adaptors import inpaint_frame_data
    from hive_amd.fusion import tsdf_fusion
    from hive_amd.io import HiveDataset
    from hive_amd.options import BackgroundMeshOptions, InpaintingMode
    seq = synthetic.make_sequence(num_frames=8, height=48, width=64, yaw_step_deg=20.0)
    masks = synthetic.ellipse_masks(8, 48, 64, num_objects=2)
    depth_mm = (seq["depth"] * 1000.0).astype(np.uint16)
    ours, by_hand = str(tmp_path / "ours"), str(tmp_path / "by_hand")
    write_hive_folder(ours, seq["color"], depth_mm, masks, seq["K"], seq["poses"])
    shutil.copytree(ours, by_hand)
    assert not HiveDataset(ours).has_inpainted_frame_data

    inpaint_frame_data(ours, InpaintingMode.CV2_Image_Depth, batch_size=3)  # batches of 3 + 3 + 2

    grown = np.stack([R.dilate_box(m, 5, 5, 5) for m in masks])
    assert 0 < grown.mean() < 1
    expect_rgb, expect_depth = R.inpaint_batch([seq["color"], depth_mm], grown, 30)
    for folder in ("rgb_inpainted", "depth_inpainted", "mask_inpainted"):
        os.makedirs(os.path.join(by_hand, folder))
    for i in range(8):
        name = f"{i:06d}.png"
        Image.fromarray(expect_rgb[i]).save(os.path.join(by_hand, "rgb_inpainted", name))
        Image.fromarray(expect_depth[i]).save(os.path.join(by_hand, "depth_inpainted", name))
        Image.fromarray(np.zeros((48, 64), np.uint8)).save(os.path.join(by_hand, "mask_inpainted", name))
        assert sorted(os.listdir(os.path.join(ours, "rgb_inpainted"))) == sorted(os.listdir(os.path.join(ours, "rgb")))
        got_rgb = np.asarray(Image.open(os.path.join(ours, "rgb_inpainted", name)))
        got_depth = np.asarray(Image.open(os.path.join(ours, "depth_inpainted", name)))
        got_mask = np.asarray(Image.open(os.path.join(ours, "mask_inpainted", name)))
        assert got_rgb.dtype == np.uint8 and np.array_equal(got_rgb, expect_rgb[i])
        assert Image.open(os.path.join(ours, "depth_inpainted", name)).mode == "I;16" and np.array_equal(got_depth, expect_depth[i])
        assert got_mask.dtype == np.uint8 and got_mask.shape == (48, 64) and not got_mask.any()
    dataset, reference = HiveDataset(ours), HiveDataset(by_hand)
    assert dataset.has_inpainted_frame_data and dataset.bg_depth_dataset is dataset.inpainted_depth_dataset
    options = BackgroundMeshOptions(sdf_voxel_size=0.08)
    mesh, expect_mesh = tsdf_fusion(dataset, options), tsdf_fusion(reference, options)
    assert len(mesh.vertices) > 0
    assert np.array_equal(mesh.vertices, expect_mesh.vertices) and np.array_equal(mesh.faces, expect_mesh.faces)
    assert np.array_equal(np.asarray(mesh.visual.vertex_colors), np.asarray(expect_mesh.visual.vertex_colors))
