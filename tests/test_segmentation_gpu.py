"""csrc/segment.hip through hive_amd.segmentation against the restatement (tests/segmentation_restatement.py): everything here is exact equality, nothing has a
tolerance.  The labelling runs on the pictures of tests/segmentation_cases.py (built from the kernel's tile), each with connectivity 8 and 4, alone, inside a
batch of mixed pictures in two orders, and a second time with the same bits; then the area filter at its edge, the 255 / 256 limit of uint8 ids, the opening,
every branch of the motion rule, the fused call against the three composed, the moving-sphere sequence end to end on the device against the CPU chain, and a
converted folder."""
import io
import os

import numpy as np
import pytest

import segmentation_cases as sc
import segmentation_restatement as sr
import tracking_cases as tc

pytestmark = pytest.mark.gpu

_wants = {}


def _want(size, connectivity):
    """name -> (labels, k, areas) of the restatement for every picture of a size: computed once, shared."""
    key = (size, connectivity)
    if key not in _wants:
        _wants[key] = {name: sr.label(m, connectivity) for name, m in sc.pictures(*size).items()}
    return _wants[key]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labelling_matches_the_restatement(gpu_ctx, size, connectivity):
    import torch
    from hive_amd import segmentation as seg
    pics, want = sc.pictures(*size), _want(size, connectivity)
    names = list(pics)
    for name in names:  # alone: int32 with areas, and uint8 where the count allows
        labels, k, areas = want[name]
        got, count, got_areas = seg.label_components(pics[name], connectivity, return_areas=True, ctx=gpu_ctx)
        assert got.dtype == torch.int32 and got.shape == size and int(count) == k, (name, int(count), k)
        assert np.array_equal(_np(got), labels), (name, int((_np(got) != labels).sum()))
        assert np.array_equal(_np(got_areas)[:k], areas) and not _np(got_areas)[k:].any(), name
        if k <= 255:
            got8, count8 = seg.label_components(torch.from_numpy(pics[name]).cuda(), connectivity, dtype=torch.uint8, ctx=gpu_ctx)
            assert got8.dtype == torch.uint8 and int(count8) == k and np.array_equal(_np(got8), labels.astype(np.uint8)), name
    for order in (names, names[::-1]):  # a batch of mixed pictures in two orders, and a second time
        batch = np.stack([pics[name] for name in order])
        got, counts = seg.label_components(batch, connectivity, ctx=gpu_ctx)
        again, counts_again = seg.label_components(batch, connectivity, ctx=gpu_ctx)
        assert np.array_equal(_np(counts), [want[name][1] for name in order]) and np.array_equal(_np(counts), _np(counts_again))
        for j, name in enumerate(order):
            assert np.array_equal(_np(got[j]), want[name][0]), (name, "in a batch")
        assert torch.equal(got, again)


def test_min_area_at_a_components_area_and_one_more(gpu_ctx):
    from hive_amd import segmentation as seg
    size = (97, 131)
    for connectivity, name in ((8, "random 0.5"), (4, "random 0.593"), (4, "random 0.3")):
        m = sc.pictures(*size)[name]
        areas = _want(size, connectivity)[name][2]
        a = int(np.sort(areas)[len(areas) // 2])  # a middle area: some components have exactly it, some less, some more
        assert (areas == a).any() and (areas > a).any()
        for min_area in (a, a + 1, 0, 1, int(areas.max()), int(areas.max()) + 1):
            labels, k, kept = sr.label(m, connectivity, min_area)
            got, count, got_areas = seg.label_components(m, connectivity, min_area=min_area, return_areas=True, ctx=gpu_ctx)
            assert int(count) == k and np.array_equal(_np(got), labels) and np.array_equal(_np(got_areas)[:k], kept), (name, min_area)
        assert sr.label(m, connectivity, a)[1] > sr.label(m, connectivity, a + 1)[1]  # area == min_area stays, one more removes it


def test_255_and_256_components(gpu_ctx):
    import torch
    from hive_amd import _lib, segmentation as seg
    row = np.zeros((1, 1023), np.uint8)
    row[0, 0::2] = 1
    labels, k = seg.label_components(row, 8)  # int32 has no limit
    assert int(k) == 512 and np.array_equal(_np(labels), sr.label(row, 8)[0])
    batch = np.zeros((3, 1, 1023), np.uint8)
    batch[0, 0, 0:509:2] = 1
    batch[2, 0, 0:511:2] = 1
    assert [sr.label(b, 8)[1] for b in batch] == [255, 0, 256]
    got, counts = seg.label_components(batch[:2], 8, dtype=torch.uint8, ctx=gpu_ctx)  # 255 components pass
    assert _np(counts).tolist() == [255, 0] and np.array_equal(_np(got[0]), sr.label(batch[0], 8)[0].astype(np.uint8)) and int(got.max()) == 255
    with pytest.raises(_lib.HiveError, match=r"frame 2 has 256 components"):
        seg.label_components(batch, 8, dtype=torch.uint8, ctx=gpu_ctx)
    got, counts = seg.label_components(batch, 8, min_area=2, dtype=torch.uint8, ctx=gpu_ctx)  # the limit counts what the area filter leaves
    assert _np(counts).tolist() == [0, 0, 0] and not _np(got).any()


@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_opening_matches_the_restatement(gpu_ctx, iterations):
    from hive_amd import segmentation as seg
    for size in [(97, 131), (33, 65), (1, 200), (200, 1), (1, 1), (16, 64), (17, 129)]:
        pics = {k: v for k, v in sc.pictures(*size).items() if k.startswith("random") or k in ("full", "empty", "corners")}
        if min(size) >= 7:
            pics.update(sc.border_masks(*size))
        rng = np.random.default_rng(5)
        pics["blobs"] = (sr.ndimage.uniform_filter(rng.random(size), 5, mode="constant") > 0.5).astype(np.uint8)
        want = {name: sr.open_mask(m, iterations) for name, m in pics.items()}
        for name, m in pics.items():
            got = _np(seg.open_mask(m, iterations, ctx=gpu_ctx))
            assert np.array_equal(got, want[name]), (size, name, int((got != want[name]).sum()))
        batch = np.stack(list(pics.values()))
        got = _np(seg.open_mask(batch, iterations, ctx=gpu_ctx))
        assert np.array_equal(got, np.stack(list(want.values()))), size


def test_motion_rule_every_branch(gpu_ctx):
    from hive_amd import segmentation as seg
    f = np.float32
    model, live = f(2.0), f(f(2.0) - f(0.05))
    d = f(model - live)
    cases = [(0.0, 2.0, 0.05, 0.0, 0), (1.0, 0.0, 0.05, 0.0, 0), (-1.0, 2.0, 0.05, 0.0, 0), (live, model, d, 0.0, 0), (live, model, np.nextafter(d, f(0)), 0.0, 1),
             (live, model, 0.0, 0.5, 0), (live, model, 0.0, 0.01, 1), (live, model, 0.01, 0.026, 0), (2.5, 2.0, 0.05, 0.0, 0), (np.nan, 2.0, 0.05, 0.0, 0),
             (1.0, np.inf, 0.0, 0.0, 0)]
    for live_, model_, a, b, want in cases:
        L, M = np.array([[live_]], f), np.array([[model_]], f)
        assert int(sr.motion_mask(L, M, a, b)[0, 0]) == want
        assert int(seg.motion_mask(L, M, a, b, ctx=gpu_ctx)[0, 0]) == want, (live_, model_, a, b)
    # a batch where every branch occurs many times, thresholds met exactly among them
    rng = np.random.default_rng(11)
    M = rng.uniform(0.5, 4.0, (3, 37, 53)).astype(f)
    steps = rng.choice(np.array([0.0, 0.03, 0.05, 0.07, 0.2, -0.1], f), M.shape)
    L = (M - steps).astype(f)
    M[rng.random(M.shape) < 0.1] = 0
    L[rng.random(M.shape) < 0.1] = 0
    for a, b in ((0.05, 0.0), (0.0, 0.02), (0.05, 0.03), (0.0, 0.0)):
        want = sr.motion_mask(L, M, a, b)
        assert 0 < want.mean() < 1 and np.array_equal(_np(seg.motion_mask(L, M, a, b, ctx=gpu_ctx)), want), (a, b)


def test_fused_call_equals_the_three_composed(gpu_ctx):
    import torch
    from hive_amd import segmentation as seg
    rng = np.random.default_rng(3)
    n, h, w = 5, 61, 83
    model = rng.uniform(1.0, 3.0, (n, h, w)).astype(np.float32)
    blobs = np.stack([sr.ndimage.uniform_filter(rng.random((h, w)), 7, mode="constant") > 0.52 for _ in range(n)])
    live = np.where(blobs, model - np.float32(0.3), model + rng.normal(0, 0.01, model.shape).astype(np.float32)).astype(np.float32)
    live[rng.random(live.shape) < 0.05] = 0
    model[rng.random(live.shape) < 0.05] = 0
    several = 0
    for kw in (dict(), dict(relative_difference=0.12, connectivity=4, min_area_share=0.002), dict(opening_iterations=0, min_area_share=0.0, min_difference=0.25),
               dict(opening_iterations=2, min_area_share=0.0)):
        options = seg.MotionSegmentationOptions(**kw)
        ids, counts = seg.motion_masks(live, model, options, ctx=gpu_ctx)
        raw = seg.motion_mask(live, model, options.min_difference, options.relative_difference, ctx=gpu_ctx)
        opened = seg.open_mask(raw, options.opening_iterations, ctx=gpu_ctx)
        labels, k = seg.label_components(opened, options.connectivity, options.min_area(h, w), dtype=torch.uint8, ctx=gpu_ctx)
        assert torch.equal(ids, labels) and torch.equal(counts, k)
        want_ids, want_counts = sr.motion_masks(live, model, options.min_difference, options.relative_difference, options.opening_iterations, options.min_area_share,
                                                options.connectivity)
        assert np.array_equal(_np(ids), want_ids) and np.array_equal(_np(counts), want_counts), kw
        several += int(want_counts.max() >= 2)
    assert several >= 3  # (the inputs are worth the comparison: frames with several objects under most of the parameter sets)


def test_sphere_sequence_on_the_device_equals_the_cpu_chain(gpu_ctx, oracle_lib):
    import torch
    from hive_amd import fusion, segmentation as seg
    seq, chain = sc.sphere_sequence(), sc.cpu_chain(oracle_lib)
    vol = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / sc.SEQ_VOXELS, ctx=gpu_ctx)
    for i in range(sc.SEQ_FRAMES):
        vol.integrate(seq["color"][i], seq["live"][i], seq["K"], seq["poses"][i])
    tsdf, _, weight = vol.get_volume(with_weight=True)
    assert np.array_equal(tsdf, chain["volume"]._tsdf) and np.array_equal(weight, chain["volume"]._weight)  # bit for bit the oracle's
    model = torch.stack([vol.raycast(seq["K"], pose, (sc.SEQ_H, sc.SEQ_W)) for pose in seq["poses"]])
    assert np.array_equal(_np(model).view(np.uint32), chain["model"].view(np.uint32))  # bit for bit the restated ray cast
    ids, counts = seg.motion_masks(seq["live"], model, ctx=gpu_ctx)
    want_ids, want_counts = sr.motion_masks(seq["live"], chain["model"])
    assert np.array_equal(_np(ids), want_ids) and np.array_equal(_np(counts), want_counts)
    assert want_counts.tolist() == [int(t.any()) for t in seq["truth"]]


# ---- a converted folder --------------------------------------------------------------------------------------------------------------------------------------------
def _write_tum(root):
    """The sphere sequence in the TUM layout (tests/tum_fixture.py's, at 48 x 64): depth PNGs in 1 / 5000 m with the sphere composited in."""
    from PIL import Image
    from scipy.spatial.transform import Rotation
    seq = sc.sphere_sequence()
    os.makedirs(os.path.join(root, "rgb")), os.makedirs(os.path.join(root, "depth"))
    lines = {"rgb.txt": ["# color images"], "depth.txt": ["# depth maps"], "groundtruth.txt": ["# timestamp tx ty tz qx qy qz qw"]}
    for i in range(sc.SEQ_FRAMES):
        t = 100.0 + i / 30.0
        Image.fromarray(seq["color"][i]).save(os.path.join(root, "rgb", f"{t:.6f}.png"))
        Image.fromarray(np.round(seq["live"][i].astype(np.float64) * 5000.0).astype(np.uint16)).save(os.path.join(root, "depth", f"{t:.6f}.png"))
        q, p = Rotation.from_matrix(seq["poses"][i][:3, :3]).as_quat(), seq["poses"][i][:3, 3]
        lines["rgb.txt"].append(f"{t:.6f} rgb/{t:.6f}.png")
        lines["depth.txt"].append(f"{t:.6f} depth/{t:.6f}.png")
        lines["groundtruth.txt"].append(f"{t:.6f} {p[0]:.9f} {p[1]:.9f} {p[2]:.9f} {q[0]:.9f} {q[1]:.9f} {q[2]:.9f} {q[3]:.9f}")
    for name, rows in lines.items():
        with open(os.path.join(root, name), "w") as f:
            f.write("\n".join(rows) + "\n")


def _adaptor(*args, **kw):
    from hive_amd.dataset_adaptors import TUMAdaptor

    class SmallTUM(TUMAdaptor):
        width, height = sc.SEQ_W, sc.SEQ_H
        intrinsic_matrix = np.asarray(tc.intrinsics(sc.SEQ_H, sc.SEQ_W), np.float64)
    return SmallTUM(*args, **kw)


def _masks_on_disk(folder):
    from PIL import Image
    names = sorted(os.listdir(os.path.join(folder, "mask")))
    return np.stack([np.asarray(Image.open(os.path.join(folder, "mask", name))) for name in names]), names


def test_segment_dataset_and_convert(tmp_path, gpu_ctx):
    from PIL import Image
    from hive_amd import foreground, segmentation as seg
    from hive_amd.io import HiveDataset
    from hive_amd.options import BackgroundMeshOptions
    tum = str(tmp_path / "tum")
    _write_tum(tum)
    truth = sc.sphere_sequence()["truth"]
    # convert() without the keyword: the mask files of today, which are all zero
    plain = _adaptor(tum, str(tmp_path / "plain")).convert()
    buffer = io.BytesIO()
    Image.fromarray(np.zeros((sc.SEQ_H, sc.SEQ_W), np.uint8)).save(buffer, format="PNG")
    masks, names = _masks_on_disk(plain.base_path)
    assert len(names) == sc.SEQ_FRAMES and not masks.any()
    assert all(open(os.path.join(plain.base_path, "mask", name), "rb").read() == buffer.getvalue() for name in names)
    # segment_dataset on that folder, both encoders: the files read back are the ids returned
    coarse = BackgroundMeshOptions(sdf_voxel_size=tc.VOLUME / sc.SEQ_VOXELS)
    dry = seg.segment_dataset(plain, mesh_options=coarse, write=False)
    assert not _masks_on_disk(plain.base_path)[0].any()
    for encoder in ("host", "gpu"):
        result = seg.segment_dataset(plain, mesh_options=coarse, chunk_frames=5, png_encoder=encoder)
        on_disk, _ = _masks_on_disk(plain.base_path)
        assert on_disk.dtype == np.uint8 and np.array_equal(on_disk, _np(result.masks)) and np.array_equal(_np(result.masks), _np(dry.masks)), encoder
        assert _np(result.counts).tolist() == _np(dry.counts).tolist() == [int(t.any()) for t in truth]
    assert not ((_np(dry.masks) != 0) & ~truth).any()  # (millimetre depths and a rounded trajectory: not the exact chain, but nothing outside the silhouette)
    # convert(segment_motion=True): the same masks in the folder it returns, and the foreground finds the object
    ds = _adaptor(tum, str(tmp_path / "moving")).convert(segment_motion=True)
    moving, _ = _masks_on_disk(ds.base_path)
    assert moving.max() == 1 and [int(m.any()) for m in moving] == [int(t.any()) for t in truth] and not ((moving != 0) & ~truth).any()
    assert np.array_equal(np.asarray(ds.depth_dataset[4]), np.asarray(plain.depth_dataset[4])) and np.array_equal(ds.camera_trajectory.values, plain.camera_trajectory.values)
    i = int(truth.reshape(len(truth), -1).sum(axis=1).argmax())
    pose = ds.camera_trajectory.to_homogenous_transforms()[i]
    args = (np.asarray(ds.rgb_dataset[i]), np.asarray(ds.depth_dataset[i]))
    mesh = foreground.process_frame(*args, np.asarray(HiveDataset(ds.base_path).mask_dataset[i]), ds.camera_matrix, pose, ctx=gpu_ctx)
    assert mesh is not None and len(mesh["vertices"]) >= 9 and len(mesh["faces"]) > 0 and list(mesh["objects"]) == [1]
    assert foreground.process_frame(*args, np.zeros((sc.SEQ_H, sc.SEQ_W), np.uint8), ds.camera_matrix, pose, ctx=gpu_ctx) is None
