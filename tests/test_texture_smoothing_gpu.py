"""csrc/texture_smooth.hip against tests/texture_smoothing_restatement.py, bit for bit: the adjacency, the labelling on synthetic tables (twice, and with a
read-back after every round), one view's table against hive_texture_select, ``texture_mesh`` on the fused room, and the pipeline switch."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import texture_smoothing_cases as SC  # noqa: E402
import texture_smoothing_restatement as SR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("vertices", "faces", "uv", "texture", "views")


# ------------------------------------------------------------------------------------------------ neighbours
@pytest.mark.parametrize("name", list(SC.NEIGHBOUR_CASES))
def test_face_neighbours(gpu_ctx, name):
    import torch
    from hive_amd import texturing
    faces, nv = SC.NEIGHBOUR_CASES[name]
    want_offsets, want = SR.face_neighbours(faces, nv)
    for source in (faces, torch.from_numpy(faces).cuda()):
        offsets, neighbours = texturing.face_neighbours(source, nv, ctx=gpu_ctx)
        assert offsets.dtype == torch.int64 and neighbours.dtype == torch.int32 and offsets.is_cuda and neighbours.is_cuda
        assert np.array_equal(offsets.cpu().numpy(), want_offsets) and np.array_equal(neighbours.cpu().numpy(), want), name
    if name == "fan of 64":
        assert len(want) == 64 * 63 > 3 * 64, "more entries than the first capacity: the wrapper asked again"


def test_face_neighbours_too_small_a_capacity_names_the_total(gpu_ctx):
    import torch
    from hive_amd import _lib
    faces, nv = SC.TETRAHEDRON
    f = torch.from_numpy(faces).cuda()
    offsets, room, total = torch.empty(5, dtype=torch.int64, device="cuda"), torch.full((12,), -7, dtype=torch.int32, device="cuda"), ctypes.c_int64(0)
    rc = gpu_ctx.lib.hive_mesh_face_neighbours(gpu_ctx.handle, _lib.ptr(f), 4, nv, _lib.ptr(offsets), _lib.ptr(room), 11, ctypes.byref(total))
    assert rc == _lib.ERR_INVALID and total.value == 12 and (room == -7).all()
    with pytest.raises(_lib.HiveError, match="12 entries"):
        gpu_ctx.check(rc)
    gpu_ctx.check(gpu_ctx.lib.hive_mesh_face_neighbours(gpu_ctx.handle, _lib.ptr(f), 4, nv, _lib.ptr(offsets), _lib.ptr(room), 12, ctypes.byref(total)))
    assert room.cpu().tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2] and offsets.cpu().tolist() == [0, 3, 6, 9, 12]


# ------------------------------------------------------------------------------------------------ smooth on synthetic tables
@pytest.mark.parametrize("family", SC.FAMILIES)
@pytest.mark.parametrize("name", list(SC.SMOOTH_MESHES))
def test_smooth_labels(gpu_ctx, name, family):
    from hive_amd import texturing
    faces, nv, n = SC.SMOOTH_MESHES[name]
    offsets, neighbours = texturing.face_neighbours(faces, nv, ctx=gpu_ctx)
    assert np.array_equal(offsets.cpu().numpy(), SC.adjacency(name)[0]) and np.array_equal(neighbours.cpu().numpy(), SC.adjacency(name)[1])
    area = SC.table(family, n, len(faces))
    assert ((area.max(axis=0) == 0).mean() > 0.02) and (area.max(axis=0) > 0).mean() > 0.8, "some faces have no view"
    moved = 0
    for seam_cost in SC.SEAM_COSTS:
        want_best, want_labels, want_stats = SC.smoothed(name, family, seam_cost)
        for what, poll in (("first run", 0), ("second run", 0), ("a read-back after every round", 1)):
            best, stats = texturing.smooth_labels(area, offsets, neighbours, seam_cost, ctx=gpu_ctx, rounds_per_poll=poll)
            best = best.cpu().numpy().view(np.uint64)
            assert np.array_equal(stats, want_stats), f"{name} {family} {seam_cost} {what}: stats {stats.tolist()}, expected {want_stats.tolist()}"
            assert np.array_equal(best, want_best) and np.array_equal(TR.views_of(best), want_labels), f"{name} {family} {seam_cost} {what}"
        moved += int(want_stats[1])
    assert moved > 0, "the case moves labels at some cost"


def test_smooth_refusals(gpu_ctx):
    from hive_amd import _lib, texturing
    faces, nv, n = SC.SMOOTH_MESHES["8 x 8"]
    offsets, neighbours = SC.adjacency("8 x 8")
    area = SC.table("random", n, len(faces))
    texturing.smooth_labels(area, offsets, neighbours, 2 ** 40 - 1, ctx=gpu_ctx)
    broken = neighbours.copy()
    broken[5] = len(faces)
    for what, call in [("seam_cost 2^40", lambda: texturing.smooth_labels(area, offsets, neighbours, 2 ** 40, ctx=gpu_ctx)),
                       ("a negative seam cost", lambda: texturing.smooth_labels(area, offsets, neighbours, -1, ctx=gpu_ctx)),
                       ("a neighbour id out of range", lambda: texturing.smooth_labels(area, offsets, broken, 1, ctx=gpu_ctx)),
                       ("offsets past the entries", lambda: texturing.smooth_labels(area, offsets + 1, neighbours, 1, ctx=gpu_ctx)),
                       ("a negative area", lambda: texturing.smooth_labels(-area, offsets, neighbours, 1, ctx=gpu_ctx))]:
        with pytest.raises(_lib.HiveError) as caught:
            call()
        assert caught.value.code == _lib.ERR_INVALID, what


# ------------------------------------------------------------------------------------------------ vote
def votes_and_keys(ctx, mesh, K, poses, masks=None, facing=0, depth_tolerance=0.05, near=0.05):
    """Per view draw and resolve as ``texture_mesh`` does, then hive_texture_select and hive_texture_vote on the same projected vertices and depth plane.
    -> (area int64 (n, nf), best uint64 (nf,))."""
    import torch
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers
    lib, handle = ctx.lib, ctx.handle
    v = torch.from_numpy(np.ascontiguousarray(mesh["vertices"], np.float64)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(mesh["faces"], np.int32)).cuda()
    nv, nf, n = len(v), len(f), len(poses)
    K = np.ascontiguousarray(K, np.float64)
    buffers = RenderBuffers(C.H, C.W, "cuda")
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((C.H, C.W), dtype=torch.float32, device="cuda")
    best = torch.zeros(nf, dtype=torch.int64, device="cuda")
    area = torch.full((n, nf), -1, dtype=torch.int64, device="cuda")  # every entry must be written
    d_masks = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks != 0).astype(np.uint8)).cuda()
    for k in range(n):
        R, t = np.ascontiguousarray(poses[k][:3, :3], np.float64), np.ascontiguousarray(poses[k][:3, 3], np.float64)
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), C.H, C.W))
        ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), C.H, C.W, near, ptr(xy), ptr(z), ptr(large), ptr(counts),
                                       ptr(buffers.key)))
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), C.H, C.W, None, None, ptr(depth), None))
        mask = ptr(None if d_masks is None else d_masks[k])
        ctx.check(lib.hive_texture_select(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), mask, C.H, C.W, k, depth_tolerance, ptr(best)))
        ctx.check(lib.hive_texture_vote(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), mask, C.H, C.W, k, depth_tolerance, facing, ptr(area)))
    return area.cpu().numpy(), best.cpu().numpy().view(np.uint64)


def keys_of(area):
    """select's keys from a table: the largest area, on equal area the lower view."""
    labels = SR.start_labels(area)
    return np.array([0 if l < 0 else (int(area[l, f]) << 16) | (65535 - int(l)) for f, l in enumerate(labels)], np.uint64)


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("nf, n", [(1, 1), (3, 3), (255, 3), (256, 1), (257, 3), (513, 3)])
def test_vote_argmax_is_select_on_soups(gpu_ctx, nf, n, with_masks):
    case = C.soup_case(nf, 6, n, with_masks)
    area, best = votes_and_keys(gpu_ctx, case["mesh"], C.K, case["poses"], case["masks"])
    assert (area >= 0).all() and np.array_equal(keys_of(area), best)
    assert np.array_equal(area, SR.vote(SR.signed_areas(case["mesh"], C.K, case["poses"], C.H, C.W, case["masks"])))


@functools.lru_cache(maxsize=None)
def room_signed():
    mesh, seq, w2c = C.room()
    return SR.signed_areas(mesh, seq["K"].astype(np.float64), w2c, C.H, C.W)


@pytest.mark.parametrize("with_masks", [False, True])
def test_vote_on_the_room(gpu_ctx, with_masks):
    mesh, seq, w2c = C.room()
    K = seq["K"].astype(np.float64)
    masks = C.masks_for(3, 9) if with_masks else None
    signed = SR.signed_areas(mesh, K, w2c, C.H, C.W, masks) if with_masks else room_signed()
    area, best = votes_and_keys(gpu_ctx, mesh, K, w2c, masks)
    assert np.array_equal(area, SR.vote(signed)) and np.array_equal(keys_of(area), best)
    front, _ = votes_and_keys(gpu_ctx, mesh, K, w2c, masks, facing=1)
    assert np.array_equal(front != 0, signed < 0) and np.array_equal(front, SR.vote(signed, 1)), "facing = 1: exactly the candidates with A < 0"
    back, _ = votes_and_keys(gpu_ctx, mesh, K, w2c, masks, facing=-1)
    assert np.array_equal(back, SR.vote(signed, -1)) and np.array_equal(front + back, area) and (back != 0).any()


def test_vote_facing_on_a_quad_and_its_mirror(gpu_ctx):
    quad = C.quad(*C.QUAD_CORNERS)
    mirror = dict(quad, faces=quad["faces"][:, ::-1].copy())
    both = C.join(quad, mirror)
    either, _ = votes_and_keys(gpu_ctx, both, C.K, C.IDENTITY[None])
    front, _ = votes_and_keys(gpu_ctx, both, C.K, C.IDENTITY[None], facing=1)
    back, _ = votes_and_keys(gpu_ctx, both, C.K, C.IDENTITY[None], facing=-1)
    assert (either[0] > 0).all() and either[0, 0] == either[0, 2] and either[0, 1] == either[0, 3]
    for f in (0, 1):
        assert (front[0, f] != 0) != (front[0, f + 2] != 0) and (back[0, f] != 0) != (back[0, f + 2] != 0), "exactly one of a face and its mirror"
    assert np.array_equal(front + back, either) and np.array_equal(front[0] != 0, back[0] == 0)
    assert np.array_equal(front, SR.vote(SR.signed_areas(both, C.K, C.IDENTITY[None], C.H, C.W), 1))


def test_vote_refusals(gpu_ctx):
    from hive_amd import _lib
    quad = C.quad(*C.QUAD_CORNERS)
    for facing in (2, -2):
        with pytest.raises(_lib.HiveError):
            votes_and_keys(gpu_ctx, quad, C.K, C.IDENTITY[None], facing=facing)
    rc = gpu_ctx.lib.hive_texture_vote(gpu_ctx.handle, None, 2 ** 30, 4, None, None, None, None, C.H, C.W, 1, 0.05, 0, None)
    assert rc == _lib.ERR_INVALID, "row 1 of 2^30 faces ends at entry 2^31"


# ------------------------------------------------------------------------------------------------ texture_mesh
def native(ctx, mesh, frames, K, poses, device_inputs=False, **kw):
    import torch
    from hive_amd import texturing
    if device_inputs:
        mesh = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mesh.items()}
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = texturing.texture_mesh(mesh, frames, K, poses, ctx=ctx, return_views=True, return_stats=True, **kw)
    return dict({k: out[k].cpu().numpy() for k in KEYS}, stats=out["stats"])


def same(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    assert [got["stats"][name] for name in ("rounds", "label_changes", "seam_entries_before", "seam_entries_after")] == want["stats"][:4].tolist(), what
    assert got["stats"]["area_given_up_px2"] == want["stats"][4] / SR.UNITS_PER_PX2, what


@functools.lru_cache(maxsize=None)
def room_restated(smoothness, cull, reverse):
    mesh, seq, w2c = C.room()
    order = slice(None, None, -1) if reverse else slice(None)
    return SR.texture_mesh(mesh, seq["color"][order], seq["K"].astype(np.float64), w2c[order], smoothness=smoothness, cull_back_faces=cull)


@pytest.mark.parametrize("smoothness, cull", [(4.0, False), (0.0, True)])
def test_texture_mesh_on_the_room(gpu_ctx, smoothness, cull):
    mesh, seq, w2c = C.room()
    frames, K = seq["color"], seq["K"].astype(np.float64)
    want = room_restated(smoothness, cull, False)
    kw = dict(smoothness=smoothness, cull_back_faces=cull)
    same(native(gpu_ctx, mesh, frames, K, w2c, **kw), want, "first run")
    same(native(gpu_ctx, mesh, frames, K, w2c, **kw), want, "second run")
    same(native(gpu_ctx, mesh, frames, K, w2c, device_inputs=True, **kw), want, "device inputs")
    # on equal areas the lower view index wins, so a reversal may move a label: the reversed run against the restatement of the reversed inputs
    same(native(gpu_ctx, mesh, frames[::-1], K, w2c[::-1], **kw), room_restated(smoothness, cull, True), "views reversed")
    plain = TR.views_of(TR.select(mesh, K, w2c, C.H, C.W))
    assert not np.array_equal(want["views"], plain), "the options change the labels of this mesh"
    if cull:
        assert want["stats"].tolist() == [0, 0] + [SR.seam_entries(want["views"], *SR.face_neighbours(mesh["faces"], len(mesh["vertices"])))] * 2 + [0]
        assert ((want["views"] >= 0) <= (plain >= 0)).all() and (want["views"] >= 0).sum() < (plain >= 0).sum()
    else:
        assert want["stats"][:4].tolist() == [2, 24, 176, 137]


def test_the_defaults_passed_explicitly_are_the_plain_call(gpu_ctx):
    from hive_amd import texturing
    mesh, seq, w2c = C.room()
    plain = texturing.texture_mesh(mesh, seq["color"], seq["K"], w2c, ctx=gpu_ctx, return_views=True)
    explicit = texturing.texture_mesh(mesh, seq["color"], seq["K"], w2c, ctx=gpu_ctx, return_views=True, smoothness=0.0, cull_back_faces=False, return_stats=True)
    assert set(plain) == set(KEYS) and set(explicit) == set(KEYS) | {"stats"} and explicit["stats"] is None
    for k in KEYS:
        assert plain[k].dtype == explicit[k].dtype and plain[k].cpu().numpy().tobytes() == explicit[k].cpu().numpy().tobytes(), k
    assert np.array_equal(plain["views"].cpu().numpy(), TR.views_of(TR.select(mesh, seq["K"].astype(np.float64), w2c, C.H, C.W)))


# ------------------------------------------------------------------------------------------------ use
def test_render_mesh_takes_the_result(gpu_ctx):
    """Textured from frames 0 and 2; PSNR in dB over the pixels both renders cover, per-face labels -> smoothed at 4 px^2.  The synthetic frames agree with one
    another (no pose error, one exposure), so no direction is implied and none is asserted.  Measured on an MI355X: frame 1 (held out) 32.85 -> 32.85,
    frame 0 34.69 -> 34.70 (3 labels of 2 052 move, 61 -> 58 seam entries)."""
    from hive_amd import render, texturing
    mesh, seq, w2c = C.room()
    K = seq["K"].astype(np.float64)
    frames, poses = seq["color"][[0, 2]], w2c[[0, 2]]
    plain = texturing.texture_mesh(mesh, frames, K, poses, ctx=gpu_ctx)
    smoothed = texturing.texture_mesh(mesh, frames, K, poses, ctx=gpu_ctx, smoothness=4.0, return_stats=True)
    stats = smoothed.pop("stats")
    assert set(smoothed) == {"vertices", "faces", "uv", "texture"} and stats["seam_entries_after"] < stats["seam_entries_before"]
    for view in (1, 0):
        a, _, face_a = render.render_mesh(K, w2c[view], plain, size=(C.H, C.W), return_depth=True, return_faces=True, ctx=gpu_ctx)
        b, _, face_b = render.render_mesh(K, w2c[view], smoothed, size=(C.H, C.W), return_depth=True, return_faces=True, ctx=gpu_ctx)
        assert np.array_equal(face_a.cpu().numpy(), face_b.cpu().numpy()), "the geometry is the same"
        covered = face_a.cpu().numpy() >= 0
        assert covered.mean() > 0.8
        before, after = render.psnr(a, seq["color"][view], covered), render.psnr(b, seq["color"][view], covered)
        print(f"pose of frame {view}: per-face labels {before:.2f} dB, smoothed at 4 px^2 {after:.2f} dB over {int(covered.sum())} pixels; smoothing {stats}")
        assert np.isfinite(before) and np.isfinite(after)


def test_pipeline_switch(gpu_ctx, tmp_path):
    """``--export_gltf --texture_background --texture_smoothness 4``: bg.glb reads back, and the profiling record carries the smoothing's stats."""
    from PIL import Image
    from hive_amd import gltf, synthetic
    from hive_amd.dataset_adaptors import get_dataset
    from hive_amd.options import BackgroundMeshOptions, PipelineOptions, WebXROptions
    from hive_amd.pipeline import Pipeline
    from tum_fixture import write_tum_sequence
    import argparse
    tum, hive = str(tmp_path / "tum"), str(tmp_path / "hive")
    n = 3
    write_tum_sequence(tum, num_frames=n, yaw_step_deg=10.0)
    ds = get_dataset(tum, hive)
    masks = synthetic.ellipse_masks(n, ds.frame_height, ds.frame_width, num_objects=3, seed=5)
    for name, m in zip(sorted(os.listdir(os.path.join(hive, "mask"))), masks):
        Image.fromarray(m).save(os.path.join(hive, "mask", name))
    parser = argparse.ArgumentParser()
    PipelineOptions.add_args(parser)
    options = PipelineOptions.from_args(parser.parse_args(["--num_frames", str(n), "--export_gltf", "--texture_background", "--texture_smoothness", "4", "--texture_cell", "6"]))
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.08, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)
    pipe = Pipeline(options=options, background_mesh_options=bg_options, webxr_options=WebXROptions(webxr_path=str(tmp_path / "player")))
    pipe.run(hive, str(tmp_path / "out"), True, export_gltf=True)
    record = pipe.profiling["background_texturing"]
    print(f"background texturing: {record}")
    stats = record["smoothing"]
    assert set(stats) == {"rounds", "label_changes", "seam_entries_before", "seam_entries_after", "area_given_up_px2"}
    assert stats["seam_entries_after"] <= stats["seam_entries_before"] and stats["rounds"] <= stats["label_changes"] and stats["area_given_up_px2"] >= 0
    back = gltf.read_glb(str(tmp_path / "out" / "mesh" / "bg.glb"))
    mesh = back.meshes()[0]
    assert list(back.geometry) == ["000000"] and len(mesh["vertices"]) == 3 * len(mesh["faces"]) == 3 * record["faces"] and mesh["texture"].any()
