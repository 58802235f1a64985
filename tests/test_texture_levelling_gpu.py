"""csrc/texture_level.hip and hive_texture_fill_adjusted against tests/texture_levelling_restatement.py, bit for bit: samples and pair sums on soups, the offsets
on meshes with given labels, ``texture_mesh`` with the two switches on soups and on the scaled-frame room, the defaults, and the pipeline switches."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import texture_levelling_cases as LC  # noqa: E402
import texture_levelling_restatement as LR  # noqa: E402
import texture_smoothing_restatement as SR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("vertices", "faces", "uv", "texture", "views")


def as_u16(t):
    return t.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ samples and sums
def votes_and_samples(ctx, mesh, frames, K, poses, masks=None, depth_tolerance=0.05, near=0.05):
    """hive_texture_vote and hive_texture_samples view by view, as texture_mesh calls them -> area int64 (n, nf), samples (the device tensor, int16 bits)."""
    import torch
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers
    lib, handle = ctx.lib, ctx.handle
    ctx.follow_torch_stream()
    v = torch.from_numpy(np.ascontiguousarray(mesh["vertices"], np.float64)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(mesh["faces"], np.int32)).cuda()
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    nv, nf, n = len(v), len(f), len(poses)
    K = np.ascontiguousarray(K, np.float64)
    buffers = RenderBuffers(C.H, C.W, "cuda")
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((C.H, C.W), dtype=torch.float32, device="cuda")
    area = torch.full((n, nf), -1, dtype=torch.int64, device="cuda")
    samples = torch.full((n, nf, 3), -1, dtype=torch.int16, device="cuda")  # every entry must be written
    d_masks = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks != 0).astype(np.uint8)).cuda()
    for k in range(n):
        R, t = np.ascontiguousarray(poses[k][:3, :3], np.float64), np.ascontiguousarray(poses[k][:3, 3], np.float64)
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), C.H, C.W))
        ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), C.H, C.W, near, ptr(xy), ptr(z), ptr(large), ptr(counts),
                                       ptr(buffers.key)))
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), C.H, C.W, None, None, ptr(depth), None))
        mask = ptr(None if d_masks is None else d_masks[k])
        ctx.check(lib.hive_texture_vote(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), mask, C.H, C.W, k, depth_tolerance, 0, ptr(area)))
        ctx.check(lib.hive_texture_samples(handle, ptr(f), nf, nv, ptr(xy), ptr(area), ptr(d_frames[k]), C.H, C.W, k, ptr(samples)))
    return area.cpu().numpy(), samples


def same_sums(got, want, what):
    for name, g, w in zip("GDN", got, want):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs"


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("n", LC.SUM_VIEWS)
@pytest.mark.parametrize("nf", LC.SUM_FACES)
def test_samples_and_sums_on_soups(gpu_ctx, nf, n, with_masks):
    from hive_amd import texturing
    case = LC.sum_case(nf, n, with_masks)
    area, samples = votes_and_samples(gpu_ctx, case["mesh"], case["frames"], C.K, case["poses"], case["masks"])
    if n <= 3:  # (the table itself: tests/test_texture_smoothing_gpu.py holds it to the restatement at every size; here where the restatement is quick)
        assert np.array_equal(area, SR.vote(SR.signed_areas(case["mesh"], C.K, case["poses"], C.H, C.W, case["masks"])))
    want = LR.samples(case["mesh"], case["frames"], C.K, case["poses"], area)
    assert np.array_equal(as_u16(samples), want), "samples"
    if nf >= 255:
        assert (want != 0).any() and ((want == 0).all(axis=2) & (area != 0)).any(), "valid samples, and candidates with a clipped pixel"
    sums = LR.sums(want)
    same_sums(texturing.exposure_sums(samples, ctx=gpu_ctx), sums, "device table")
    same_sums(texturing.exposure_sums(want, ctx=gpu_ctx), sums, "host table")
    if n == 1:
        assert not any(x.any() for x in sums)
    elif nf >= 255:
        assert sums[2].any()


@pytest.mark.parametrize("nf", [4099, 2048, 2049])
def test_sums_of_the_largest_samples_in_closed_form(gpu_ctx, nf):
    from hive_amd import texturing
    table = np.full((2, nf, 3), 762, np.uint16)
    for t in (table, table[:, ::-1].copy()):
        G, D, N = texturing.exposure_sums(t, ctx=gpu_ctx)
        off = ~np.eye(2, dtype=bool)
        assert (G[:, off] == nf * 762 ** 2).all() and (D[:, off] == nf * 762 ** 2).all() and (N[off] == nf).all()
        assert not G[:, ~off].any() and not D[:, ~off].any() and not N[~off].any()
    ragged = np.arange(1, 2 * nf * 3 + 1, dtype=np.int64).reshape(2, nf, 3) % 763
    ragged = ragged.astype(np.uint16)
    want = LR.sums(ragged)
    same_sums(texturing.exposure_sums(ragged, ctx=gpu_ctx), want, "first run")
    same_sums(texturing.exposure_sums(ragged[:, ::-1].copy(), ctx=gpu_ctx), want, "faces reversed")


def test_sums_refusals(gpu_ctx):
    from hive_amd import _lib, texturing
    with pytest.raises(ValueError, match="256"):
        texturing.exposure_sums(np.zeros((257, 2, 3), np.uint16), ctx=gpu_ctx)
    G = np.zeros((3, 257, 257), np.int64)
    rc = gpu_ctx.lib.hive_texture_exposure_sums(gpu_ctx.handle, None, 257, 2, _lib.ptr(G), _lib.ptr(G), _lib.ptr(G))
    assert rc == _lib.ERR_INVALID
    with pytest.raises(_lib.HiveError, match="256"):
        gpu_ctx.check(rc)
    same_sums(texturing.exposure_sums(np.full((256, 3, 3), 5, np.uint16), ctx=gpu_ctx), LR.sums(np.full((256, 3, 3), 5, np.uint16)), "256 views")


# ------------------------------------------------------------------------------------------------ offsets on given labels
@pytest.mark.parametrize("name", list(LC.LEVEL_CASES))
def test_level_offsets(gpu_ctx, name):
    import torch
    from hive_amd import texturing
    case = LC.level_case(name)
    for sweeps in LC.SWEEPS:
        want, want_stats = LC.levelled(name, sweeps)
        for what in ("first run", "second run", "device inputs"):
            mesh, labels, frames = case["mesh"], case["labels"], case["frames"]
            if what == "device inputs":
                mesh = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mesh.items()}
                labels, frames = torch.from_numpy(labels).cuda(), torch.from_numpy(frames).cuda()
            offsets, stats = texturing.level_offsets(mesh, labels, frames, C.K, case["poses"], case["q"], sweeps, ctx=gpu_ctx)
            assert offsets.dtype == torch.float64 and offsets.is_cuda and tuple(offsets.shape) == want.shape
            assert offsets.cpu().numpy().tobytes() == want.tobytes(), f"{name}, {sweeps} sweeps, {what}"
            assert stats == want_stats, f"{name}, {sweeps} sweeps, {what}: {stats}, expected {want_stats}"
    assert want_stats["seam_vertices"] > 0 and want_stats["max_offset"] > 0


def test_level_refusals(gpu_ctx):
    from hive_amd import texturing
    case = LC.level_case("two quads")
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="sweeps"):
            texturing.level_offsets(case["mesh"], case["labels"], case["frames"], C.K, case["poses"], None, bad, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        texturing.level_offsets(case["mesh"], case["labels"][:3], case["frames"], C.K, case["poses"], None, 1, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        texturing.level_offsets(case["mesh"], case["labels"], case["frames"], C.K, case["poses"], np.ones((3, 3)), 1, ctx=gpu_ctx)


# ------------------------------------------------------------------------------------------------ texture_mesh
def native(ctx, mesh, frames, K, poses, device_inputs=False, **kw):
    import torch
    from hive_amd import texturing
    if device_inputs:
        mesh = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mesh.items()}
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = texturing.texture_mesh(mesh, frames, K, poses, ctx=ctx, return_views=True, return_stats=True, **kw)
    return dict({k: out[k].cpu().numpy() for k in KEYS}, stats=out["stats"])


def same(got, want, what, exposure, levelling):
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    stats = got["stats"]
    assert [stats[name] for name in ("rounds", "label_changes", "seam_entries_before", "seam_entries_after")] == want["stats"]["smoothing"][:4].tolist(), what
    assert ("exposure" in stats, "levelling" in stats) == (exposure, levelling), what
    if exposure:
        g, w = stats["exposure"], want["stats"]["exposure"]
        assert np.array_equal(g["gains"], w["gains"]) and np.array_equal(g["pair_counts"], w["pair_counts"]) and g["fallback_channels"] == w["fallback_channels"], what
    if levelling:
        assert stats["levelling"] == want["stats"]["levelling"], f"{what}: {stats['levelling']}, expected {want['stats']['levelling']}"


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("cell", C.SOUP_CELLS)
@pytest.mark.parametrize("nf", C.SOUP_FACES)
def test_texture_mesh_on_soups(gpu_ctx, nf, cell, with_masks):
    """Both switches, then unit gains and zero offsets: hive_texture_fill_adjusted's atlas is hive_texture_fill's."""
    import torch
    from hive_amd import texturing
    from hive_amd._lib import ptr
    case = C.soup_case(nf, cell, 3, with_masks)
    kw = dict(masks=case["masks"], cell=cell)
    want = LR.texture_mesh(case["mesh"], case["frames"], C.K, case["poses"], exposure=True, levelling=True, **kw)
    same(native(gpu_ctx, case["mesh"], case["frames"], C.K, case["poses"], exposure=True, levelling=True, **kw), want, "both switches", True, True)
    # the adjusted fill alone on the keys of this case
    mesh, n = case["mesh"], 3
    v, f = torch.from_numpy(mesh["vertices"]).cuda(), torch.from_numpy(mesh["faces"]).cuda()
    c = torch.from_numpy(np.ascontiguousarray(mesh["vertex_colors"][:, :3])).cuda()
    best = torch.from_numpy(want["best"].view(np.int64)).cuda()
    frames = torch.from_numpy(case["frames"]).cuda()
    poses = torch.from_numpy(np.ascontiguousarray(np.concatenate([case["poses"][:, :3, :3].reshape(n, 9), case["poses"][:, :3, 3]], axis=1))).cuda()
    wt, ht, _ = texturing.atlas_layout(nf, cell)
    plain, adjusted = torch.zeros((ht, wt, 3), dtype=torch.uint8, device="cuda"), torch.full((ht, wt, 3), 7, dtype=torch.uint8, device="cuda")
    unit = torch.full((n, 3), 65536, dtype=torch.int32, device="cuda")
    zero = torch.zeros((nf, 3, 3), dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(C.K, np.float64)
    args = (gpu_ctx.handle, ptr(v), len(v), ptr(c), ptr(f), nf, ptr(best), ptr(frames), n, C.H, C.W, ptr(K), ptr(poses), 0.05, cell)
    gpu_ctx.follow_torch_stream()
    gpu_ctx.check(gpu_ctx.lib.hive_texture_fill(*args, ptr(plain)))
    gpu_ctx.check(gpu_ctx.lib.hive_texture_fill_adjusted(*args, ptr(unit), ptr(zero), ptr(adjusted)))
    assert torch.equal(plain, adjusted) and plain.any()


@pytest.mark.parametrize("n_views", [2, 3])
def test_texture_mesh_on_the_scaled_room(gpu_ctx, n_views):
    room = LC.room(n_views)
    mesh, frames, K, poses = room["mesh"], room["frames"], room["K"], room["poses"]
    want = LC.room_restated(n_views, True, True)
    kw = dict(exposure=True, levelling=True)
    same(native(gpu_ctx, mesh, frames, K, poses, **kw), want, "first run", True, True)
    same(native(gpu_ctx, mesh, frames, K, poses, **kw), want, "second run", True, True)
    same(native(gpu_ctx, mesh, frames, K, poses, device_inputs=True, **kw), want, "device inputs", True, True)
    same(native(gpu_ctx, mesh, frames, K, poses, exposure=True), LC.room_restated(n_views, True, False), "exposure alone", True, False)
    same(native(gpu_ctx, mesh, frames, K, poses, levelling=True, levelling_sweeps=1), LC.room_restated(n_views, False, True, 1), "levelling alone, one sweep", False, True)
    assert want["stats"]["levelling"]["seam_vertices"] > 10 and want["stats"]["levelling"]["max_offset"] > 1.0
    # the views reversed: the restatement of the reversed inputs (on equal areas the lower index wins, so a reversal may move a label) ...
    backwards = LC.room_restated(n_views, True, True, 64, True)
    same(native(gpu_ctx, mesh, frames[::-1], K, poses[::-1], **kw), backwards, "views reversed", True, True)
    # ... and against the forward run: the labels map by reverse_labels; the gains are the forward ones permuted up to the renormalisation's summation order
    labels_map = np.array_equal(C.reverse_labels(backwards["views"], n_views), want["views"])
    gains_map = np.array_equal(backwards["gains_q16"][::-1], want["gains_q16"])
    print(f"{n_views} views reversed: labels map {labels_map}, Q16 gains permute exactly {gains_map}: {backwards['gains_q16'][::-1].tolist()} against {want['gains_q16'].tolist()}")
    if labels_map and gains_map:
        assert np.array_equal(backwards["texture"], want["texture"]), "the same labels and gains: the same atlas"
    elif labels_map:  # the summation order moved a Q16 value: the offsets at equal q instead
        from hive_amd import texturing
        a, _ = texturing.level_offsets(mesh, want["views"], frames, K, poses, want["gains_q16"], 64, ctx=gpu_ctx)
        b, _ = texturing.level_offsets(mesh, backwards["views"], frames[::-1], K, poses[::-1], want["gains_q16"][::-1], 64, ctx=gpu_ctx)
        assert np.abs(a.cpu().numpy() - b.cpu().numpy()).max() <= 1e-9, "the mean at a seam vertex of three labels is summed in another order: rounding alone"


def test_the_defaults_passed_explicitly_are_the_plain_call(gpu_ctx):
    from hive_amd import render, texturing
    mesh, seq, w2c = C.room()
    plain = texturing.texture_mesh(mesh, seq["color"], seq["K"], w2c, ctx=gpu_ctx, return_views=True)
    explicit = texturing.texture_mesh(mesh, seq["color"], seq["K"], w2c, ctx=gpu_ctx, return_views=True, return_stats=True, exposure=False, exposure_prior=0.01,
                                      levelling=False, levelling_sweeps=64)
    assert set(plain) == set(KEYS) and set(explicit) == set(KEYS) | {"stats"} and explicit["stats"] is None
    for k in KEYS:
        assert plain[k].dtype == explicit[k].dtype and plain[k].cpu().numpy().tobytes() == explicit[k].cpu().numpy().tobytes(), k
    room = LC.room(2)
    both = texturing.texture_mesh(room["mesh"], room["frames"], room["K"], room["poses"], ctx=gpu_ctx, exposure=True, levelling=True)
    scaled = texturing.texture_mesh(room["mesh"], room["frames"], room["K"], room["poses"], ctx=gpu_ctx)
    assert set(both) == {"vertices", "faces", "uv", "texture"}
    psnr = []
    for textured in (scaled, both):
        image, _, face = render.render_mesh(room["K"], room["all_poses"][1], textured, size=(C.H, C.W), return_depth=True, return_faces=True, ctx=gpu_ctx)
        covered = face.cpu().numpy() >= 0
        psnr.append(render.psnr(image, room["all_clean"][1], covered))
    print(f"pose of frame 1 (held out): scaled frames {psnr[0]:.2f} dB, gains and levelling {psnr[1]:.2f} dB over {int(covered.sum())} pixels")
    assert covered.mean() > 0.8 and psnr[1] > psnr[0]


def test_pipeline_switches(gpu_ctx, tmp_path):
    """``--export_gltf --texture_background --texture_exposure --texture_levelling``: bg.glb reads back and the record holds gains and seam counts; with both off
    bg.glb is byte for byte the file of a run without the flags."""
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

    def run(out, *flags):
        parser = argparse.ArgumentParser()
        PipelineOptions.add_args(parser)
        options = PipelineOptions.from_args(parser.parse_args(["--num_frames", str(n), "--export_gltf", "--texture_background", "--texture_cell", "6", *flags]))
        bg_options = BackgroundMeshOptions(sdf_voxel_size=0.08, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)
        pipe = Pipeline(options=options, background_mesh_options=bg_options, webxr_options=WebXROptions(webxr_path=str(tmp_path / ("player_" + out))))
        pipe.run(hive, str(tmp_path / out), True, export_gltf=True)
        return pipe.profiling["background_texturing"], str(tmp_path / out / "mesh" / "bg.glb")

    off, off_glb = run("off")
    explicit, explicit_glb = run("explicit", "--texture_levelling_sweeps", "64")
    assert set(off) == set(explicit) == {"key_frames", "faces", "faces_with_a_view", "atlas"}
    assert open(off_glb, "rb").read() == open(explicit_glb, "rb").read()
    record, glb = run("on", "--texture_exposure", "--texture_levelling")
    print(f"background texturing: {record}")
    assert set(record) == set(off) | {"exposure", "levelling"} and {k: record[k] for k in off} == off
    gains = np.asarray(record["exposure"]["gains"])
    assert gains.shape == (len(record["key_frames"]), 3) and (gains >= 0.25).all() and (gains <= 4.0).all()
    assert np.asarray(record["exposure"]["pair_counts"]).shape == (len(gains), len(gains)) and record["exposure"]["fallback_channels"] == []
    assert record["levelling"]["sweeps"] == 64 and record["levelling"]["seam_vertices"] >= 0 and record["levelling"]["max_offset"] >= 0
    back = gltf.read_glb(glb)
    mesh = back.meshes()[0]
    assert list(back.geometry) == ["000000"] and len(mesh["vertices"]) == 3 * len(mesh["faces"]) == 3 * record["faces"] and mesh["texture"].any()
