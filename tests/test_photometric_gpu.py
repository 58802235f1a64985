"""The photometric term of csrc/track.hip and hive_amd/tracking.py on the GPU against the numpy restatement (tests/photometric_restatement.py): the intensity
pyramid and all 56 sums, both counts and both masks of ``hive_rgbd_icp_step`` bit for bit, ``icp_align`` with colour and the track-and-fuse loop on the
two-wall slide against the same loops restated on the CPU.  Scenes and written figures: tests/photometric_cases.py."""
import inspect

import numpy as np
import pytest

import photometric_cases as pc
import photometric_restatement as pr
import tracking_cases as tc
import tracking_restatement as tr

pytestmark = pytest.mark.gpu

COS_MIN = float(np.cos(np.deg2rad(20.0)))


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _picture(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    color = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    color[0, 0], color[-1, -1] = 255, 0
    return color


@pytest.mark.parametrize("H, W, levels", [(13, 37, 2), (48, 64, 3), (23, 31, 3), (4, 4, 1)])
def test_gray_pyramid_matches_the_restatement_bit_for_bit(gpu_ctx, H, W, levels):
    import torch
    from hive_amd import tracking
    color = _picture(H, W)
    want = pr.gray_pyramid(color, levels)
    for source in (color, torch.from_numpy(color).cuda()):
        got = tracking.intensity_pyramid(source, levels, ctx=gpu_ctx)
        assert len(got) == levels
        for l in range(levels):
            g = got[l].cpu().numpy()
            assert g.shape == want[l].shape == (H >> l, W >> l) and g.dtype == np.float32
            assert np.array_equal(_bits32(g), _bits32(want[l])), (H, W, l, int((_bits32(g) != _bits32(want[l])).sum()))
    with pytest.raises(ValueError):
        tracking.intensity_pyramid(color, 8, ctx=gpu_ctx)


@pytest.fixture(scope="module")
def scenes(oracle_lib):
    """(H, W) -> the two-wall scene at that size with the inputs of one step at level 0: the restated model maps at the fused pose, the live frame's maps and
    intensity, and the estimate after two restated updates with weight 0.1."""
    out = {}
    for H, W, voxels in ((24, 32, 32), (48, 64, 64)):
        s = pc.two_wall_scene(oracle_lib, H, W, voxels)
        s["dist"] = float(2.0 * s["vol"]._trunc_margin)
        s["model_d"], s["model_v"], s["model_n"], s["model_c"] = tr.raycast_oracle(s["vol"], s["K"], s["pose"], (H, W))
        _, Vs, Ns, _ = tr.frame_maps(s["depth"], s["K"], 1)
        s["live_v"], s["live_n"], s["live_i"] = Vs[0], Ns[0], pr.gray(s["color"])
        est = s["pose"].copy()
        for _ in range(2):
            sums, _, _ = _restated(s, s["K"], est)
            xi, _ = tr.solve(pr.combine(sums, 0.1))
            est = tr.se3_exp(xi) @ est
        s["est_2"] = est
        out[(H, W)] = s
    return out


MAPS = ("live_v", "live_n", "live_i", "model_v", "model_n", "model_d", "model_c")


def _restated(maps, K, est, model_pose=None):
    model_pose = maps["pose"] if model_pose is None else model_pose
    return pr.rgbd_icp_step(K, maps["live_v"], maps["live_n"], maps["live_i"], maps["model_v"], maps["model_n"], maps["model_d"], maps["model_c"], model_pose, est,
                            maps["dist"], COS_MIN)


def _check_step(gpu_ctx, maps, K, est, model_pose=None):
    """One ``hive_rgbd_icp_step`` against the restatement and against ``hive_icp_step``, bit for bit; -> (sums, pairs, masks) of the restatement."""
    import torch
    from hive_amd import tracking
    model_pose = maps["pose"] if model_pose is None else model_pose
    H, W = maps["live_i"].shape
    want, want_pairs, want_masks = _restated(maps, K, est, model_pose)
    dev = [torch.from_numpy(np.ascontiguousarray(maps[k])).cuda() for k in MAPS]
    masks = [torch.full((H, W), 7, dtype=torch.uint8, device="cuda") for _ in range(2)]
    got, pairs = tracking.rgbd_icp_step(gpu_ctx, K, *dev, model_pose, est, maps["dist"], COS_MIN, pair_mask=masks[0], photo_mask=masks[1])
    again, pairs_again = tracking.rgbd_icp_step(gpu_ctx, K, *dev, model_pose, est, maps["dist"], COS_MIN)
    geo, geo_pairs = tracking.icp_step(gpu_ctx, K, dev[0], dev[1], dev[3], dev[4], model_pose, est, maps["dist"], COS_MIN)
    print(f"{H} x {W}: pairs {pairs} (restated {want_pairs}), sums that differ {int((_bits64(got) != _bits64(want)).sum())} of 56")
    assert pairs == tuple(want_pairs) == pairs_again == (int(want_masks[0].sum()), int(want_masks[1].sum()))
    for g, w in zip(masks, want_masks):
        assert np.array_equal(g.cpu().numpy(), w.astype(np.uint8))
    assert got.shape == (56,) and np.array_equal(_bits64(got), _bits64(want))
    assert np.array_equal(_bits64(got), _bits64(again))
    assert np.array_equal(_bits64(got[:28]), _bits64(geo)) and pairs[0] == geo_pairs
    return want, want_pairs, want_masks


@pytest.mark.parametrize("size", [(24, 32), (48, 64)])
def test_rgbd_icp_step_sums_counts_and_masks(gpu_ctx, scenes, size):
    """The first iteration and the estimate after two updates: the image border is rejected, and most of the rest is kept for both terms."""
    s = scenes[size]
    H, W = size
    for est in (s["pose"], s["est_2"]):
        _, pairs, masks = _check_step(gpu_ctx, s, s["K"], est)
        assert pairs[0] > 0.3 * H * W and pairs[1] > 0.3 * H * W
        border = np.ones((H, W), bool)
        border[2:-2, 2:-2] = False
        assert masks[1][~border].any() and not masks[1].all()


def _crop(s, y, x, h, w):
    """The step's inputs cut to rows y .. y + h and columns x .. x + w, the principal point moved with them."""
    out = {k: np.ascontiguousarray(s[k][y:y + h, x:x + w]) for k in MAPS}
    out.update(pose=s["pose"], dist=s["dist"])
    K = np.array(s["K"], np.float32)
    K[0, 2], K[1, 2] = K[0, 2] - x, K[1, 2] - y
    return out, K


@pytest.mark.parametrize("h, w", [(13, 17), (17, 31), (3, 8), (4, 4)])
def test_rgbd_icp_step_on_crops(gpu_ctx, scenes, h, w):
    """H W below 256, H W no multiple of 256, a picture too small for a photometric cell, and the smallest one that has a cell (x0 = y0 = 1)."""
    s = scenes[(48, 64)]
    maps, K = _crop(s, 16, 20, h, w)
    for est in (s["pose"], s["est_2"]):
        sums, pairs, _ = _check_step(gpu_ctx, maps, K, est)
        assert pairs[0] > 0
        if h < 4:
            assert pairs[1] == 0 and not sums[28:].any()
        elif h > 4:
            assert pairs[1] > 0


def test_rgbd_icp_step_with_model_holes_and_without_a_model(gpu_ctx, scenes, oracle_lib):
    """The volume seen from outside has holes in its ray cast: pixels beside a hole are rejected.  Seen from a pose that looks away nothing is hit: no pairs
    of either kind and sums of zeros."""
    H, W = 48, 64
    s = scenes[(H, W)]
    for pose, empty in ((tc.outside_pose(), False), (tc.away_pose(), True)):
        maps = dict(dist=s["dist"], pose=pose)
        maps["model_d"], maps["model_v"], maps["model_n"], maps["model_c"] = tr.raycast_oracle(s["vol"], s["K"], pose, (H, W))
        hit = maps["model_d"] > 0
        if empty:
            assert not hit.any()
            maps.update({k: s[k] for k in ("live_v", "live_n", "live_i")})
        else:  # the live frame is the model's own picture
            assert hit.any() and not hit.all()
            _, Vs, Ns, _ = tr.frame_maps(maps["model_d"], s["K"], 1)
            maps.update(live_v=Vs[0], live_n=Ns[0], live_i=pr.gray(maps["model_c"]))
        sums, pairs, masks = _check_step(gpu_ctx, maps, s["K"], pose, pose)
        if empty:
            assert pairs == (0, 0) and not sums.any()
        else:
            inner = np.zeros((H, W), bool)
            inner[2:-2, 2:-2] = True
            assert 0 < pairs[1] < int((hit & inner).sum())  # pixels with a hit away from the border that a neighbouring hole rejects


def _device_volume(gpu_ctx, ora):
    from hive_amd import fusion
    dev = fusion.TSDFVolume(tc.bounds(), ora._voxel_size, ctx=gpu_ctx)
    assert tuple(dev.vol_dim) == ora._tsdf.shape
    dev.set_volume(ora._tsdf, ora._color, ora._weight)
    return dev


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("size", [(24, 32), (48, 64)])
def test_icp_align_with_colour_against_the_restatement(gpu_ctx, scenes, size):
    """The tolerance and the fields of test_tracking_gpu.py's test_icp_align_against_the_restatement; with a weight of 0 the colour changes nothing."""
    from hive_amd import tracking
    s = scenes[size]
    H, W = size
    volume = _device_volume(gpu_ctx, s["vol"])
    want = pr.icp_align(s["vol"], s["depth"], s["K"], s["pose"], color=s["color"], photometric_weight=0.1, max_cond=tracking.DEFAULT_MAX_COND)
    got = tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx, color=s["color"], photometric_weight=0.1)
    assert got.ok and want["ok"] and got.iterations_run == want["iterations_run"] == 19
    rel = 10 * max(want["conds"]) * (H * W) * 2.0 ** -52
    diff = np.abs(got.pose - want["pose"]).max() / np.abs(want["pose"]).max()
    err = float(np.linalg.norm(got.pose[:3, 3] - s["moved"][:3, 3]) / (tc.VOLUME / s["voxels"]))
    print(f"{size}: pose difference {diff:.3g} relative (bound {rel:.3g}), error against the true pose {err:.4f} voxel, cond(A) {got.cond:.3g}, pairs {got.pairs}")
    assert diff <= rel
    assert err <= 2 * pc.TWO_WALL_MEASURED_VOXELS[(H, W, s["voxels"])]
    assert got.pairs == want["pairs"] and got.cond < tracking.DEFAULT_MAX_COND
    plain = tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx)
    zero = tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx, color=s["color"], photometric_weight=0.0)
    assert not plain.ok and _same(plain, zero)


def test_a_weight_of_zero_changes_nothing_on_the_corner_scene(gpu_ctx, oracle_lib):
    """Where geometry alone tracks: the same bits with and without a colour at weight 0, and other bits at weight 0.1."""
    from hive_amd import tracking
    H, W, voxels = 24, 32, 32
    s = tr.icp_scene(oracle_lib, H, W, voxels)
    color = tc.room_frame(s["orbit"][1], s["K"], H, W, seed=1)[0]
    volume = _device_volume(gpu_ctx, s["vol"])
    plain = tracking.icp_align(volume, s["depth"], s["K"], s["orbit"][0], ctx=gpu_ctx)
    zero = tracking.icp_align(volume, s["depth"], s["K"], s["orbit"][0], ctx=gpu_ctx, color=color, photometric_weight=0.0)
    some = tracking.icp_align(volume, s["depth"], s["K"], s["orbit"][0], ctx=gpu_ctx, color=color, photometric_weight=0.1)
    assert plain.ok and some.ok and _same(plain, zero) and not np.array_equal(plain.pose, some.pose)


def test_track_and_fuse_on_the_two_wall_slide(gpu_ctx):
    """8 poses at 48 x 64 into 64^3, 2 levels.  With weight 0.1 the same loop restated on the CPU (tests/test_photometric_cpu.py) has an ATE RMSE of 1.194 mm;
    the bound is twice that, as for the corner orbit.  Geometry alone loses every frame after the first: the test that fails without the feature."""
    from hive_amd import tracking
    poses = pc.slide_poses()
    K, colors, depths = pc.frames(poses)
    _, _, results = tracking.track_and_fuse(colors, depths, K, tc.bounds(), tc.VOLUME / 64, first_pose=poses[0], levels=2)
    assert results[0].ok and not any(r.ok for r in results[1:])
    assert "photometric_weight" in inspect.signature(tracking.icp_align).parameters
    volume, trajectory, results = tracking.track_and_fuse(colors, depths, K, tc.bounds(), tc.VOLUME / 64, first_pose=poses[0], levels=2, photometric_weight=0.1)
    got = np.linalg.inv(trajectory.to_homogenous_transforms())
    rmse = pc.ate_rmse(poses, got)
    print(f"ATE RMSE {rmse * 1000:.3f} mm, cond(A) up to {max(r.cond for r in results):.3g}")
    assert all(r.ok for r in results) and len(trajectory) == 8
    assert rmse <= 2 * pc.SLIDE_ATE[0.1]
    assert volume.stats()[0] == 8


def test_argument_errors(gpu_ctx, scenes):
    from hive_amd import tracking
    s = scenes[(24, 32)]
    volume = _device_volume(gpu_ctx, s["vol"])
    with pytest.raises(ValueError):
        tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx, color=s["color"], photometric_weight=-0.1)
    with pytest.raises(ValueError):
        tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx, color=s["color"][:, :-1], photometric_weight=0.1)
    with pytest.raises(ValueError):
        tracking.icp_align(volume, s["depth"], s["K"], s["pose"], ctx=gpu_ctx, color=s["color"].astype(np.float32), photometric_weight=0.1)
    tracker = tracking.Tracker(volume, s["K"], s["pose"], photometric_weight=-1.0)
    tracker.frames = 1
    with pytest.raises(ValueError):
        tracker.step(s["color"], s["depth"])
