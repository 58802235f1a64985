"""csrc/track.hip and hive_amd/tracking.py on the GPU against the numpy restatements (tests/tracking_restatement.py): the frame maps bit for bit, the ICP sums
inside the float64 summation bound with the pairs exact, ``icp_align`` and the track-and-fuse loop against the same loops restated on the CPU, and what a lost
frame leaves behind.  Scenes: tests/tracking_cases.py; the bounds that come from CPU measurements are written there."""
import os

import numpy as np
import pytest

import tracking_cases as tc
import tracking_restatement as tr

pytestmark = pytest.mark.gpu

IMAGES = [(1, 1), (5, 7), (24, 32), (47, 63), (48, 64)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _live_depth(H, W):
    """The corner view with 2 % of its pixels zeroed, a block of zeros, and a depth step inside a 2 x 2 block on either side of pyr_delta = 0.05."""
    depth = tc.room_depth(tc.corner_orbit(12)[1], tc.intrinsics(H, W), H, W)[0].copy()
    rng = np.random.default_rng(H * 1000 + W)
    depth[rng.random(depth.shape) < 0.02] = 0.0
    if H >= 12 and W >= 12:
        depth[4:8, 4:8] = 0.0                                   # whole blocks of zeros at every level
        depth[8:10, 0:2] = [[1.0, 1.04], [1.0, 1.06]]           # 1.06 is left out, 1.04 is averaged
        depth[10:12, 0:2] = [[0.0, 1.3], [1.3499, 1.3501]]      # the nearest sample is not the first; 1.3501 - 1.3 is beyond 0.05 in float32
    return depth


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("size", IMAGES)
def test_frame_maps_match_the_restatement_bit_for_bit(gpu_ctx, size, levels):
    from hive_amd import tracking
    H, W = size
    if (H >> (levels - 1)) == 0 or (W >> (levels - 1)) == 0:
        with pytest.raises(ValueError):
            tracking.frame_maps(np.ones(size, np.float32), tc.intrinsics(H, W), levels, ctx=gpu_ctx)
        return
    depth, K = _live_depth(H, W), tc.intrinsics(H, W)
    want_d, want_v, want_n, want_K = tr.frame_maps(depth, K, levels, 0.05)
    got = tracking.frame_maps(depth, K, levels, 0.05, ctx=gpu_ctx)
    assert np.array_equal(_bits(got.K), _bits(want_K))
    for l in range(levels):
        assert got.sizes[l] == want_d[l].shape == (H >> l, W >> l)
        for name, g, w in (("depth", got.depth[l], want_d[l]), ("vertex", got.vertex[l], want_v[l]), ("normal", got.normal[l], want_n[l])):
            g = g.cpu().numpy()
            assert np.array_equal(_bits(g), _bits(w)), (size, l, name, int((_bits(g) != _bits(w)).sum()))
    if min(H, W) >= 24:
        assert np.abs(want_n[levels - 1]).sum(axis=-1).astype(bool).mean() > 0.5  # the maps are not empty


@pytest.fixture(scope="module")
def icp_scenes(oracle_lib):
    """(H, W) -> the corner scene at that size: K, an oracle volume with the first orbit frame, the restated model maps at its pose, the live maps of the
    second orbit frame."""
    out = {}
    for H, W, voxels in ((24, 32, 32), (47, 63, 64), (48, 64, 64)):
        out[(H, W)] = tr.icp_scene(oracle_lib, H, W, voxels)
    return out


def _device_volume(gpu_ctx, ora):
    from hive_amd import fusion
    dev = fusion.TSDFVolume(tc.bounds(), ora._voxel_size, ctx=gpu_ctx)
    assert tuple(dev.vol_dim) == ora._tsdf.shape
    dev.set_volume(ora._tsdf, ora._color, ora._weight)
    return dev


@pytest.mark.parametrize("size", [(24, 32), (47, 63)])
def test_icp_step_sums_and_pairs(gpu_ctx, icp_scenes, size):
    import torch
    from hive_amd import tracking
    s = icp_scenes[size]
    H, W = size
    dist, cos_min = 2 * s["vol"]._trunc_margin, float(np.cos(np.deg2rad(20.0)))
    dev = [torch.from_numpy(s[k]).cuda() for k in ("live_v", "live_n", "model_v", "model_n")]
    model_pose = s["orbit"][0]
    for est in (s["orbit"][0], s["orbit"][1]):  # the start of the alignment and its goal
        terms, mask = tr.icp_terms(s["K"], s["live_v"], s["live_n"], s["model_v"], s["model_n"], model_pose, est, dist, cos_min)
        want, want_pairs = tr.icp_sums(terms)
        got_mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        got, pairs = tracking.icp_step(gpu_ctx, s["K"], *dev, model_pose, est, dist, cos_min, pair_mask=got_mask)
        again, pairs_again = tracking.icp_step(gpu_ctx, s["K"], *dev, model_pose, est, dist, cos_min)
        assert pairs == want_pairs == int(mask.sum()) == pairs_again and pairs > 0.3 * H * W
        assert np.array_equal(got_mask.cpu().numpy().astype(bool), mask)
        bound = terms.shape[0] * 2.0 ** -52 * np.abs(terms[:, :28]).sum(axis=0)  # the float64 summation bound, n 2^-52 sum |term|
        print(f"{size}: pairs {pairs}, largest |difference| / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3g}")
        assert np.all(np.abs(got - want) <= bound)
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    far = s["orbit"][0].copy()
    far[:3, 3] += [5.0, -3.0, 4.0]
    sums, pairs = tracking.icp_step(gpu_ctx, s["K"], *dev, model_pose, far, dist, cos_min)
    assert pairs == 0 and not sums.any() and not np.isnan(sums).any()


@pytest.mark.parametrize("size", [(24, 32), (48, 64)])
def test_icp_align_against_the_restatement(gpu_ctx, icp_scenes, size):
    from hive_amd import tracking
    s = icp_scenes[size]
    H, W = size
    want = tr.icp_align(s["vol"], s["depth"], s["K"], s["orbit"][0], max_cond=tracking.DEFAULT_MAX_COND)
    got = tracking.icp_align(_device_volume(gpu_ctx, s["vol"]), s["depth"], s["K"], s["orbit"][0], ctx=gpu_ctx)
    assert got.ok and want["ok"] and got.iterations_run == want["iterations_run"] == 19
    rel = 10 * max(want["conds"]) * (H * W) * 2.0 ** -52
    diff = np.abs(got.pose - want["pose"]).max() / np.abs(want["pose"]).max()
    err = float(np.linalg.norm(got.pose[:3, 3] - s["orbit"][1][:3, 3]) / (tc.VOLUME / s["voxels"]))
    print(f"{size}: pose difference {diff:.3g} relative (bound {rel:.3g}), error against the true pose {err:.4f} voxel, cond(A) {got.cond:.3g}, pairs {got.pairs}")
    assert diff <= rel
    assert err <= 2 * tc.ICP_MEASURED_VOXELS[(H, W, s["voxels"])]
    assert got.pairs == want["pairs"]


def _orbit_frames(n, H=48, W=64):
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    frames = [tc.room_frame(p, K, H, W, seed=i) for i, p in enumerate(orbit[:n])]
    return K, orbit[:n], [f[0] for f in frames], [f[1] for f in frames]


def _ate_rmse(truth_c2w, trajectory):
    from hive_amd.geometric import Trajectory
    ate = Trajectory.from_homogenous_transforms(np.linalg.inv(truth_c2w)).calculate_ate(trajectory)
    return float(np.sqrt(np.mean(np.sum(ate ** 2, axis=1))))


def test_track_and_fuse_on_the_corner_orbit(gpu_ctx):
    """48 x 64 into 64^3, 2 levels.  The same loop restated on the CPU (tests/test_tracking_cpu.py) has an ATE RMSE of 0.632 mm; the bound is twice that,
    because an association can flip on the last bit of a sum."""
    from hive_amd import tracking
    K, orbit, colors, depths = _orbit_frames(12)
    volume, trajectory, results = tracking.track_and_fuse(colors, depths, K, tc.bounds(), tc.VOLUME / 64, first_pose=orbit[0], levels=2)
    rmse = _ate_rmse(orbit, trajectory)
    print(f"ATE RMSE {rmse * 1000:.3f} mm, cond(A) up to {max(r.cond for r in results):.3g}")
    assert all(r.ok for r in results) and len(trajectory) == 12
    assert rmse <= 2 * tc.TRACK_ATE_12
    assert volume.stats()[0] == sum(r.ok for r in results) == 12


def test_lost_frames_leave_pose_and_volume_alone(gpu_ctx):
    """A frame of another place (the two-wall view) and an all-zero depth frame in the middle of the orbit: lost, nothing raised, nothing integrated, the
    pose kept; the next orbit frame tracks again."""
    from hive_amd import fusion, tracking
    K, orbit, colors, depths = _orbit_frames(4)
    volume = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / 64, ctx=gpu_ctx)
    tracker = tracking.Tracker(volume, K, orbit[0], levels=2)
    assert tracker.step(colors[0], depths[0]).ok and tracker.step(colors[1], depths[1]).ok
    pose, stats, planes = tracker.pose.copy(), volume.stats(), volume.get_volume(with_weight=True)
    elsewhere = tc.room_frame(tc.two_wall_pose(), K, 48, 64)
    for color, depth in (elsewhere, (colors[2], np.zeros_like(depths[2]))):
        res = tracker.step(color, depth)
        assert not res.ok and np.array_equal(res.pose, pose) and np.array_equal(tracker.pose, pose)
        assert volume.stats() == stats
        assert all(np.array_equal(a, b) for a, b in zip(volume.get_volume(with_weight=True), planes))
    assert res.pairs == 0
    res = tracker.step(colors[2], depths[2])
    assert res.ok and volume.stats()[0] == 3 and not np.array_equal(tracker.pose, pose)


def test_two_wall_view_is_lost_through_max_cond(gpu_ctx):
    """A tracker whose last good pose sees two walls only: the next frame has pairs enough and a singular A, as in the restatement."""
    from hive_amd import fusion, tracking
    H, W = 48, 64
    K, pose = tc.intrinsics(H, W), tc.two_wall_pose()
    moved = pose.copy()
    moved[:3, 3] += [0.010, 0.012, -0.008]
    volume = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / 64, ctx=gpu_ctx)
    tracker = tracking.Tracker(volume, K, pose)
    assert tracker.step(*tc.room_frame(pose, K, H, W)).ok
    stats = volume.stats()
    res = tracker.step(*tc.room_frame(moved, K, H, W, seed=1))
    print(f"pairs {res.pairs}, cond(A) {res.cond:.3g}")
    assert not res.ok and np.array_equal(res.pose, pose) and volume.stats() == stats == (1, 1)
    assert res.pairs >= 0.1 * (H // 4) * (W // 4) and res.iterations_run == 1 and res.cond > tracking.DEFAULT_MAX_COND


class _SmallTUM:
    """Writes a TUM-layout sequence (rgb.txt, depth.txt, groundtruth.txt, rgb/, depth/ with 1 / 5000 m units) of the corner orbit at 48 x 64."""

    @staticmethod
    def write(base, poses, colors, depths):
        from PIL import Image
        from scipy.spatial.transform import Rotation
        os.makedirs(os.path.join(base, "rgb")), os.makedirs(os.path.join(base, "depth"))
        lines = {"rgb.txt": [], "depth.txt": [], "groundtruth.txt": []}
        for i, (pose, color, depth) in enumerate(zip(poses, colors, depths)):
            stamp = f"{1000.0 + i / 30.0:.6f}"
            Image.fromarray(color).save(os.path.join(base, "rgb", f"{stamp}.png"))
            Image.fromarray(np.rint(depth * 5000.0).astype(np.uint16)).save(os.path.join(base, "depth", f"{stamp}.png"))
            q = Rotation.from_matrix(pose[:3, :3]).as_quat()
            lines["rgb.txt"].append(f"{stamp} rgb/{stamp}.png")
            lines["depth.txt"].append(f"{stamp} depth/{stamp}.png")
            lines["groundtruth.txt"].append(f"{stamp} " + " ".join(f"{v:.9f}" for v in (*pose[:3, 3], *q)))
        for name, rows in lines.items():
            with open(os.path.join(base, name), "w") as f:
                f.write("# synthetic\n" + "\n".join(rows) + "\n")


def test_estimate_trajectory_on_a_tum_layout_dataset(gpu_ctx, tmp_path):
    """6 corner-orbit frames at 48 x 64 through the TUM adaptor (its intrinsics and size set for the small frames) and ``estimate_trajectory``: only the first
    pose of the dataset is used.  The ATE bound is the track-and-fuse test's: twice the CPU loop's ATE over these 6 frames (0.663 mm)."""
    from hive_amd import tracking
    from hive_amd.dataset_adaptors import TUMAdaptor
    from hive_amd.options import BackgroundMeshOptions
    K, orbit, colors, depths = _orbit_frames(6)

    class SmallTUM(TUMAdaptor):
        width, height = 64, 48
        intrinsic_matrix = K.astype(np.float64)

    _SmallTUM.write(str(tmp_path / "tum"), orbit, colors, depths)
    dataset = SmallTUM(str(tmp_path / "tum"), str(tmp_path / "hive")).convert()
    assert dataset.num_frames == 6
    volume, trajectory, results = tracking.estimate_trajectory(dataset, BackgroundMeshOptions(sdf_voxel_size=tc.VOLUME / 64), levels=2)
    truth = dataset.camera_trajectory
    ate = truth.calculate_ate(trajectory)
    rmse = float(np.sqrt(np.mean(np.sum(ate ** 2, axis=1))))
    print(f"ATE RMSE {rmse * 1000:.3f} mm over {len(trajectory)} frames, volume {tuple(volume.vol_dim)}")
    assert len(trajectory) == dataset.num_frames == len(results) and all(r.ok for r in results)
    assert np.allclose(trajectory.values[0], truth.values[0], atol=1e-6)
    assert rmse <= 2 * tc.TRACK_ATE_6
    assert volume.stats()[0] == 6
