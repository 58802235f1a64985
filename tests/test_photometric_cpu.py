"""The photometric term's rules themselves, without a GPU: the numpy restatement (tests/photometric_restatement.py) over oracle volumes of the small room
(tests/photometric_cases.py) against the true poses.  What csrc/track.hip is then held to bit for bit (tests/test_photometric_gpu.py) is shown here to be worth
matching: colour keeps the two-wall view tracked, and costs accuracy on the corner orbit when it is weighted heavily.  Every figure is printed before it is
asserted; the written ones are in photometric_cases.py."""
import os
import re

import numpy as np
import pytest

import photometric_cases as pc
import photometric_restatement as pr
import tracking_cases as tc
import tracking_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def translation_error_voxels(pose, truth, voxels):
    return float(np.linalg.norm(pose[:3, 3] - truth[:3, 3]) / (tc.VOLUME / voxels))


@pytest.mark.parametrize("H, W, voxels", [(24, 32, 32), (48, 64, 64)])
def test_two_wall_alignment_holds_with_colour(oracle_lib, H, W, voxels):
    """The two-wall frame fused, the frame 17.5 mm away aligned from its pose with defaults: lost without colour (as tracking_restatement has it), found with
    photometric_weight = 0.1, with cond(A) of the combined equations under the default gate at every step."""
    from hive_amd import tracking
    s = pc.two_wall_scene(oracle_lib, H, W, voxels)
    res = pr.icp_align(s["vol"], s["depth"], s["K"], s["pose"], color=s["color"], photometric_weight=0.1, max_cond=tracking.DEFAULT_MAX_COND)
    err, start = translation_error_voxels(res["pose"], s["moved"], voxels), translation_error_voxels(s["pose"], s["moved"], voxels)
    print(f"{H} x {W} into {voxels}^3, weight 0.1: {start:.3f} -> {err:.4f} voxel, pairs {res['pairs']}, cond(A) {min(res['conds']):.3g} .. {max(res['conds']):.3g}")
    assert res["ok"] and res["iterations_run"] == 19
    assert err <= 2 * pc.TWO_WALL_MEASURED_VOXELS[(H, W, voxels)]
    assert max(res["conds"]) < tracking.DEFAULT_MAX_COND
    assert max(res["conds"]) <= pc.TWO_WALL_COND_MAX_SEEN[(H, W, voxels)] * 1.01
    want = tr.icp_align(s["vol"], s["depth"], s["K"], s["pose"], max_cond=tracking.DEFAULT_MAX_COND)
    none = pr.icp_align(s["vol"], s["depth"], s["K"], s["pose"], color=s["color"], photometric_weight=0.0, max_cond=tracking.DEFAULT_MAX_COND)
    print(f"weight 0: ok {none['ok']}, cond(A) {none['cond']:.3g}")
    assert not none["ok"] and not want["ok"] and np.array_equal(none["pose"], want["pose"]) and np.array_equal(none["pose"], s["pose"])
    assert {k: v for k, v in none.items() if k != "pose"} == {k: v for k, v in want.items() if k != "pose"}


@pytest.fixture(scope="module")
def slide():
    poses = pc.slide_poses()
    return (poses, *pc.frames(poses))


@pytest.fixture(scope="module")
def orbit():
    poses = tc.corner_orbit(12)
    return (poses, *pc.frames(poses))


@pytest.mark.parametrize("weight", pc.WEIGHTS)
def test_two_wall_slide_on_the_cpu(oracle_lib, slide, weight):
    """8 poses sliding past the walls' edge, 48 x 64 into 64^3, 2 levels: frames 2 .. 8 are tracked against a model fused from tracked poses.  Below one voxel
    is a condition, not a measurement: the model's colour is per voxel, so sub-voxel is the bar."""
    from hive_amd import tracking
    poses, K, colors, depths = slide
    _, got, results = pr.track_and_fuse(oracle_lib, colors, depths, K, tc.bounds(), tc.VOLUME / 64, poses[0], photometric_weight=weight, levels=2,
                                        max_cond=tracking.DEFAULT_MAX_COND)
    rmse = pc.ate_rmse(poses, got)
    print(f"slide, weight {weight}: ATE RMSE {rmse * 1000:.3f} mm, ok {[r['ok'] for r in results]}, cond(A) up to {max(max(r['conds']) for r in results[1:]):.3g}")
    assert all(r["ok"] for r in results)
    assert rmse <= 1.25 * pc.SLIDE_ATE[weight]  # the figure written is this run's, give or take the host's LAPACK
    assert rmse < tc.VOLUME / 64


def test_two_wall_slide_is_lost_without_colour(oracle_lib, slide):
    from hive_amd import tracking
    poses, K, colors, depths = slide
    _, got, results = pr.track_and_fuse(oracle_lib, colors, depths, K, tc.bounds(), tc.VOLUME / 64, poses[0], levels=2, max_cond=tracking.DEFAULT_MAX_COND)
    print(f"slide, no colour: ok {[r['ok'] for r in results]}")
    assert results[0]["ok"] and not any(r["ok"] for r in results[1:])
    assert all(np.array_equal(p, poses[0]) for p in got)


@pytest.mark.parametrize("weight", pc.WEIGHTS)
def test_corner_orbit_with_colour_on_the_cpu(oracle_lib, orbit, weight):
    """The 12-pose corner orbit, where geometry fixes the pose already.  A finding, not a gain: the model's colour is the nearest voxel's and the frames carry
    noise of sigma 4 grey levels, so a heavy colour term costs accuracy (0.632 mm without colour, 0.637 mm at 0.03, 2.07 mm at 0.1).  Hence off by default."""
    from hive_amd import tracking
    poses, K, colors, depths = orbit
    _, got, results = pr.track_and_fuse(oracle_lib, colors, depths, K, tc.bounds(), tc.VOLUME / 64, poses[0], photometric_weight=weight, levels=2,
                                        max_cond=tracking.DEFAULT_MAX_COND)
    rmse = pc.ate_rmse(poses, got)
    print(f"orbit, weight {weight}: ATE RMSE {rmse * 1000:.3f} mm (geometry alone: {tc.TRACK_ATE_12 * 1000:.3f} mm)")
    assert all(r["ok"] for r in results)
    assert rmse <= 1.25 * pc.ORBIT_ATE[weight]


def test_minus_jacobian_is_the_residuals_derivative(oracle_lib):
    """-J is the derivative of r by xi (the update is T <- exp(xi) T): central differences of the restated residual over 50 kept pixels.

    The model's intensity is the plane I(x, y) = x / 64 + y / 128 (exact in float32), so that bilinear sampling and the central-difference gradients are
    exact and r is a smooth function of xi; the live intensity is the model's own, shifted by 0.25.  With step h the differences are off by (h^2 / 6) |r'''|
    plus rounding of 2 ulp(|r|) / (2 h).  r = I_live - (gu pu + gv pv + const) with pu = fx X / Z + cx: along xi_i the point moves on a circle or a line, so
    the k-th derivatives of X and Z are at most L = max(1, |q|, |c|), and with m = L / min Z >= 1 the third derivative of X / Z is at most
    m + 3 m^2 + 3 m^2 + 6 m^3 + m^2 + 6 m^3 + 6 m^4 <= 26 m^4.  The tolerance is that bound; it is about 1e-5 of |J|."""
    H, W, voxels, h = 48, 64, 64, 1e-4
    s = pc.two_wall_scene(oracle_lib, H, W, voxels)
    depth_m, _, _, _ = tr.raycast_oracle(s["vol"], s["K"], s["pose"], (H, W))
    _, Vs, _, _ = tr.frame_maps(s["depth"], s["K"], 1)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    gu, gv = 1.0 / 64, 1.0 / 128
    model_I = (u * np.float32(gu) + v * np.float32(gv)).astype(np.float32)
    live_I = (model_I + np.float32(0.25)).astype(np.float32)
    dist = 2 * s["vol"]._trunc_margin

    def residual(est):
        d = {}
        _, mask = pr.photo_terms(s["K"], Vs[0], live_I, model_I, depth_m, s["pose"], est, dist, details=d)
        return d["r"], d["J"], mask.reshape(-1)

    est = tr.se3_exp(np.array([0.004, -0.003, 0.002, 0.003, -0.002, 0.004])) @ s["moved"]
    r0, J, keep = residual(est)
    diffs = []
    for i in range(6):
        xi = np.zeros(6)
        xi[i] = h
        rp, _, kp = residual(tr.se3_exp(xi) @ est)
        rm, _, km = residual(tr.se3_exp(-xi) @ est)
        keep = keep & kp & km
        diffs.append((rp - rm) / (2 * h))
    picked = np.flatnonzero(keep)
    picked = picked[np.linspace(0, len(picked) - 1, 50).astype(int)]
    assert len(np.unique(picked)) == 50
    fd, J = np.stack(diffs, axis=1)[picked], J[picked]
    Kd = np.asarray(s["K"], np.float64)
    q = (est[:3, :3] @ Vs[0].reshape(-1, 3)[picked].astype(np.float64).T).T + est[:3, 3]
    c = (np.linalg.inv(s["pose"])[:3, :3] @ q.T).T + np.linalg.inv(s["pose"])[:3, 3]
    m = max(1.0, np.linalg.norm(q, axis=1).max(), np.linalg.norm(c, axis=1).max()) / c[:, 2].min()
    tol = (h * h / 6) * (gu * Kd[0, 0] + gv * Kd[1, 1]) * 26 * m ** 4 + 2 * 2.0 ** -52 * np.abs(r0[picked]).max() / (2 * h)
    worst = np.abs(fd + J).max()
    print(f"50 of {int(keep.sum())} kept pixels: |J| up to {np.abs(J).max():.3g}, largest |difference| {worst:.3g}, tolerance {tol:.3g} (m = {m:.3g})")
    assert m >= 1 and np.abs(J).max() > 0.1
    assert worst <= tol


def test_gray_rules():
    """The integer luma and the plain 2 x 2 mean, by hand."""
    c = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0]],
                  [[0, 0, 255], [1, 2, 3], [10, 20, 30], [200, 100, 50]]], np.uint8)
    assert pr.luma(c).tolist() == [[255, 0, 76, 150], [29, 2, 18, 124]]
    I = pr.gray_pyramid(c, 2)
    assert I[0].dtype == np.float32 and I[0][0, 2] == np.float32(76) / np.float32(255)
    assert I[1].shape == (1, 2) and I[1][0, 0] == ((I[0][0, 0] + I[0][0, 1]) + (I[0][1, 0] + I[0][1, 1])) * np.float32(0.25)
    assert pr.gray_pyramid(np.zeros((5, 7, 3), np.uint8), 2)[1].shape == (2, 3)


def test_small_pictures_have_no_photometric_pairs():
    V = np.ones((3, 8, 3), np.float32)
    terms, mask = pr.photo_terms(tc.intrinsics(3, 8), V, np.ones((3, 8), np.float32), np.ones((3, 8), np.float32), np.ones((3, 8), np.float32), np.eye(4), np.eye(4), 1.0)
    assert not mask.any() and not terms.any()


def test_entry_points_are_declared():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    exported = open(os.path.join(ROOT, "hive_amd", "csrc", "track.hip")).read()
    exported = exported[exported.index('extern "C"'):]
    for name in ("hive_gray_pyramid", "hive_rgbd_icp_step"):
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert re.search(rf"^int {name}\(", exported, flags=re.M), name
    assert len(_lib.SIGNATURES["hive_rgbd_icp_step"][1]) == 19 and len(_lib.SIGNATURES["hive_gray_pyramid"][1]) == 6
    assert re.search(r"^#define HIVE_ABI_VERSION 9$", header, flags=re.M) and _lib.ABI_VERSION == 9


def test_arguments_without_a_gpu():
    """The new keywords exist, and the weight is checked before anything touches the device."""
    import inspect
    from hive_amd import tracking
    params = inspect.signature(tracking.icp_align).parameters
    assert params["color"].default is None and params["photometric_weight"].default == 0.0
    assert tracking.TrackResult._fields == ("pose", "ok", "pairs", "rmse", "cond", "iterations_run")
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            tracking.icp_align(None, np.ones((4, 4), np.float32), np.eye(3), np.eye(4), ctx=object(), photometric_weight=bad)
    sums = np.arange(56, dtype=np.float64)
    both = tracking.combined_sums(sums, 0.5)
    assert np.array_equal(both[:27], sums[:27] + 0.25 * sums[28:55]) and both[27] == 27 and both.shape == (28,)
    assert np.array_equal(both, pr.combine(sums, 0.5))
