"""Frame registration on the CPU: the numpy restatement of csrc/register.hip (tests/rigid_restatement.py) against other float64 algorithms, and
``registration.chain_pairs`` on hand-built graphs.  The restated Jacobi is compared with ``numpy.linalg.eigh``, the restated Horn solver with an SVD Kabsch /
Umeyama and with scipy's ``Rotation.align_vectors``: different algorithms, so each bound is four times the deviation measured here and written down in
tests/register_cases.py; every figure is printed before it is asserted.  Nothing here is pinned against cv2's estimateAffine3D, Open3D, BundleFusion or COLMAP."""
import numpy as np
import pytest

import ransac_restatement as RR
import register_cases as C
import rigid_restatement as GR


def kabsch(p, q, with_scale):
    """SVD Kabsch / Umeyama in plain numpy: (A = s R, t) with det R = +1."""
    cp, cq = p.mean(axis=0), q.mean(axis=0)
    dp, dq = p - cp, q - cq
    U, _, Vt = np.linalg.svd(dq.T @ dp)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    s = np.sqrt((dq * dq).sum() / (dp * dp).sum()) if with_scale else 1.0
    return s * R, cq - s * R @ cp


def solve(name):
    p, q, T, with_scale = C.horn_case(name)
    cp, cq, S, sp, sq = C.centred(p, q)
    A, t, scale, ok = GR.horn(cp[None], cq[None], S[None], np.array([sp]), np.array([sq]), with_scale)
    assert ok[0], name
    return p, q, T, with_scale, A[0], t[0], scale[0]


def test_sweeps_are_the_measured_number_plus_two():
    """The off-diagonal norm after every sweep, relative to the Frobenius norm, over the Horn matrices of all committed cases."""
    history = []
    GR.jacobi(C.horn_matrices(), 10, history)
    print("off-diagonal / Frobenius after sweep 1 ..:", ["%.2e" % h for h in history])
    first = next(k + 1 for k, h in enumerate(history) if h <= 2.0 ** -52)
    assert first == C.SWEEPS_MEASURED and GR.SWEEPS == C.SWEEPS_MEASURED + 2
    assert all(h <= 2.0 ** -52 for h in history[first - 1:])


def test_jacobi_against_eigh():
    N = C.horn_matrices()
    a, v = GR.jacobi(N)
    worst = 0.0
    for k in range(len(N)):
        _, e = np.linalg.eigh(N[k])
        x = v[k][:, int(np.argmax(np.diag(a[k])))]
        x = x / np.linalg.norm(x)
        worst = max(worst, min(np.abs(x - e[:, -1]).max(), np.abs(x + e[:, -1]).max()))
    print("eigenvector deviation over", len(N), "matrices:", worst)
    assert len(N) > 1000 and worst <= 4 * C.EIGENVECTOR_DEVIATION


def test_horn_against_kabsch_and_align_vectors():
    from scipy.spatial.transform import Rotation
    worst, worst_scipy, rotation_only = 0.0, 0.0, 0
    for name in sorted(C.HORN_CASES):
        p, q, T, with_scale, A, t, scale = solve(name)
        Ak, tk = kabsch(p, q, with_scale)
        worst = max(worst, np.abs(A - Ak).max(), np.abs(t - tk).max())
        assert abs(np.linalg.det(A / scale) - 1.0) < 1e-12, name  # a rotation, the mirrored set included
        if not with_scale:
            rot, _ = Rotation.align_vectors(q - q.mean(axis=0), p - p.mean(axis=0))
            worst_scipy = max(worst_scipy, np.abs(rot.as_matrix() - A).max())
            rotation_only += 1
    print("Kabsch deviation:", worst, " align_vectors deviation:", worst_scipy)
    assert rotation_only == len(C.HORN_CASES) - 2
    assert worst <= 4 * C.KABSCH_DEVIATION and worst_scipy <= 4 * C.ALIGN_VECTORS_DEVIATION


def test_horn_recovers_the_planted_transforms_and_their_scale():
    for name, bound in (("identity", 1e-15), ("quarter", 1e-7), ("half_turn", 1e-7), ("scaled", 1e-6), ("shrunk", 1e-6), ("minimal", 1e-6)):
        _, _, T, _, A, t, scale = solve(name)
        assert np.abs(A - T[:3, :3]).max() <= bound and np.abs(t - T[:3, 3]).max() <= bound, name
        assert abs(scale - C.HORN_CASES[name][4]) <= bound


def test_sign_rule_and_no_model():
    """w >= 0, and with w == 0 the first non-zero component is positive: a half turn about y from exact sums.  Zero spread or a NaN: no model."""
    p = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, -2.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    q = p * np.array([-1.0, 1.0, -1.0])
    cp, cq, S, sp, sq = C.centred(p, q)
    A, t, scale, ok = GR.horn(cp[None], cq[None], S[None], np.array([sp]), np.array([sq]), False)
    assert ok[0] and (A[0] == np.diag([-1.0, 1.0, -1.0])).all() and (t[0] == 0).all()
    same = np.ones((4, 3))
    for a, b in ((same, p[:4]), (p[:4], same)):
        cp, cq, S, sp, sq = C.centred(a, b)
        assert not GR.horn(cp[None], cq[None], S[None], np.array([sp]), np.array([sq]), True)[3][0]
    bad = p.copy()
    bad[2, 1] = np.nan
    cp, cq, S, sp, sq = C.centred(bad, q)
    assert not GR.horn(cp[None], cq[None], S[None], np.array([sp]), np.array([sq]), False)[3][0]


@pytest.mark.parametrize("M", (3, 4, 5, 64, 1000))
def test_draws_are_distinct_and_below_M(M):
    base = RR.base_key(3, (4, 9))
    s = GR.draw3(base, np.arange(4000), M)
    assert s.shape == (4000, 3) and s.min() >= 0 and s.max() < M
    assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()
    assert (s == RR.draw(base, np.arange(4000), max(M, 4))[:, :3]).all() or M < 4  # the first three of the four-draw rule
    if M == 3:
        assert (np.sort(s, axis=1) == np.arange(3)).all()
    else:
        assert len(np.unique(s)) == min(M, len(np.unique(s))) and len(np.unique(s)) > min(M, 64) // 2


def test_degeneracy_rule_on_both_sides_of_its_constant():
    """sin^2 of the angle at p0 against 2^-20: collinear and repeated points are rejected; a sample just on the accepting side, and its mirror just on the other."""
    p0, p1 = np.zeros(3), np.array([1.0, 0.0, 0.0])
    tri = lambda p2: np.stack([p0, p1, np.asarray(p2, dtype=np.float64)])[None]
    assert GR.degenerate(tri([2.0, 0.0, 0.0]))[0]          # collinear
    assert GR.degenerate(tri([1.0, 0.0, 0.0]))[0]          # two equal points
    assert GR.degenerate(np.zeros((1, 3, 3)))[0]           # all equal
    root = 2.0 ** -10                                      # sin = 2^-10 exactly on the rule's edge: tan slightly above / below it
    assert not GR.degenerate(tri([1.0, root * 1.001, 0.0]))[0]
    assert GR.degenerate(tri([1.0, root * 0.999, 0.0]))[0]
    assert not GR.degenerate(1000.0 * tri([1.0, root * 1.001, 0.0]))[0] and GR.degenerate(1e-3 * tri([1.0, root * 0.999, 0.0]))[0]  # scale-free
    # a degenerate sample on either side rejects the trial
    good, line = tri([0.3, 0.8, 0.1])[0], tri([2.0, 0.0, 0.0])[0]
    pts_p, pts_q = np.concatenate([good, line]), np.concatenate([good, good])
    for a, b in ((pts_p, pts_q), (pts_q, pts_p)):
        ok = GR.minimal(a, b, np.array([[0, 1, 2], [3, 4, 5]]), False)[3]
        assert ok.tolist() == [True, False]


@pytest.mark.parametrize("name", sorted(C.PLANTED))
def test_restated_ransac_finds_the_planted_transform(name):
    rows, camera, T, inliers, with_scale = C.planted(name)
    fit = C.restated_planted(name)
    deviation = np.abs(fit["T"][:3] - T[:3]).max()
    print(name, "trial", fit["trial"], "counts", fit["winner_count"], fit["count"], "deviation", deviation, "rms", fit["rms"])
    assert fit["trial"] >= 0 and deviation <= 4 * C.PLANTED_DEVIATION[name]
    if C.PLANTED[name][2] == 0.0:
        assert (fit["mask"].astype(bool) == inliers).all()
    assert (fit["T"][3] == [0, 0, 0, 1]).all() and (abs(fit["scale"] - 1.6) < 1e-6 if with_scale else fit["scale"] == 1.0)


def test_restated_ransac_without_a_model():
    rows = C.mixed(40)
    line = rows.copy()
    line[:, 0:3] = np.arange(40, dtype=np.float32)[:, None] * np.array([1.0, 2.0, 0.5], dtype=np.float32)
    same = rows.copy()
    same[:, 3:6] = 1.5
    for r, kw in ((line, {}), (same, {}), (rows[:2], {}), (rows, dict(min_count=41))):
        fit = GR.ransac(r, **kw)
        assert fit["trial"] == -1 and np.isnan(fit["T"]).all() and np.isnan(fit["rms"]) and np.isnan(fit["scale"]) and not fit["mask"].any()
    three = GR.ransac(rows[20:23], trials=50)  # every trial draws the same three points: the lowest trial wins
    assert three["trial"] == 0 and three["count"] == 3


# ---- chain_pairs ----
def _edge(T, count=50, trial=0):
    s = np.cbrt(np.linalg.det(T[:3, :3]))
    return T, s, [trial, count, count]


def _chain(n, edges, **kw):
    from hive_amd.registration import chain_pairs
    pairs = [e[0] for e in edges]
    parts = [_edge(*e[1:]) for e in edges]
    return chain_pairs(n, pairs, np.stack([p[0] for p in parts]), np.array([p[1] for p in parts]), np.array([p[2] for p in parts]), **kw)


def test_chain_forward_backward_and_lost():
    A, B = C.transform(C.rotation((0, 1, 0), 10.0), (0.1, 0.0, 0.0)), C.transform(C.rotation((1, 0, 0), -5.0), (0.0, 0.2, 0.05))
    first = C.transform(C.rotation((0, 0, 1), 30.0), (1.0, 2.0, 3.0))
    # 0 -> 1 forward, 2 reached only through the backward edge (2, 1), 3 has no edge with enough inliers, 4 has an edge without a model
    poses, lam, lost = _chain(5, [((0, 1), A), ((2, 1), B), ((1, 3), A, 19), ((3, 4), A, 50, -1)], first_pose=first)
    assert lost == [3, 4] and (lam == 1).all()
    assert np.allclose(poses[0], first, atol=0) and np.allclose(poses[1], A @ first, atol=1e-15)
    assert np.allclose(poses[2], np.linalg.inv(B) @ A @ first, atol=1e-15)
    assert (poses[3] == poses[2]).all() and (poses[4] == poses[2]).all()  # the nearest reached frame below
    # nothing below the lost frame: the nearest above
    poses, lam, lost = _chain(3, [((1, 2), A)], root=1)
    assert lost == [0] and (poses[0] == poses[1]).all() and (poses[1] == np.eye(4)).all() and np.allclose(poses[2], A, atol=1e-15)
    with pytest.raises(ValueError):
        _chain(2, [((0, 2), A)])


def test_chain_first_arrival_wins_in_the_stated_order():
    A, B, D = (C.transform(C.rotation((0, 1, 0), d), (0.1 * d, 0.0, 0.0)) for d in (4.0, 7.0, -3.0))
    wrong = C.transform(np.eye(3), (9.0, 9.0, 9.0))
    # frame 3 is reached from 1 and from 2 at the same depth: the frontier is taken in ascending frame index, so 1's edge wins although 2's comes first in the list
    poses, _, lost = _chain(4, [((2, 3), wrong), ((0, 2), B), ((0, 1), A), ((1, 3), D)])
    assert lost == [] and np.allclose(poses[3], D @ A, atol=1e-15) and np.allclose(poses[2], B, atol=1e-15)
    # two edges of one frame to the same target: the first in the pair list wins; a shorter route beats a longer one
    poses, _, _ = _chain(3, [((0, 1), A), ((0, 1), wrong), ((1, 2), D), ((0, 2), B)])
    assert np.allclose(poses[1], A, atol=1e-15) and np.allclose(poses[2], B, atol=1e-15)


def test_chain_scales_two_and_a_half_give_depth_scales_and_metric_translations():
    """Frame 1's depth is in half units (s = 2 maps frame 0's points onto frame 1's), frame 2's in double units of frame 1's (s = 0.5)."""
    R1, R2 = C.rotation((0, 1, 0), 8.0), C.rotation((1, 1, 0), -6.0)
    t1, t2 = np.array([0.2, -0.1, 0.4]), np.array([-0.3, 0.2, 0.1])  # in the target frame's own unit
    poses, lam, lost = _chain(3, [((0, 1), C.transform(R1, t1, 2.0)), ((1, 2), C.transform(R2, t2, 0.5))])
    assert lost == [] and lam.tolist() == [1.0, 0.5, 1.0]
    G1 = C.transform(R1, 0.5 * t1)
    assert np.allclose(poses[1], G1, atol=1e-15) and np.allclose(poses[2], C.transform(R2, 1.0 * t2) @ G1, atol=1e-15)
    # the same chain walked backwards from frame 2 gives the same relative poses and scales relative to frame 2
    back, lam_b, _ = _chain(3, [((0, 1), C.transform(R1, t1, 2.0)), ((1, 2), C.transform(R2, t2, 0.5))], root=2)
    assert np.allclose(lam_b, [1.0, 0.5, 1.0], atol=1e-15)
    assert np.allclose(back[1] @ np.linalg.inv(back[0]), poses[1] @ np.linalg.inv(poses[0]), atol=1e-14)
    # a metric point seen in every frame: lambda_f * (what frame f measures) = G_f applied to the world point
    x = np.array([0.3, -0.2, 2.0])
    in1 = 2.0 * R1 @ x + t1
    in2 = 0.5 * R2 @ in1 + t2
    for f, seen in ((1, in1), (2, in2)):
        assert np.allclose(lam[f] * seen, poses[f][:3, :3] @ x + poses[f][:3, 3], atol=1e-14)


# ---- the synthetic orbit ----
def test_orbit_trajectory_from_the_restated_ransac():
    o = C.orbit()
    fits, poses, lam, lost = C.restated_orbit()
    assert len(o["pairs"]) == 19 and all(len(r) >= 100 for r in o["rows"])
    assert all(f["trial"] >= 0 and f["count"] >= C.ORBIT_MIN_INLIERS for f in fits)  # with these seeds every pair finds a model
    for f, r in zip(fits, o["rows"]):
        assert 0.55 * len(r) <= f["count"] <= 0.65 * len(r)  # the 60 % that were not replaced
    ate = C.ate_rmse(poses, o["poses"])
    print("orbit ATE RMSE:", ate, "m")
    assert lost == [] and (lam == 1).all() and ate <= 4 * C.ORBIT_ATE


def test_restated_pipeline_on_the_pixel_shift():
    m, fit = C.restated_shift()
    dt, dR = np.abs(fit["T"][:3, 3] - C.shift_expected()).max(), np.abs(fit["T"][:3, :3] - np.eye(3)).max()
    print("survivors", m["survivors"], "inliers", fit["count"], "translation deviation", dt, "rotation deviation", dR)
    assert fit["trial"] >= 0 and fit["count"] >= 10 and max(dt, dR) <= 4 * C.SHIFT_DEVIATION


# ---- the symbol ----
def test_symbol_and_abi():
    import ctypes

    from hive_amd import _lib
    assert _lib.ABI_VERSION == 9 and "hive_ransac_rigid" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["hive_ransac_rigid"]
    assert restype is ctypes.c_int and len(args) == 19 and args[8] == ctypes.POINTER(ctypes.c_double)


def test_python_entry_points_exist():
    import inspect

    from hive_amd import features, registration
    from hive_amd.pose_optimisation import FeatureExtractor, FrameSamplingMode
    assert list(inspect.signature(features.ransac_rigid).parameters) == ["rows", "counts", "keys", "camera_matrix", "threshold", "trials", "seed", "min_count", "with_scale", "ctx"]
    assert list(inspect.signature(features.estimate_rigid_transform).parameters) == ["points_i", "points_j", "threshold", "trials", "seed", "pair_key", "with_scale",
                                                                                    "return_stats", "ctx"]
    sig = inspect.signature(registration.estimate_trajectory)
    assert sig.parameters["frame_sampling"].default is FrameSamplingMode.Hierarchical and sig.parameters["threshold"].default == 0.05
    assert registration.RegistrationResult._fields == ("trajectory", "depth_scale", "lost", "pair_stats", "pair_transforms", "feature_set")
    init = inspect.signature(FeatureExtractor.__init__).parameters
    assert init["model"].default == "homography" and init["rigid_threshold"].default == 0.05 and init["with_scale"].default is False
    with pytest.raises(ValueError, match="model"):
        FeatureExtractor(None, [], model="affine")


def test_tum_adaptor_still_refuses_what_is_out_of_scope(tmp_path):
    """``estimate_pose`` with ``estimate_depth`` (per-frame depth scales before fusion) and ``static_camera`` keep raising, before anything is written."""
    import os

    from tum_fixture import write_tum_sequence
    from hive_amd.dataset_adaptors import TUMAdaptor
    tum, out = str(tmp_path / "tum"), str(tmp_path / "hive")
    write_tum_sequence(tum, num_frames=2)
    adaptor = TUMAdaptor(tum, out)
    with pytest.raises(NotImplementedError, match="depth scales"):
        adaptor.convert(estimate_pose=True, estimate_depth=True)
    with pytest.raises(NotImplementedError, match="static-camera"):
        adaptor.convert(estimate_pose=True, static_camera=True)
    assert not os.path.exists(out)
