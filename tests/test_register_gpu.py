"""Frame registration on the GPU (csrc/register.hip behind hive_amd.features, hive_amd.pose_optimisation and hive_amd.registration) against the numpy restatement
(tests/rigid_restatement.py), bit for bit: T, scale, rms, the inlier mask, the winning trial and the counts.  The cases and the CPU-measured bounds are those of
tests/register_cases.py, which tests/test_register_cpu.py proves.  Not pinned against cv2's estimateAffine3D, Open3D, BundleFusion or COLMAP: all absent."""
import numpy as np
import pytest

import register_cases as C
import rigid_restatement as GR

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _run(cases, stride=None, camera=None, words=None, column=False, **kw):
    """``cases``: [(rows float32 (M, w), key)] as ONE batch under one stride; rows past a pair's count hold NaN, so a read of them shows.  ``column``: the counts
    as a column view two words apart.  -> numpy (T, scale, rms, mask, result)."""
    import torch
    from hive_amd.features import ransac_rigid
    stride = stride or max(max(len(c[0]) for c in cases), 1)
    words = words or max(c[0].shape[1] for c in cases)
    rows = np.full((len(cases), stride, words), np.nan, dtype=np.float32)
    for p, (r, _) in enumerate(cases):
        rows[p, :len(r), :r.shape[1]] = r
    counts = np.array([len(c[0]) for c in cases], dtype=np.int32)
    if column:
        counts_d = torch.from_numpy(np.stack([np.full_like(counts, -7), counts], axis=1)).cuda()[:, 1]
    else:
        counts_d = torch.from_numpy(counts).cuda()
    K = None if camera is None else np.array([[camera[0], 0.0, camera[2]], [0.0, camera[1], camera[3]], [0.0, 0.0, 1.0]])
    out = ransac_rigid(torch.from_numpy(rows).cuda(), counts_d, [c[1] for c in cases], K, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _check(got, p, want, M):
    T, scale, rms, mask, result = got
    assert result[p].tolist() == [want["trial"], want["winner_count"], want["count"]], (p, result[p], want["trial"], want["winner_count"], want["count"])
    assert (mask[p, :M] == want["mask"]).all() and not mask[p, M:].any(), p
    assert _bits(T[p]) == _bits(want["T"]), (p, T[p], want["T"])
    assert _bits(scale[p]) == _bits(np.float64(want["scale"])) and _bits(rms[p]) == _bits(np.float64(want["rms"])), (p, scale[p], want["scale"], rms[p], want["rms"])


def test_counts_at_the_lane_and_chunk_tails_in_one_batch():
    """M = 0, 2 (no model), 3, 4, 63, 64, 65, 511, 512, 513, 1030 under one stride of 1100, the rows past M filled with NaN.  At M = 3 every trial draws the
    same three points, so the lowest trial wins."""
    sizes = (65, 0, 3, 1030, 4, 512, 2, 63, 513, 64, 511)
    cases = [(C.mixed(M), (M, M + 1)) for M in sizes]
    got = _run(cases, stride=1100)
    assert got[0].dtype == np.float64 and got[0].shape == (11, 4, 4) and got[3].dtype == np.uint8 and got[3].shape == (11, 1100) and got[4].dtype == np.int32
    for p, (rows, key) in enumerate(cases):
        want = GR.ransac(rows, pair_key=key)
        _check(got, p, want, len(rows))
        assert (want["trial"] >= 0) == (len(rows) >= 3)
        if len(rows) >= 9:
            assert want["count"] == len(rows) - len(rows) // 4
    assert got[4][2].tolist() == [0, 3, 3] and got[4][1].tolist() == [-1, 0, 0] and got[4][6].tolist() == [-1, 0, 0]
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]) and np.isnan(got[2][6])


@pytest.mark.parametrize("trials", (1, 255, 256, 257, 2000))
def test_trial_counts(trials):
    """A workgroup with 255 dead lanes, with one, a full one, a second with 255, and eight of which the last has 48: dead lanes must not vote."""
    rows = C.planted("forty")[0]
    want = C.restated_planted("forty", trials=trials)
    _check(_run([(rows, (0, 0))], trials=trials), 0, want, len(rows))
    assert want["trial"] < trials


@pytest.mark.parametrize("name", sorted(C.PLANTED))
def test_planted_cases_bit_for_bit_and_within_the_measured_bound(name):
    """Outlier shares of 0, 40 and 70 %, both layouts, with and without scale: the bits of the restatement, the planted transform within the CPU-measured bound,
    and the planted inlier set where the noise is zero."""
    rows, camera, T, inliers, with_scale = C.planted(name)
    want = C.restated_planted(name)
    got = _run([(rows, (0, 0))], camera=camera, with_scale=with_scale)
    _check(got, 0, want, len(rows))
    assert np.abs(got[0][0][:3] - T[:3]).max() <= 4 * C.PLANTED_DEVIATION[name]
    if C.PLANTED[name][2] == 0.0:
        assert (got[3][0].astype(bool) == inliers).all()


def test_row_words_column_counts_and_a_mirrored_set():
    """Rows of 6 and of 8 words give the same bits; the counts as a column view two words apart; a mirrored point set still gives a rotation (det +1)."""
    six, eight = C.mixed(100, words=6), C.mixed(100, words=8)
    want = GR.ransac(six, pair_key=(1, 2))
    a, b = _run([(six, (1, 2))], words=6), _run([(eight, (1, 2))], words=8, column=True)
    _check(a, 0, want, 100), _check(b, 0, want, 100)
    rows_c, camera = C.planted("camera")[:2]
    wide = np.concatenate([rows_c, np.full((len(rows_c), 2), 3.0, np.float32)], axis=1)
    _check(_run([(wide, (0, 0))], camera=camera, column=True, stride=len(wide) + 5), 0, C.restated_planted("camera"), len(wide))
    p, q, _, _ = C.horn_case("mirrored")
    mirrored = np.concatenate([p, q], axis=1).astype(np.float32)
    for with_scale in (False, True):
        got = _run([(mirrored, (3, 3))], with_scale=with_scale)
        _check(got, 0, GR.ransac(mirrored, pair_key=(3, 3), with_scale=with_scale), len(mirrored))
        A = got[0][0][:3, :3] / got[1][0]
        assert got[4][0, 0] >= 0 and got[4][0, 2] >= 3 and abs(np.linalg.det(A) - 1.0) < 1e-12 and np.abs(A @ A.T - np.eye(3)).max() < 1e-12


def test_no_model():
    """All points collinear, all points equal, a count above the stride, a negative count, a count below min_count: the winning trial -1 or -2 as stated, T, scale
    and rms NaN, the mask 0 -- and the neighbours in the batch untouched by it."""
    import torch
    from hive_amd.features import ransac_rigid
    rows = C.mixed(40)
    line = rows.copy()
    line[:, 0:3] = np.arange(40, dtype=np.float32)[:, None] * np.array([1.0, 2.0, 0.5], dtype=np.float32)
    same = rows.copy()
    same[:, 3:6] = 1.5
    got = _run([(line, (0, 1)), (same, (0, 2)), (rows, (0, 3))])
    for p, r in enumerate((line, same, rows)):
        _check(got, p, GR.ransac(r, pair_key=(0, p + 1)), 40)
    assert got[4][:2].tolist() == [[-1, 0, 0], [-1, 0, 0]] and got[4][2, 0] >= 0
    assert np.isnan(got[0][:2]).all() and np.isnan(got[1][:2]).all() and np.isnan(got[2][:2]).all() and not got[3][:2].any()
    stack = torch.from_numpy(np.stack([rows] * 4)).cuda()
    counts = torch.tensor([40, 41, -1, 39], dtype=torch.int32).cuda()
    T, scale, rms, mask, result = (t.cpu().numpy() for t in ransac_rigid(stack, counts, [(0, 3)] * 4, min_count=40))
    _check((T, scale, rms, mask, result), 0, GR.ransac(rows, pair_key=(0, 3), min_count=40), 40)
    assert result[1:].tolist() == [[-2, 0, 0], [-2, 0, 0], [-1, 0, 0]]
    assert np.isnan(T[1:]).all() and np.isnan(scale[1:]).all() and np.isnan(rms[1:]).all() and not mask[1:].any()


def test_same_bits_alone_first_last_reversed_and_again():
    rows = C.planted("noisy")[0]
    key = (7, 9)
    want = GR.ransac(rows, pair_key=key)
    others = [(C.mixed(M), (M, 0)) for M in (40, 100)]
    alone = _run([(rows, key)])
    first = _run([(rows, key)] + others, stride=200)
    last = _run(others + [(rows, key)], stride=200)
    again = _run(others + [(rows, key)], stride=200)
    reverse = _run(([(rows, key)] + others)[::-1], stride=200)
    for got, p in ((alone, 0), (first, 0), (last, 2), (again, 2), (reverse, 2)):
        _check(got, p, want, len(rows))
    for a, b in zip(last, again):
        assert _bits(a) == _bits(b)
    for a, b in zip(first, reverse):
        assert _bits(a) == _bits(b[::-1])


def test_seed_and_pair_key_change_the_trial_not_the_planted_mask():
    rows, _, _, inliers, _ = C.planted("seventy")
    trials = {C.restated_planted("seventy")["trial"]}
    for seed, key in ((1, (0, 0)), (0, (3, 4)), (0, (4, 3))):
        got = _run([(rows, key)], seed=seed)
        _check(got, 0, GR.ransac(rows, seed=seed, pair_key=key), len(rows))
        assert (got[3][0].astype(bool) == inliers).all()
        trials.add(int(got[4][0, 0]))
    assert len(trials) >= 3


def test_estimate_rigid_transform_numpy_and_device():
    import torch
    from hive_amd.features import estimate_rigid_transform
    rows, _, T0, inliers, _ = C.planted("forty")
    p, q = rows[:, 0:3].copy(), rows[:, 3:6].copy()
    want = C.restated_planted("forty")
    T, mask, stats = estimate_rigid_transform(p, q, return_stats=True)
    assert isinstance(T, np.ndarray) and T.dtype == np.float64 and T.shape == (4, 4) and isinstance(mask, np.ndarray) and mask.dtype == np.uint8 and mask.shape == (len(p),)
    assert _bits(T) == _bits(want["T"]) and (mask == want["mask"]).all() and stats[:3] == (want["trial"], want["winner_count"], want["count"])
    assert stats[3] == want["scale"] and stats[4] == want["rms"]
    Td, maskd = estimate_rigid_transform(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda(), pair_key=(2, 5), with_scale=True)
    want = GR.ransac(rows, pair_key=(2, 5), with_scale=True)
    assert Td.is_cuda and maskd.is_cuda and _bits(Td.cpu().numpy()) == _bits(want["T"]) and (maskd.cpu().numpy() == want["mask"]).all()
    for m in (0, 2):
        T, mask = estimate_rigid_transform(p[:m], q[:m])
        assert T is None and mask.shape == (m,) and not mask.any()
    line = np.arange(30, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    assert estimate_rigid_transform(line, line)[0] is None and estimate_rigid_transform(torch.from_numpy(line).cuda(), torch.from_numpy(line).cuda())[0] is None
    with pytest.raises(ValueError):
        estimate_rigid_transform(p, q[:5])
    with pytest.raises(ValueError):
        estimate_rigid_transform(p[:, :2], q[:, :2])


def test_argument_checks_and_empty_inputs():
    import torch
    from hive_amd.features import ransac_rigid
    rows = torch.zeros((2, 8, 6), dtype=torch.float32).cuda()
    counts = torch.zeros(2, dtype=torch.int32).cuda()
    for bad in (lambda: ransac_rigid(rows[:, :, :5].contiguous(), counts, [(0, 1)] * 2), lambda: ransac_rigid(rows, counts[:1], [(0, 1)] * 2),
                lambda: ransac_rigid(rows, counts, [(0, 1)]), lambda: ransac_rigid(rows.double(), counts, [(0, 1)] * 2),
                lambda: ransac_rigid(rows, counts, [(0, 1)] * 2, camera_matrix=np.eye(4))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="camera"):
        ransac_rigid(rows, counts, [(0, 1)] * 2, camera_matrix=np.diag([0.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError, match="threshold"):
        ransac_rigid(rows, counts, [(0, 1)] * 2, threshold=0.0)
    T, scale, rms, mask, result = ransac_rigid(torch.zeros((2, 0, 6), dtype=torch.float32).cuda(), counts, [(0, 1)] * 2)
    assert mask.shape == (2, 0) and result.cpu().numpy().tolist() == [[-1, 0, 0]] * 2 and np.isnan(T.cpu().numpy()).all() and np.isnan(rms.cpu().numpy()).all()
    T, scale, rms, mask, result = ransac_rigid(torch.zeros((0, 4, 6), dtype=torch.float32).cuda(), counts[:0], np.zeros((0, 2)))
    assert T.shape == (0, 4, 4) and scale.shape == (0,) and mask.shape == (0, 4) and result.shape == (0, 3)


# ---- the extractor ----
def _sift():
    from hive_amd.features import SIFT
    return _once("sift", lambda: SIFT(nfeatures=2048, capacity=512))


def _options():
    import feature_cases
    from hive_amd.pose_optimisation import FeatureExtractionOptions
    return FeatureExtractionOptions(ignore_dynamic_objects=True, min_features=feature_cases.MIN_FEATURES, max_features=2048)


def test_feature_extractor_rigid_on_a_pure_pixel_shift():
    """The blob frames over a constant-depth plane: the translation (dx d / fx, dy d / fy, 0) and no rotation within four times what the restated pipeline
    deviates on the CPU, the bits of the restated pipeline, and the same FeatureSet rows as the restated mask keeps."""
    from hive_amd.pose_optimisation import FeatureExtractor
    m, fit = C.restated_shift()
    ex = FeatureExtractor(C.ShiftDataset(), [C.SHIFT_PAIR], _options(), sift=_sift(), model="rigid")
    fs = ex.extract_feature_points()
    T, scale, rms, result = ex.pair_transforms
    assert T.shape == (1, 4, 4) and T.dtype == np.float64 and result.tolist() == [[fit["trial"], fit["winner_count"], fit["count"]]]
    assert _bits(T[0]) == _bits(fit["T"]) and scale[0] == 1.0 and _bits(rms[0]) == _bits(np.float64(fit["rms"]))
    assert np.abs(T[0][:3, 3] - C.shift_expected()).max() <= 4 * C.SHIFT_DEVIATION and np.abs(T[0][:3, :3] - np.eye(3)).max() <= 4 * C.SHIFT_DEVIATION
    keep = fit["mask"].astype(bool)
    assert ex.pair_stats.tolist() == [[m["ratio_survivors"], m["survivors"], fit["trial"], fit["winner_count"], fit["count"]]] and len(fs) == fit["count"] >= 10
    assert _bits(fs.frame_i.points.cpu().numpy()) == _bits(m["points_i"][keep]) and _bits(fs.frame_j.points.cpu().numpy()) == _bits(m["points_j"][keep])
    assert (fs.frame_i.depth.cpu().numpy() == C.SHIFT_DEPTH).all() and (fs.frame_i.index.cpu().numpy() == 0).all() and (fs.frame_j.index.cpu().numpy() == 1).all()


def test_feature_extractor_homography_is_what_it_was():
    """``model="homography"`` (spelled out or by default) on the same input: the restated homography pipeline's rows and statistics, and no transforms."""
    import feature_cases
    import ransac_restatement as RR
    from hive_amd.pose_optimisation import FeatureExtractor
    m, _ = C.restated_shift()
    fit = RR.ransac(m["points_i"], m["points_j"], 3.0, 2000, 0, C.SHIFT_PAIR, min_count=feature_cases.MIN_FEATURES)
    keep = fit["mask"].astype(bool)
    sets = []
    for kw in (dict(model="homography"), {}):
        ex = FeatureExtractor(C.ShiftDataset(), [C.SHIFT_PAIR], _options(), sift=_sift(), **kw)
        fs = ex.extract_feature_points()
        assert ex.pair_transforms is None and ex.pair_stats.tolist() == [[m["ratio_survivors"], m["survivors"], fit["trial"], fit["winner_count"], fit["count"]]]
        assert _bits(fs.frame_i.points.cpu().numpy()) == _bits(m["points_i"][keep]) and _bits(fs.frame_j.points.cpu().numpy()) == _bits(m["points_j"][keep])
        sets.append(fs)
    for a, b in zip(sets[0].state_dict().values(), sets[1].state_dict().values()):
        assert _bits(a.cpu().numpy()) == _bits(b.cpu().numpy())


def test_estimate_trajectory_on_the_pixel_shift_dataset():
    """``registration.estimate_trajectory`` end to end through SIFT: four frames, of which (0, 1) and (2, 3) are pixel shifts and the two halves show different
    pictures, so frames 2 and 3 are lost and copy frame 1's pose.  The poses are ``chain_pairs`` of the extractor's transforms."""
    from hive_amd.geometric import Trajectory
    from hive_amd.registration import chain_pairs, estimate_trajectory

    class WithTrajectory(C.ShiftDataset):
        def __init__(self):
            super().__init__()
            first = C.transform(C.rotation((0, 1, 0), 20.0), (0.5, -0.25, 1.0))
            self.camera_trajectory = Trajectory.from_homogenous_transforms(np.stack([first] * self.num_frames))
    data = WithTrajectory()
    out = estimate_trajectory(data, feature_extraction_options=_options(), sift=_sift())
    T, scale, rms, result = out.pair_transforms
    _, fit = C.restated_shift()
    assert len(T) == 4 and _bits(T[0]) == _bits(fit["T"]) and out.lost == [2, 3] and (out.depth_scale == 1).all()  # hierarchical pairs: (0, 1) (1, 2) (2, 3) (0, 2)
    first = data.camera_trajectory.to_homogenous_transforms()[0]
    poses, _, lost = chain_pairs(4, [(0, 1), (1, 2), (2, 3), (0, 2)], T, scale, result, min_inliers=10, first_pose=first)
    got = out.trajectory.to_homogenous_transforms()
    assert lost == [2, 3] and np.abs(got - poses).max() < 1e-12 and np.abs(got[1] - fit["T"] @ first).max() < 1e-12 and np.abs(got[3] - got[1]).max() == 0
    assert len(out.feature_set) == int(out.pair_stats[:, 4].sum()) >= fit["count"]


def test_orbit_trajectory_bit_for_bit():
    """The 19 hierarchical pairs of the synthetic orbit as one batch through ``ransac_rigid`` with the camera matrix (SIFT bypassed: the rows come from the planted
    points), then ``chain_pairs``: the restated fits and the CPU trajectory, bit for bit."""
    import torch
    from hive_amd.features import ransac_rigid
    from hive_amd.registration import chain_pairs
    o = C.orbit()
    fits, poses, lam, lost = C.restated_orbit()
    stride = max(len(r) for r in o["rows"]) + 3
    rows = np.full((len(o["rows"]), stride, 8), np.nan, dtype=np.float32)
    for p, r in enumerate(o["rows"]):
        rows[p, :len(r)] = r
    counts = torch.tensor([[0, len(r)] for r in o["rows"]], dtype=torch.int32).cuda()
    out = ransac_rigid(torch.from_numpy(rows).cuda(), counts[:, 1], o["pairs"], o["K"], trials=C.ORBIT_TRIALS, min_count=C.ORBIT_MIN_INLIERS)
    got = tuple(t.cpu().numpy() for t in out)
    for p, (fit, r) in enumerate(zip(fits, o["rows"])):
        _check(got, p, fit, len(r))
    got_poses, got_lam, got_lost = chain_pairs(12, o["pairs"], got[0], got[1], got[4], min_inliers=C.ORBIT_MIN_INLIERS, first_pose=o["poses"][0])
    assert got_lost == lost == [] and _bits(got_poses) == _bits(poses) and _bits(got_lam) == _bits(lam)
    assert C.ate_rmse(got_poses, o["poses"]) <= 4 * C.ORBIT_ATE


def test_tum_adaptor_estimates_the_poses(tmp_path):
    """``TUMAdaptor.convert(estimate_pose=True)`` with sensor depth: the folder as ``convert()`` writes it, with the trajectory of
    ``registration.estimate_trajectory`` on that folder in the place of the ground-truth file's, anchored at its first pose.  The synthetic room's frames have
    under twenty keypoints, so no pair has a model: every later frame is lost, warned about, and copies the first pose."""
    from tum_fixture import write_tum_sequence
    from hive_amd import registration
    from hive_amd.dataset_adaptors import TUMAdaptor
    tum = str(tmp_path / "tum")
    write_tum_sequence(tum, num_frames=3)
    plain = TUMAdaptor(tum, str(tmp_path / "plain")).convert()
    with pytest.warns(UserWarning, match=r"\[1, 2\]"):
        ds = TUMAdaptor(tum, str(tmp_path / "posed")).convert(estimate_pose=True)
    assert ds.num_frames == 3 and np.array_equal(ds.depth_dataset[1], plain.depth_dataset[1]) and np.array_equal(ds.rgb_dataset[2], plain.rgb_dataset[2])
    want = registration.estimate_trajectory(plain)
    assert want.lost == [1, 2] and (want.pair_stats[:, 2] == -1).all()
    got, truth = ds.camera_trajectory.to_homogenous_transforms(), plain.camera_trajectory.to_homogenous_transforms()
    assert np.abs(got - want.trajectory.to_homogenous_transforms()).max() < 1e-6  # the file holds float32
    assert np.abs(got - truth[0]).max() < 1e-6 and np.abs(truth[2] - truth[0]).max() > 0.1
