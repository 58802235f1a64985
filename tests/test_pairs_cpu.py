"""Feature pairs for pose optimisation without a GPU: the numpy restatement of the filter and the homography RANSAC (tests/ransac_restatement.py) on the cases
of tests/feature_cases.py -- the conditions that keep tests/test_pairs_gpu.py from passing on empty data -- and the host side of hive_amd.pose_optimisation:
the frame-pair lists, FeatureData / FeatureSet, the options."""
import logging

import numpy as np
import pytest

import feature_cases as C
import ransac_restatement as RR


@pytest.mark.parametrize("name", sorted(C.PLANTED))
def test_restatement_finds_the_planted_inliers_exactly(name):
    pi, pj, planted = C.planted(name)
    r = C.restated_planted(name)
    assert 0 <= r["trial"] < 2000 and r["winner_count"] <= r["count"] == int(planted.sum())
    assert (r["mask"].astype(bool) == planted).all()
    noise = C.PLANTED[name][2]
    err = np.abs(C.project(r["H"], pi[planted]) - pj[planted].astype(np.float64)).max()
    assert r["H"][2, 2] == 1.0 and err <= 2 * noise + 1e-3, err  # float32 targets: 640 * 2^-24 = 4e-5 of rounding


def test_no_model_cases_and_the_draw():
    k = np.arange(30, dtype=np.float32)
    line = np.stack([10 + 3 * k, 20 + 2 * k], axis=1)
    same = np.full((30, 2), 7.5, dtype=np.float32)
    pi, pj, _ = C.planted("small")
    for a, b in ((line, line + 5), (line, pj[:30]), (same, same), (pi[:30], same), (pi[:3], pj[:3]), (pi[:0], pj[:0])):
        r = RR.ransac(a, b)
        assert r["trial"] == -1 and r["count"] == 0 and not r["mask"].any() and np.isnan(r["H"]).all() and r["mask"].shape == (len(a),)
    assert RR.ransac(pi[:9], pj[:9], min_count=10)["trial"] == -1
    base = RR.base_key(0, (0, 1))
    for M in (4, 5, 64, 1000):
        s = RR.draw(base, np.arange(500), M)
        assert s.min() >= 0 and s.max() < M and all(len(set(row)) == 4 for row in s.tolist())
    assert not np.array_equal(RR.draw(base, np.arange(50), 100), RR.draw(RR.base_key(0, (1, 0)), np.arange(50), 100))  # the key is ordered
    # the mix and the draw are pinned by the planted cases' winning trials
    assert [C.restated_planted(n)["trial"] for n in sorted(C.PLANTED)] == [4, 108, 0]


def test_duplicates_and_the_tie_between_two_models():
    pi, pj, planted = C.planted("small")
    r = RR.ransac(np.repeat(pi, 2, axis=0), np.repeat(pj, 2, axis=0))
    assert (r["mask"].astype(bool) == np.repeat(planted, 2)).all()
    pi, pj, which = C.two_models()
    r = RR.ransac(pi, pj)
    assert r["count"] == 25 and len(set(which[r["mask"].astype(bool)])) == 1  # one of the two, whole


@pytest.mark.parametrize("seed_index", (0, 1))
@pytest.mark.parametrize("masked", (False, True))
def test_two_motion_cases_reach_their_minima(seed_index, masked):
    """Enough survivors on both motions, and a RANSAC that keeps the background and drops the object."""
    i, j, seed = 2 * seed_index, 2 * seed_index + 1, C.SEEDS[seed_index]
    m = C.restated_match(i, j, masked, holes=False)
    bg, obj = C.on_motion(m["points_i"], m["points_j"], C.BACKGROUND_MOTION), C.on_motion(m["points_i"], m["points_j"], C.OBJECT_MOTION)
    want = C.MINIMA[(seed, masked)]
    assert m["survivors"] >= want[0] and bg.sum() >= want[1] and m["ratio_survivors"] == m["survivors"]
    assert (obj.sum() == 0) if masked else (obj.sum() >= want[2])
    assert (m["points_i"][:, 0] >= 0).all() and (np.diff(m["query"]) > 0).all()  # query order
    r = C.restated_ransac(i, j, masked, holes=False)
    keep = r["mask"].astype(bool)
    assert r["count"] >= C.MIN_INLIERS and bg[keep].all() and not obj[keep].any()


def test_depth_hole_removes_survivors_and_pairs_fall_below_the_minimum():
    for masked in (False, True):
        full, holed = C.restated_match(0, 1, masked, holes=False), C.restated_match(0, 1, masked, holes=True)
        assert full["survivors"] - holed["survivors"] >= 2 and holed["ratio_survivors"] == full["ratio_survivors"]
        assert set(holed["query"]) < set(full["query"]) and holed["survivors"] >= C.MIN_FEATURES
        assert C.restated_ransac(0, 1, masked)["count"] >= C.MIN_FEATURES
    assert (C.depth_stack()[0] == 0).sum() > 0 and (C.depth_stack()[1:] > 0).all()
    assert C.restated_match(1, 2, False)["survivors"] < C.MIN_FEATURES  # pictures of two seeds: the pair the extractor must drop
    few = C.restated_match(0, 1, False, min_features=50)  # frame 0 has 49 keypoints
    assert few["indices"] is None and few["survivors"] == 0
    d = C.restated_match(0, 1, False)["distances"].astype(np.float64)
    assert not (d[:, 0] == 0.7 * d[:, 1]).any()  # no exact ratio tie in these cases: that branch is not covered


def test_sample_frame_pairs_every_mode():
    from hive_amd.pose_optimisation import FrameSamplingMode as M, sample_frame_pairs as s
    assert [m.name for m in M] == ["Exhaustive", "Consecutive", "ConsecutiveNoOverlap", "ConsecutiveNoOverlapOffset", "Hierarchical"]
    for mode in M:
        assert s(mode, 0) == [] and s(mode, 1) == []
    assert s(M.Exhaustive, 2) == s(M.Consecutive, 2) == s(M.ConsecutiveNoOverlap, 2) == s(M.Hierarchical, 2) == [(0, 1)]
    assert s(M.ConsecutiveNoOverlapOffset, 2) == []
    assert s(M.Exhaustive, 5) == [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4)]
    assert s(M.Consecutive, 5) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert s(M.ConsecutiveNoOverlap, 5) == [(0, 1), (2, 3)]
    assert s(M.ConsecutiveNoOverlapOffset, 5) == [(1, 2), (3, 4)]
    assert s(M.Hierarchical, 5) == [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (2, 4), (0, 4)]
    assert s(M.Exhaustive, 8) == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (2, 3), (2, 4), (2, 5), (2, 6),
                                  (2, 7), (3, 4), (3, 5), (3, 6), (3, 7), (4, 5), (4, 6), (4, 7), (5, 6), (5, 7), (6, 7)]
    assert s(M.Consecutive, 8) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]
    assert s(M.ConsecutiveNoOverlap, 8) == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert s(M.ConsecutiveNoOverlapOffset, 8) == [(1, 2), (3, 4), (5, 6)]
    assert s(M.Hierarchical, 8) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (0, 2), (2, 4), (4, 6), (0, 4)]
    assert s(M.Exhaustive, 9) == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (1, 8), (2, 3), (2, 4),
                                  (2, 5), (2, 6), (2, 7), (2, 8), (3, 4), (3, 5), (3, 6), (3, 7), (3, 8), (4, 5), (4, 6), (4, 7), (4, 8), (5, 6), (5, 7), (5, 8), (6, 7),
                                  (6, 8), (7, 8)]
    assert s(M.Consecutive, 9) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    assert s(M.ConsecutiveNoOverlap, 9) == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert s(M.ConsecutiveNoOverlapOffset, 9) == [(1, 2), (3, 4), (5, 6), (7, 8)]
    assert s(M.Hierarchical, 9) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (0, 2), (2, 4), (4, 6), (6, 8), (0, 4), (4, 8), (0, 8)]
    with pytest.raises(RuntimeError, match="Unsupported"):
        s("Hierarchical", 5)


def _feature_set():
    import torch
    from hive_amd.pose_optimisation import FeatureData, FeatureSet
    index_i, index_j = torch.tensor([0, 0, 1, 1, 2, 0]), torch.tensor([1, 1, 2, 2, 3, 2])
    points = torch.arange(12, dtype=torch.float64).reshape(6, 2)
    return FeatureSet(torch.eye(3, dtype=torch.float32) * 2, FeatureData(index_i, points, torch.arange(6) + 0.5), FeatureData(index_j, points + 100, torch.arange(6) + 1.5))


def test_feature_set_round_trips(tmp_path):
    import torch
    from hive_amd.pose_optimisation import FeatureData, FeatureSet
    fs = _feature_set()
    assert len(fs) == 6 == len(fs.frame_i) == len(fs.frame_j) and fs.device.type == "cpu"
    assert fs.frame_i.index.dtype == torch.int64 and fs.frame_i.points.dtype == torch.float32 and fs.frame_i.depth.dtype == torch.float32
    assert tuple(fs.frame_i.points.shape) == (6, 2) and len(FeatureSet()) == 0 and len(FeatureData()) == 0 and tuple(FeatureData().points.shape) == (0, 2)
    path = str(tmp_path / "feature_set.pth")
    fs.save(path)
    state = torch.load(path)
    assert type(state) is dict and sorted(state) == sorted(("camera_matrix",) + FeatureSet.KEYS)
    back = FeatureSet.load(path)
    for a, b in zip(fs.state_dict().values(), back.state_dict().values()):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # a file as the reference writes it: the state_dict of a module with the same names
    import collections
    torch.save(collections.OrderedDict(fs.state_dict()), path)
    assert torch.equal(FeatureSet.load(path).frame_j.points, fs.frame_j.points)
    sub = fs.sample_at([0, 1, 2])
    assert sub.frame_i.index.tolist() == [0, 0, 1, 1, 0] and sub.frame_j.index.tolist() == [1, 1, 2, 2, 2] and torch.equal(sub.camera_matrix, fs.camera_matrix)
    assert sub.frame_i.depth.tolist() == [0.5, 1.5, 2.5, 3.5, 5.5] and len(fs.sample_at([0])) == 0
    pairs = fs.subset_from([(1, 2), (0, 2), (3, 2)])
    assert pairs.frame_i.index.tolist() == [1, 1, 0] and pairs.frame_j.points[:, 0].tolist() == [104.0, 106.0, 110.0]
    picked = fs.frame_i.sample_at(torch.tensor([5, 0]))
    assert picked.index.tolist() == [0, 0] and picked.depth.tolist() == [5.5, 0.5]
    picked.points[0, 0] = -1.0
    assert fs.frame_i.points[5, 0] == 10.0  # a copy
    with pytest.raises(ValueError):
        FeatureData(torch.zeros(2), torch.zeros((3, 2)), torch.zeros(2))


def test_options_errors_and_warnings(caplog):
    from hive_amd.pose_optimisation import FeatureExtractionOptions as O
    with caplog.at_level(logging.WARNING):
        o = O()
    assert (o.ignore_dynamic_objects, o.min_features, o.max_features) == (True, 20, 2048) and not caplog.records
    assert repr(o) == "FeatureExtractionOptions(ignore_dynamic_objects=True, min_features=20, max_features=2048)"
    for bad in (dict(min_features=4), dict(min_features=20.0), dict(max_features=20), dict(max_features=10), dict(max_features=64.0)):
        with pytest.raises(ValueError, match="must be a positive integer"):
            O(**bad)
    with caplog.at_level(logging.WARNING):
        O(min_features=10)
    assert len(caplog.records) == 1 and "at least 20" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        O(min_features=20, max_features=39)
    assert len(caplog.records) == 1 and "2 * `min_features` (40)" in caplog.text
    assert O(max_features=None).max_features is None


def test_new_symbols_are_declared():
    from hive_amd import _lib
    assert _lib.ABI_VERSION == 9
    for name, args in (("hive_pairs_match", 17), ("hive_ransac_homography", 15), ("hive_pairs_compact", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args
    import hive_amd.features as F
    for name in ("match_pairs", "ransac_homography", "find_homography", "compact_pairs"):
        assert callable(getattr(F, name))
