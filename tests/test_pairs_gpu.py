"""Feature pairs for pose optimisation on the GPU (csrc/pairs.hip behind hive_amd.features and hive_amd.pose_optimisation) against the numpy restatements
(tests/sift_restatement.py, tests/ransac_restatement.py), bit for bit: the raw 2-NN table, the filtered rows and their counts, the homography, its inlier mask,
the winning trial, the counts, and the FeatureSet of a whole extraction.  The cases are those of tests/feature_cases.py, which tests/test_pairs_cpu.py proves
not to be empty.  No case holds a ratio that is an exact tie d0 == 0.7 d1 (test_pairs_cpu.py asserts it), so that branch of the filter is not covered."""
import logging

import numpy as np
import pytest

import feature_cases as C
import ransac_restatement as RR

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _sift():
    from hive_amd.features import SIFT
    return _once("sift", lambda: SIFT(nfeatures=2048, capacity=512))


def _features(masked):
    """One SIFT batch over the four frames: the device triple, and the counts on the host."""
    def make():
        import torch
        gray, masks = C.frames()
        mask = torch.from_numpy((masks == 0).astype(np.uint8)).cuda() if masked else None
        feats = _sift().detect_device(torch.from_numpy(gray).cuda(), mask)
        counts = feats[2].cpu().numpy()
        _sift().check_counts(counts)
        for k in range(4):  # the detector is tests/test_sift_gpu.py's matter; here it only has to agree so that a difference below is the matcher's
            assert _bits(feats[0][k, :counts[k, 2]].cpu().numpy()) == _bits(C.restated_sift(k, masked)[0])
        return feats, counts
    return _once(("features", masked), make)


# ---- matcher and filter ----
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("holes", (False, True))
def test_match_pairs_bit_for_bit(masked, holes):
    """An arbitrary pair list over one batch -- both directions, a repeated pair, both seeds, and a pair of two seeds -- with and without the zeroed rectangle."""
    import torch
    from hive_amd.features import match_pairs
    feats, counts = _features(masked)
    pairs = [(0, 1), (1, 0), (0, 1), (2, 3), (3, 2), (2, 3), (1, 2)]
    depth = torch.from_numpy(C.depth_stack(holes)).cuda()
    rows, pair_counts, idx, dist = (t.cpu().numpy() for t in match_pairs(feats, pairs, depth, 0.7, C.MIN_FEATURES, return_table=True))
    assert rows.shape == (7, 512, 8) and rows.dtype == np.float32 and pair_counts.dtype == np.int32 and idx.shape == dist.shape == (7, 512, 2)
    for p, (i, j) in enumerate(pairs):
        want = C.restated_match(i, j, masked, holes)
        q = int(counts[i, 2])
        assert (idx[p, :q] == want["indices"]).all() and _bits(dist[p, :q]) == _bits(want["distances"]), (p, i, j)
        assert pair_counts[p].tolist() == [want["ratio_survivors"], want["survivors"]], (p, i, j)
        n = want["survivors"]
        got = rows[p, :n]
        assert _bits(got[:, 0:2]) == _bits(want["points_i"]) and _bits(got[:, 2:4]) == _bits(want["points_j"])
        assert _bits(got[:, 4]) == _bits(want["depth_i"]) and _bits(got[:, 5]) == _bits(want["depth_j"])
        assert (got[:, 6].view(np.int32) == want["query"]).all() and (got[:, 7].view(np.int32) == want["train"]).all()
    assert _bits(rows[0, :pair_counts[0, 1]]) == _bits(rows[2, :pair_counts[2, 1]])  # the repeated pair
    full = C.restated_match(0, 1, masked, False)["survivors"]
    assert (pair_counts[0, 1] < full) == holes and pair_counts[6, 1] < C.MIN_FEATURES <= pair_counts[0, 1]
    # without the table, and below the minimum: no rows
    rows2, counts2 = match_pairs(feats, pairs[:2], depth, 0.7, C.MIN_FEATURES)
    assert (counts2.cpu().numpy() == pair_counts[:2]).all() and _bits(rows2[1, :pair_counts[1, 1]].cpu().numpy()) == _bits(rows[1, :pair_counts[1, 1]])
    _, none = match_pairs(feats, [(0, 1)], depth, 0.7, int(counts[:2, 2].min()) + 1)
    assert none.cpu().numpy().tolist() == [[0, 0]]
    with pytest.raises(ValueError, match="pictures"):
        match_pairs(feats, [(0, 4)], depth)


# ---- RANSAC ----
def _run(cases, stride=None, junk=1.0e30, **kw):
    """``cases``: [(points_i, points_j, key)] as ONE batch under one stride; rows past a pair's count hold ``junk``.  -> numpy (H, mask, result)."""
    import torch
    from hive_amd.features import ransac_homography
    stride = stride or max(max(len(c[0]) for c in cases), 1)
    rows = np.full((len(cases), stride, 4), junk, dtype=np.float32)
    for p, (pi, pj, _) in enumerate(cases):
        rows[p, :len(pi), 0:2], rows[p, :len(pi), 2:4] = pi, pj
    counts = torch.tensor([len(c[0]) for c in cases], dtype=torch.int32).cuda()
    out = ransac_homography(torch.from_numpy(rows).cuda(), counts, [c[2] for c in cases], **kw)
    return tuple(t.cpu().numpy() for t in out)


def _check(got, p, want, M):
    H, mask, result = got
    assert result[p].tolist() == [want["trial"], want["winner_count"], want["count"]], (p, result[p], want["trial"], want["winner_count"], want["count"])
    assert (mask[p, :M] == want["mask"]).all() and not mask[p, M:].any(), p
    assert _bits(H[p]) == _bits(want["H"]), (p, H[p], want["H"])


def _mixed(M, seed=5):
    """M correspondences of the planted homography, the first quarter replaced by outliers (none below 9 points)."""
    rng = np.random.default_rng(seed + M)
    src = rng.uniform(0, (640, 480), (M, 2))
    dst = C.project(C.PLANTED_H, src) if M else src
    n_out = M // 4 if M > 8 else 0
    dst[:n_out] = rng.uniform(0, (640, 480), (n_out, 2))
    return src.astype(np.float32), dst.astype(np.float32)


@pytest.mark.parametrize("name", sorted(C.PLANTED))
def test_planted_cases_bit_for_bit(name):
    pi, pj, planted = C.planted(name)
    want = C.restated_planted(name)
    got = _run([(pi, pj, (0, 0))])
    _check(got, 0, want, len(pi))
    assert (got[1][0].astype(bool) == planted).all()


def test_counts_at_the_lane_stride_tails_in_one_batch():
    """M = 0, 3 (no model), 4, 5, 63, 64, 65, 257: pairs of different sizes, one of them empty, under one stride of 300."""
    sizes = (65, 0, 3, 4, 257, 5, 63, 64)
    cases = [_mixed(M) + ((M, M + 1),) for M in sizes]
    got = _run(cases, stride=300)
    for p, (pi, pj, key) in enumerate(cases):
        want = RR.ransac(pi, pj, pair_key=key)
        _check(got, p, want, len(pi))
        assert (want["trial"] >= 0) == (len(pi) >= 4)
    assert np.isnan(got[0][1]).all() and np.isnan(got[0][2]).all() and got[2][1].tolist() == [-1, 0, 0]


@pytest.mark.parametrize("trials", (1, 63, 65, 2000))
def test_trial_counts(trials):
    pi, pj, _ = C.planted("medium")
    _check(_run([(pi, pj, (0, 0))], trials=trials), 0, C.restated_planted("medium", trials=trials), len(pi))


def test_degenerate_duplicated_and_tied_sets():
    """All points collinear (on both sides, on one) and all points equal: no model and a zero mask.  Every correspondence twice: samples with a duplicate are
    rejected by the pivot rule.  Two disjoint models of equal size: the tie goes to the lower trial."""
    k = np.arange(30, dtype=np.float32)
    line = np.stack([10 + 3 * k, 20 + 2 * k], axis=1)
    same = np.full((30, 2), 7.5, dtype=np.float32)
    pi, pj, planted = C.planted("small")
    two_i, two_j, which = C.two_models()
    cases = [(line, line + 5, (0, 1)), (line, pj[:30], (0, 2)), (same, same, (0, 3)), (pi[:30], same, (0, 4)),
             (np.repeat(pi, 2, axis=0), np.repeat(pj, 2, axis=0), (0, 5)), (two_i, two_j, (0, 6))]
    got = _run(cases)
    for p, (a, b, key) in enumerate(cases):
        want = RR.ransac(a, b, pair_key=key)
        _check(got, p, want, len(a))
        assert (want["trial"] == -1) == (p < 4)
    assert not got[1][:4].any() and np.isnan(got[0][:4]).all()
    assert (got[1][4, :len(pi) * 2].astype(bool) == np.repeat(planted, 2)).all()
    assert got[2][5, 2] == 25 and len(set(which[got[1][5, :50].astype(bool)])) == 1


def test_same_bits_alone_first_last_and_again():
    pi, pj, _ = C.planted("noisy")
    key = (7, 9)
    want = RR.ransac(pi, pj, pair_key=key)
    others = [_mixed(M) + ((M, 0),) for M in (40, 100)]
    alone = _run([(pi, pj, key)])
    first = _run([(pi, pj, key)] + others, stride=200)
    last = _run(others + [(pi, pj, key)], stride=200)
    again = _run(others + [(pi, pj, key)], stride=200)
    for got, p in ((alone, 0), (first, 0), (last, 2), (again, 2)):
        _check(got, p, want, len(pi))
    for a, b in zip(last, again):
        assert _bits(a) == _bits(b)


def test_seed_and_pair_key_change_the_trial_not_the_planted_mask():
    pi, pj, planted = C.planted("noisy")
    base = C.restated_planted("noisy")
    variants = [dict(seed=1, pair_key=(0, 0)), dict(seed=0, pair_key=(3, 4)), dict(seed=0, pair_key=(4, 3))]
    trials = {base["trial"]}
    for kw in variants:
        want = RR.ransac(pi, pj, **kw)
        got = _run([(pi, pj, kw["pair_key"])], seed=kw["seed"])
        _check(got, 0, want, len(pi))
        assert (got[1][0].astype(bool) == planted).all()
        trials.add(int(got[2][0, 0]))
    assert len(trials) == 4  # each a different winning trial


def _synthetic_features(n_i=600, n_j=700, side=200, capacity=1024, seed=11):
    """A hive_sift_detect triple made by hand, larger than a workgroup's step of 256 queries: picture 0 has n_i keypoints, picture 1 has n_j, of which the first
    n_i - 60 are picture 0's moved by the planted homography (scaled into the picture) with descriptors a few levels off, in a shuffled order."""
    rng = np.random.default_rng(seed)
    pos_i = rng.uniform(5, side - 5, (n_i, 2))
    Hm = np.array([[0.97, 0.03, 4.0], [-0.02, 1.01, 2.5], [2.0e-5, -1.0e-5, 1.0]])
    desc_i = rng.integers(0, 256, (n_i, 128))
    pos_j = rng.uniform(5, side - 5, (n_j, 2))
    desc_j = rng.integers(0, 256, (n_j, 128))
    shared = n_i - 60
    pos_j[:shared] = C.project(Hm, pos_i[:shared])
    desc_j[:shared] = np.clip(desc_i[:shared] + rng.integers(-3, 4, (shared, 128)), 0, 255)
    order = rng.permutation(n_j)
    pos_j, desc_j = pos_j[order], desc_j[order]
    kps = np.zeros((2, capacity, 6), dtype=np.float32)
    desc = np.zeros((2, capacity, 128), dtype=np.uint8)
    kps[0, :n_i, :2], kps[1, :n_j, :2] = pos_i, pos_j
    desc[0, :n_i], desc[1, :n_j] = desc_i, desc_j
    depth = np.ones((2, side, side), dtype=np.float32)
    depth[0, 40:70, 30:90] = 0.0
    depth[1, 120:140, 100:180] = 0.0
    return kps, desc, np.array([[n_i, n_i, n_i], [n_j, n_j, n_j]], dtype=np.int32), depth


def test_more_rows_than_one_step_of_a_workgroup():
    """600 queries against 700 trains, more than 256 survivors and inliers, and 1 100 correspondences, more than the 512 points the trial kernel stages at a
    time: the loops of the filter, the trial kernel and the compaction over their chunks, against the restatement."""
    import torch
    from hive_amd.features import compact_pairs, match_pairs, ransac_homography
    kps, desc, counts, depth = _synthetic_features()
    feats = tuple(torch.from_numpy(a).cuda() for a in (kps, desc, counts))
    pairs = [(0, 1), (1, 0)]
    rows, pair_counts, idx, dist = match_pairs(feats, pairs, torch.from_numpy(depth).cuda(), 0.7, 20, return_table=True)
    H, mask, result = ransac_homography(rows, pair_counts[:, 1], pairs, min_count=20)
    out, kept, offsets = (t.cpu().numpy() for t in compact_pairs(rows, pair_counts, mask, result, 20))
    rows_h, pc, mask_h, result_h = rows.cpu().numpy(), pair_counts.cpu().numpy(), mask.cpu().numpy(), result.cpu().numpy()
    expected = []
    for p, (i, j) in enumerate(pairs):
        n_i, n_j = counts[i, 2], counts[j, 2]
        want = RR.match_filter(kps[i, :n_i], desc[i, :n_i], kps[j, :n_j], desc[j, :n_j], depth[i], depth[j], 0.7, 20)
        assert (idx[p, :n_i].cpu().numpy() == want["indices"]).all() and _bits(dist[p, :n_i].cpu().numpy()) == _bits(want["distances"])
        n = want["survivors"]
        assert pc[p].tolist() == [want["ratio_survivors"], n] and 256 < n < want["ratio_survivors"]
        got = rows_h[p, :n]
        assert _bits(got[:, 0:2]) == _bits(want["points_i"]) and _bits(got[:, 2:4]) == _bits(want["points_j"])
        assert (got[:, 6].view(np.int32) == want["query"]).all() and (got[:, 7].view(np.int32) == want["train"]).all()
        fit = RR.ransac(want["points_i"], want["points_j"], pair_key=(i, j), min_count=20)
        _check((H.cpu().numpy().reshape(2, 3, 3), mask_h, result_h), p, fit, n)
        assert fit["count"] > 256
        expected.append(got[fit["mask"].astype(bool)])
    assert kept.tolist() == [len(e) for e in expected] and offsets.tolist() == [0, len(expected[0]), len(expected[0]) + len(expected[1])]
    assert _bits(out[:offsets[2]]) == _bits(np.concatenate(expected))
    pi, pj = _mixed(1100)
    _check(_run([(pi, pj, (5, 6))]), 0, RR.ransac(pi, pj, pair_key=(5, 6)), 1100)


@pytest.mark.parametrize("q_first,t_first,n", ((0, 5, 5), (5, 0, 5), (2, 3, 3)))
def test_pair_list_and_picture_runs_share_one_matcher(q_first, t_first, n):
    """``match_pairs`` with the pair list [(q_first + p, t_first + p)] and ``score_pairs`` (hive_mifd) on the same triple give the same 2-NN table, byte for
    byte, over the rows a pair has: capacity 130 (two full tiles of 64 and a tail of 2), pictures with 0, 1, 2, 65 and 130 keypoints on either side.  The
    triple is filled by hand; rows past a picture's count hold junk that must not be read."""
    import torch
    from hive_amd.features import SIFT, match_pairs, score_pairs
    cap, held = 130, [0, 1, 2, 65, 130, 130, 65, 2, 1, 0]
    rng = np.random.default_rng(17)
    desc = torch.from_numpy(rng.integers(0, 256, (10, cap, 128), dtype=np.uint8)).cuda()
    kps = torch.from_numpy(rng.uniform(0, 7, (10, cap, 6)).astype(np.float32)).cuda()
    counts = torch.from_numpy(np.repeat(np.array(held, np.int32)[:, None], 3, axis=1)).cuda()
    feats = (kps, desc, counts)
    pairs = [(q_first + p, t_first + p) for p in range(n)]
    _, _, idx_a, dist_a = match_pairs(feats, pairs, torch.ones((10, 8, 8), dtype=torch.float32, device="cuda"), return_table=True)
    sift = _once("sift130", lambda: SIFT(capacity=cap))
    _, _, idx_b, dist_b = score_pairs(sift, feats, q_first, t_first, n, sift._context(kps.device))
    for p, (i, j) in enumerate(pairs):
        Q, T = held[i], held[j]
        ia, da = idx_a[p, :Q].cpu().numpy(), dist_a[p, :Q].cpu().numpy()
        assert _bits(ia) == _bits(idx_b[p, :Q].cpu().numpy()) and _bits(da) == _bits(dist_b[p, :Q].cpu().numpy()), (i, j)
        assert ((ia[:, 0] >= 0) == (T >= 1)).all() and ((ia[:, 1] >= 0) == (T >= 2)).all() and (ia < max(T, 1)).all()
        assert (np.isinf(da) == (ia < 0)).all() and (da[:, 0] <= da[:, 1]).all()


def test_more_pairs_than_one_step_of_the_offsets_scan():
    """300 pairs of 12 to 20 correspondences; those with fewer than min_features = 14 of them, or of inliers, are dropped: the scan over the pairs in steps of 256."""
    import torch
    from hive_amd.features import compact_pairs, ransac_homography
    cases = [_mixed(12 + p % 9, seed=p) + ((p, p + 3),) for p in range(300)]
    stride = 24
    rows = np.zeros((300, stride, 8), dtype=np.float32)
    for p, (pi, pj, _) in enumerate(cases):
        rows[p, :len(pi), 0:2], rows[p, :len(pi), 2:4] = pi, pj
        rows[p, :, 4] = p  # a mark in the depth column
    counts = np.array([[len(c[0]), len(c[0])] for c in cases], dtype=np.int32)
    rows_d, counts_d = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
    H, mask, result = ransac_homography(rows_d, counts_d[:, 1], [c[2] for c in cases], trials=64, min_count=14)
    out, kept, offsets = (t.cpu().numpy() for t in compact_pairs(rows_d, counts_d, mask, result, 14))
    got = (H.cpu().numpy(), mask.cpu().numpy(), result.cpu().numpy())
    expected = []
    for p, (pi, pj, key) in enumerate(cases):
        want = RR.ransac(pi, pj, trials=64, pair_key=key, min_count=14)
        _check(got, p, want, len(pi))
        expected.append(rows[p, :len(pi)][want["mask"].astype(bool)] if want["count"] >= 14 else rows[p, :0])
    lengths = [len(e) for e in expected]
    assert kept.tolist() == lengths and offsets.tolist() == [0] + np.cumsum(lengths).tolist()
    assert 0 < sum(n == 0 for n in lengths) < 300 and _bits(out[:offsets[-1]]) == _bits(np.concatenate(expected))


def test_find_homography_numpy_and_device():
    import torch
    from hive_amd.features import find_homography
    pi, pj, planted = C.planted("small")
    want = C.restated_planted("small")
    H, mask, stats = find_homography(pi, pj, return_stats=True)
    assert isinstance(H, np.ndarray) and H.dtype == np.float64 and H.shape == (3, 3) and mask.dtype == np.uint8 and mask.shape == (len(pi),)
    assert _bits(H) == _bits(want["H"]) and (mask == want["mask"]).all() and stats == (want["trial"], want["winner_count"], want["count"])
    Hd, maskd = find_homography(torch.from_numpy(pi).cuda(), torch.from_numpy(pj).cuda(), pair_key=(2, 5))
    want = RR.ransac(pi, pj, pair_key=(2, 5))
    assert Hd.is_cuda and maskd.is_cuda and _bits(Hd.cpu().numpy()) == _bits(want["H"]) and (maskd.cpu().numpy() == want["mask"]).all()
    for m in (0, 3):
        H, mask = find_homography(pi[:m], pj[:m])
        assert H is None and mask.shape == (m,) and not mask.any()
    with pytest.raises(ValueError):
        find_homography(pi, pj[:5])


# ---- the extractor ----
PAIRS = [(0, 1), (1, 2), (2, 3), (1, 0), (3, 2)]


def _options(ignore):
    from hive_amd.pose_optimisation import FeatureExtractionOptions
    return FeatureExtractionOptions(ignore_dynamic_objects=ignore, min_features=C.MIN_FEATURES, max_features=2048)


def _same_feature_set(fs, want):
    import torch
    assert fs.frame_i.index.dtype == torch.int64 and fs.frame_i.points.dtype == torch.float32 and fs.frame_i.depth.dtype == torch.float32
    assert len(fs) == len(want["index_i"]) > 0
    for side in ("i", "j"):
        data = getattr(fs, f"frame_{side}")
        assert (data.index.cpu().numpy() == want[f"index_{side}"]).all()
        assert _bits(data.points.cpu().numpy()) == _bits(want[f"points_{side}"]) and _bits(data.depth.cpu().numpy()) == _bits(want[f"depth_{side}"])


@pytest.mark.parametrize("ignore,holes,pairs", ((False, False, PAIRS[:4]), (True, True, PAIRS)))
def test_feature_extractor_end_to_end(ignore, holes, pairs, caplog):
    """Without the masks on the depth stack without the hole, and without the pair (3, 2): with as few background keypoints as these pictures leave there, one
    homography within 3 pixels of six background and six object matches exists, and the restatement finds it as the device does (the rows would still agree)."""
    from hive_amd.pose_optimisation import FeatureExtractor
    data = C.Dataset(holes)
    ex = FeatureExtractor(data, pairs, _options(ignore), sift=_sift())
    with caplog.at_level(logging.INFO):
        fs = ex.extract_feature_points()
    want = C.restated_feature_set(pairs, masked=ignore, holes=holes)
    _same_feature_set(fs, want)
    assert fs.device.type == "cuda" and _bits(fs.camera_matrix.cpu().numpy()) == _bits(data.camera_matrix)
    assert ex.pair_stats[:, 4].tolist() == want["kept"] and want["kept"][1] == 0 and min(want["kept"][0], want["kept"][2]) >= C.MIN_FEATURES
    assert not ((fs.frame_i.index == 1) & (fs.frame_j.index == 2)).any()  # the pair below min_features is absent
    pi, pj = fs.frame_i.points.cpu().numpy(), fs.frame_j.points.cpu().numpy()
    forward = (fs.frame_i.index < fs.frame_j.index).cpu().numpy()
    # nothing that moves with the object is left (a pair (j, i) is the motion seen backwards); the rows lie within the RANSAC's 3 pixels of the background motion
    assert not C.on_motion(pi[forward], pj[forward], C.OBJECT_MOTION).any() and not C.on_motion(pj[~forward], pi[~forward], C.OBJECT_MOTION).any()
    assert C.on_motion(pi[forward], pj[forward], C.BACKGROUND_MOTION).sum() >= 2 * C.MIN_FEATURES
    if not ignore:  # the object's matches reached the RANSAC and were removed by it
        m = C.restated_match(0, 1, False, holes)
        assert C.on_motion(m["points_i"], m["points_j"], C.OBJECT_MOTION).sum() >= 7 and ex.pair_stats[0, 1] == m["survivors"] > want["kept"][0]
    good = sum(k > 0 for k in want["kept"])
    assert f"Found {good} good frame pairs ({good}/{len(pairs)})" in caplog.text and "Frame pairs cover 100.00% of the frames." in caplog.text
    assert "Found 1 group(s) of consecutive frames." in caplog.text


def test_feature_extractor_with_its_own_sift_and_no_pairs():
    from hive_amd.pose_optimisation import FeatureExtractor
    fs = FeatureExtractor(C.Dataset(), [(2, 3)], _options(True)).extract_feature_points()
    _same_feature_set(fs, C.restated_feature_set([(2, 3)], masked=True))
    assert len(FeatureExtractor(C.Dataset(), [], _options(True)).extract_feature_points()) == 0
    with pytest.raises(ValueError, match="frames"):
        FeatureExtractor(C.Dataset(), [(0, 4)], _options(True)).extract_feature_points()


def test_debug_path_cache_is_reused_and_rebuilt(tmp_path):
    import os

    from hive_amd.pose_optimisation import FeatureExtractor, FeatureSet

    class NoSift:
        def detect_device(self, *a, **k):
            raise AssertionError("the cached feature set must be used")
    path = str(tmp_path / "debug")
    first = FeatureExtractor(C.Dataset(), PAIRS[:3], _options(True), debug_path=path, sift=_sift()).extract_feature_points()
    assert sorted(os.listdir(path)) == ["feature_set.pth", "frame_pairs.txt"]
    assert np.loadtxt(os.path.join(path, "frame_pairs.txt")).tolist() == [[0.0, 1.0], [1.0, 2.0], [2.0, 3.0]]
    cached = FeatureExtractor(C.Dataset(), PAIRS[:3], _options(True), debug_path=path, sift=NoSift()).extract_feature_points()
    on_disk = FeatureSet.load(os.path.join(path, "feature_set.pth"))
    for a, b, c in zip(first.state_dict().values(), cached.state_dict().values(), on_disk.state_dict().values()):
        assert _bits(a.cpu().numpy()) == _bits(b.cpu().numpy()) == _bits(c.numpy())
    with pytest.raises(AssertionError, match="cached"):  # another pair list: the cache is dropped before anything runs
        FeatureExtractor(C.Dataset(), PAIRS[:1], _options(True), debug_path=path, sift=NoSift()).extract_feature_points()
    assert sorted(os.listdir(path)) == ["frame_pairs.txt"]
    rebuilt = FeatureExtractor(C.Dataset(), PAIRS[:1], _options(True), debug_path=path, sift=_sift()).extract_feature_points()
    _same_feature_set(rebuilt, C.restated_feature_set(PAIRS[:1], masked=True))
    assert len(rebuilt) < len(first) and len(FeatureSet.load(os.path.join(path, "feature_set.pth"))) == len(rebuilt)


def test_entry_points_refuse_bad_arguments_with_a_message(gpu_ctx):
    """NULL pointers, P = 0, a stride of 0 and half a 2-NN table return HIVE_ERR_INVALID with a message and launch nothing; a count above the stride, which only
    the device can see, is refused per pair with the result -2 (never cut)."""
    import torch
    from hive_amd import _lib
    from hive_amd._lib import ptr
    from hive_amd.features import compact_pairs, ransac_homography
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    feats, _ = _features(False)
    kps, desc, counts = feats
    depth = torch.from_numpy(C.depth_stack()).cuda()
    pairs = torch.tensor([[0, 1]], dtype=torch.int32).cuda()
    rows = torch.full((1, 512, 8), 7.0, dtype=torch.float32).cuda()
    pc = torch.full((1, 2), 7, dtype=torch.int32).cuda()
    idx = torch.zeros((1, 512, 2), dtype=torch.int32).cuda()
    Hm = torch.zeros((1, 9), dtype=torch.float64).cuda()
    mask = torch.full((1, 512), 7, dtype=torch.uint8).cuda()
    res = torch.full((1, 3), 7, dtype=torch.int32).cuda()
    off = torch.zeros(2, dtype=torch.int64).cuda()
    match = lambda kp, P, i, d: lib.hive_pairs_match(h, kp, ptr(desc), ptr(counts), 512, 4, ptr(pairs), P, ptr(depth), C.H, C.W, 0.7, 10, ptr(rows), ptr(pc), i, d)
    ransac = lambda r, P, stride, trials: lib.hive_ransac_homography(h, r, 8, ptr(pc), 2, ptr(pairs), P, stride, 3.0, trials, 0, 0, ptr(Hm), ptr(mask), ptr(res))
    compact = lambda m, P, stride: lib.hive_pairs_compact(h, ptr(rows), ptr(pc), m, ptr(res), P, stride, 10, ptr(rows), ptr(res), ptr(off))
    for what, call in (("NULL", lambda: match(None, 1, None, None)), ("P = 0", lambda: match(ptr(kps), 0, None, None)), ("half", lambda: match(ptr(kps), 1, ptr(idx), None)),
                       ("NULL", lambda: ransac(None, 1, 512, 2000)), ("P = 0", lambda: ransac(ptr(rows), 0, 512, 2000)), ("stride = 0", lambda: ransac(ptr(rows), 1, 0, 2000)),
                       ("trials = 0", lambda: ransac(ptr(rows), 1, 512, 0)), ("NULL", lambda: compact(None, 1, 512)), ("P = 0", lambda: compact(ptr(mask), 0, 512)),
                       ("stride = 0", lambda: compact(ptr(mask), 1, 0))):
        assert call() == _lib.ERR_INVALID, what
        assert what.split()[0] in lib.hive_last_error(h).decode(), (what, lib.hive_last_error(h))
    assert (rows.cpu().numpy() == 7).all() and (pc.cpu().numpy() == 7).all() and (mask.cpu().numpy() == 7).all() and (res.cpu().numpy() == 7).all()
    # stride < count: the pair is refused on the device, its neighbours are not touched by it
    pi, pj, _ = C.planted("small")
    pts = torch.from_numpy(np.stack([np.concatenate([pi, pj], axis=1)[:40]] * 3)).cuda().contiguous()
    Hs, masks, result = ransac_homography(pts, torch.tensor([40, 41, -1], dtype=torch.int32).cuda(), [(0, 0)] * 3)
    want = RR.ransac(pi[:40], pj[:40])
    result = result.cpu().numpy()
    assert result[0].tolist() == [want["trial"], want["winner_count"], want["count"]] and result[1:].tolist() == [[-2, 0, 0], [-2, 0, 0]]
    assert not masks[1:].cpu().numpy().any() and np.isnan(Hs[1:].cpu().numpy()).all() and _bits(Hs[0].cpu().numpy()) == _bits(want["H"])
    # the compaction drops what the RANSAC refused
    _, kept, offsets = compact_pairs(torch.zeros((3, 40, 8), dtype=torch.float32).cuda(), torch.tensor([[40, 40], [41, 41], [0, 0]], dtype=torch.int32).cuda(), masks.contiguous(),
                                     torch.from_numpy(result).cuda(), 10)
    assert kept.cpu().numpy().tolist() == [want["count"], 0, 0] and offsets.cpu().numpy().tolist() == [0, want["count"], want["count"], want["count"]]
