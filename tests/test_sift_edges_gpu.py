"""csrc/sift.hip away from its defaults, bit for bit against the numpy restatement (tests/sift_restatement.py) at every stage -- every Gaussian layer of every
octave, the candidate table, the keypoints, the descriptors, the counts -- on the cases of tests/sift_cases.py that tests/test_sift_cpu.py proves:

* ``PARAMETER_SETS`` on the 96 x 128 pair: nOctaveLayers 1 to 5 (the picture / layer split of the detection's grid, the layer bound, contr * L, the size
  exponent, the host's threshold, the seed layer and the L + 3 plane strides all hold a `3` at the defaults), three sets whose last blur has 33 taps (radius 16,
  the blur's LDS tile completely full), contrastThreshold 0, 0.09 and 6 / 255, edgeThreshold 2 and 50, one combined set; a mask and nfeatures at five layers;
* ``SHAPES``: 6 x 6 up to 240 x 320, both sides of every change of the octave count, planes of 2 x 5, 2 x 3, 3 x 35 and 35 x 3, pictures without a candidate;
* ``BUILT``: the descriptor radius clamp, a candidate in octave 4, a descriptor byte of 255;
* the host paths of hive_amd.features.SIFT that no test ran: a capacity met exactly and missed by one keypoint, batches in chunks, a native detector remade for
  a larger batch; MIFD of pictures with one keypoint each, and the ratio test's strict `<` on an exact tie.

Stated as unreached (sift_cases.UNREACHED): the 2^29 guard of the refinement and an angle folded from 360 to 0.  Nothing here provokes a fault: every refusal
is decided on the host, from counts the kernels wrote within the capacity, before or after launches that stay inside their buffers."""
import warnings

import numpy as np
import pytest

import sift_cases
import sift_restatement as R
from test_sift_gpu import _bits, _cand_table, _restated_cand_table

pytestmark = pytest.mark.gpu

_sifts = {}


def _sift(**kw):
    from hive_amd.features import SIFT
    key = tuple(sorted(kw.items()))
    if key not in _sifts:
        _sifts[key] = SIFT(**dict(dict(capacity=512), **kw))
    return _sifts[key]


def _run(sift, pictures, masks=None):
    """The device's stages of a batch of pictures of one size: counts, per picture (keypoints, descriptors), the candidate words, [octave][layer] -> (N, rows, cols)."""
    import torch
    from hive_amd.features import octave_sizes
    gray = torch.from_numpy(np.stack(pictures)).cuda()
    kps, desc, counts = sift.detect_device(gray, None if masks is None else torch.from_numpy(np.stack(masks)).cuda())
    counts = counts.cpu().numpy()
    sift.check_counts(counts)
    found = [(kps[i, :k].cpu().numpy(), desc[i, :k].cpu().numpy()) for i, k in enumerate(counts[:, 2])]
    cand = sift.read_candidates().cpu().numpy()
    layers = [[sift.read_layer(o, l).cpu().numpy() for l in range(sift.nOctaveLayers + 3)] for o in range(len(octave_sizes(*pictures[0].shape)))]
    return dict(counts=counts, found=found, cand=cand, layers=layers)


def _same_stages(got, i, want):
    """Picture ``i`` of a ``_run`` equals the restatement's stages ``want``: every layer, the counts, the candidate table, the keypoints, the descriptors."""
    pyr = want["pyramid"]
    assert len(got["layers"]) == len(pyr)
    for o, octave in enumerate(pyr):
        assert len(got["layers"][o]) == len(octave)
        for l, plane in enumerate(octave):
            layer = got["layers"][o][l][i]
            assert layer.shape == plane.shape and layer.dtype == np.float32
            assert _bits(layer) == _bits(plane), f"octave {o} layer {l}: {np.abs(layer - plane).max()}"
    assert got["counts"][i].tolist() == [len(want["candidates"]), want["raw"], len(want["keypoints"])]
    assert (_cand_table(got["cand"][i], len(want["candidates"])) == _restated_cand_table(want["candidates"])).all()
    kps, desc = got["found"][i]
    assert kps.dtype == np.float32 and kps.shape == want["keypoints"].shape and _bits(kps) == _bits(want["keypoints"])
    assert desc.dtype == np.uint8 and desc.shape == want["descriptors"].shape and _bits(desc) == _bits(want["descriptors"])


def _same_pictures(a, i, b, j):
    """Picture ``i`` of run ``a`` and picture ``j`` of run ``b`` have the same bits at every stage."""
    for la, lb in zip(a["layers"], b["layers"]):
        for pa, pb in zip(la, lb):
            assert _bits(pa[i]) == _bits(pb[j])
    assert a["counts"][i].tolist() == b["counts"][j].tolist()
    n = int(a["counts"][i, 0])
    assert (_cand_table(a["cand"][i], n) == _cand_table(b["cand"][j], n)).all()
    assert _bits(a["found"][i][0]) == _bits(b["found"][j][0]) and _bits(a["found"][i][1]) == _bits(b["found"][j][1])


@pytest.mark.parametrize("name", sift_cases.PARAMETER_SETS)
def test_parameter_sets_bit_for_bit(name):
    """The 96 x 128 pair as a batch of two at every parameter set.  At four and five layers also a batch of three different pictures, each equal to its own
    single run (and the third to the restatement): the grid's second dimension is picture * nOctaveLayers + layer."""
    sift = _sift(**sift_cases.PARAMETER_SETS[name])
    ref, est = sift_cases.pair(*sift_cases.PARAMETER_CASE)
    both = _run(sift, [ref, est])
    for i, which in enumerate(("ref", "est")):
        want = sift_cases.restated(*sift_cases.PARAMETER_CASE, which, params=name)
        assert len(want["candidates"]) > 0 and len(want["pyramid"][0]) == sift.nOctaveLayers + 3
        _same_stages(both, i, want)
    if name in ("L4", "L5"):
        third = sift_cases.pair(*sift_cases.THIRD_CASE)[0]
        three = _run(sift, [third, est, ref])
        _same_stages(three, 0, sift_cases.restated(*sift_cases.THIRD_CASE, "ref", params=name))
        for i, picture in enumerate((third, est, ref)):
            _same_pictures(three, i, _run(sift, [picture]), 0)


def test_mask_and_nfeatures_with_five_layers():
    """A masked and an open picture in one batch at nOctaveLayers = 5; nfeatures = 10 keeps the restatement's set."""
    ref = sift_cases.pair(*sift_cases.PARAMETER_CASE)[0]
    mask = sift_cases.mask_for(*sift_cases.PARAMETER_CASE[:2])
    masked = sift_cases.restated(*sift_cases.PARAMETER_CASE, "ref", mask=True, params="L5")
    full = sift_cases.restated(*sift_cases.PARAMETER_CASE, "ref", params="L5")
    assert 0 < len(masked["candidates"]) < len(full["candidates"])
    got = _run(_sift(**sift_cases.PARAMETER_SETS["L5"]), [ref, ref], [mask, np.ones_like(mask)])
    _same_stages(got, 0, masked)
    _same_stages(got, 1, full)
    few = sift_cases.restated(*sift_cases.PARAMETER_CASE, "ref", nfeatures=10, params="L5")
    assert 0 < len(few["keypoints"]) < len(full["keypoints"]) and len(few["candidates"]) == len(full["candidates"])
    _same_stages(_run(_sift(nfeatures=10, **sift_cases.PARAMETER_SETS["L5"]), [ref]), 0, few)


@pytest.mark.parametrize("H,W", sift_cases.SHAPES)
def test_shapes_bit_for_bit(H, W):
    """Every layer of every octave down to the 2 x 5, 2 x 3, 3 x 35 and 35 x 3 planes, candidates, keypoints, descriptors and counts; a picture without
    candidates has counts of 0 and comes back as empty arrays; 240 x 320 also as the second of two pictures."""
    ref, est = sift_cases.pair(H, W, 0)
    want = sift_cases.restated(H, W, 0)
    assert tuple(o.shape[1:] for o in want["pyramid"]) == sift_cases.SHAPE_COUNTS[(H, W)][0]
    _same_stages(_run(_sift(), [ref]), 0, want)
    kps, desc = _sift().detect_and_compute(ref)
    assert kps.shape == (len(want["keypoints"]), 6) and desc.shape == (len(want["keypoints"]), 128) and kps.dtype == np.float32 and desc.dtype == np.uint8
    if (H, W) == (240, 320):
        _same_stages(_run(_sift(), [est, ref]), 1, want)


@pytest.mark.parametrize("name", sift_cases.BUILT)
def test_built_pictures_bit_for_bit(name):
    """The pictures built for the descriptor radius clamp, a candidate in octave 4 and a descriptor byte of 255, through every stage."""
    want = sift_cases.restated_built(name)
    key = sift_cases.BUILT[name][1]
    assert key is None or want["census"][key] >= 1
    got = _run(_sift(), [sift_cases.built(name)])
    _same_stages(got, 0, want)
    if name == "byte 255":
        assert got["found"][0][1].max() == 255
    if name == "octave 4":
        assert (_cand_table(got["cand"][0], 1)[:, 4] & 255).tolist() == [4]


def test_capacity_met_exactly_and_missed_by_one():
    """A picture with more raw keypoints than candidates: a capacity of the raw count succeeds; one less, still above the candidates, raises with the count of
    keypoints; one below the candidates raises with their count.  The refusals are the host's, from the counts: the kernels count past the capacity and store
    within it.  After each refusal the same object detects another picture."""
    from hive_amd import _lib
    from hive_amd.features import SIFT
    ref = sift_cases.pair(*sift_cases.PARAMETER_CASE)[0]
    want = sift_cases.restated(*sift_cases.PARAMETER_CASE, "ref")
    small_picture, small = sift_cases.pair(22, 40, 0)[0], sift_cases.restated(22, 40, 0)
    n_cand, raw = len(want["candidates"]), want["raw"]
    assert raw - 1 >= n_cand > len(small["keypoints"]) > 0
    exact = SIFT(capacity=raw)
    _same_stages(_run(exact, [ref]), 0, want)
    exact.close()
    for capacity, message in ((raw - 1, f"{raw} keypoints"), (n_cand - 1, f"{n_cand} refined candidates")):
        sift = SIFT(capacity=capacity)
        with pytest.raises(_lib.HiveError, match=message):
            sift.detect_and_compute(ref)
        kps, desc = sift.detect_and_compute(small_picture)
        assert _bits(kps) == _bits(small["keypoints"]) and _bits(desc) == _bits(small["descriptors"])
        sift.close()


def _chunk_pictures():
    H, W = sift_cases.CHUNK_CASE
    ref, est = sift_cases.pair(H, W, 0)
    return [sift_cases.pair(H, W, 5)[0], sift_cases.pair(H, W, 6)[0], ref, sift_cases.pair(H, W, 7)[0], est]


def test_a_batch_in_chunks_equals_the_single_runs():
    """Five 61 x 83 pictures through a workspace that holds two (test_sift_cpu.py proves the chunk sizes): 2 + 2 + 1.  Every picture equals its single run, the two
    of the committed case equal the restatement, and ``read_layer`` returns the last chunk's one picture."""
    from hive_amd.features import SIFT
    H, W = sift_cases.CHUNK_CASE
    pictures = _chunk_pictures()
    sift = SIFT(capacity=512, workspace_bytes=sift_cases.CHUNK_WORKSPACE)
    assert sift._chunk(H, W, 5) == 2
    got = sift.detect_and_compute(np.stack(pictures))
    layer = sift.read_layer(2, 3).cpu().numpy()
    assert [entry[2] for entry in sift._native.values()] == [2]
    want_ref, want_est = sift_cases.restated(H, W, 0, False, "ref"), sift_cases.restated(H, W, 0, False, "est")
    assert layer.shape == (1,) + want_est["pyramid"][2][3].shape and _bits(layer[0]) == _bits(want_est["pyramid"][2][3])
    for i, picture in enumerate(pictures):
        alone = _sift().detect_and_compute(picture)
        assert len(alone[0]) > 0 and _bits(got[i][0]) == _bits(alone[0]) and _bits(got[i][1]) == _bits(alone[1])
    for i, want in ((2, want_ref), (4, want_est)):
        assert _bits(got[i][0]) == _bits(want["keypoints"]) and _bits(got[i][1]) == _bits(want["descriptors"])
    sift.close()


def test_a_larger_batch_remakes_the_native_detector():
    """A fresh object detects one picture, then three in one call: the native detector made for one picture is destroyed and remade for three, and all four results
    equal the restatement."""
    from hive_amd.features import SIFT
    H, W = sift_cases.CHUNK_CASE
    cases = ((H, W, 0, False, "ref"), (H, W, 0, False, "est"), (H, W, 2, True, "ref"), (H, W, 2, True, "est"))
    pictures = [sift_cases.pair(*case[:4])[0 if case[4] == "ref" else 1] for case in cases]
    sift = SIFT(capacity=512)
    one = sift.detect_and_compute(pictures[0])
    assert [entry[2] for entry in sift._native.values()] == [1]
    three = sift.detect_and_compute(np.stack(pictures[1:]))
    assert [entry[2] for entry in sift._native.values()] == [3]
    for (kps, desc), case in zip([one] + three, cases):
        want = sift_cases.restated(*case)
        assert len(want["keypoints"]) > 0 and _bits(kps) == _bits(want["keypoints"]) and _bits(desc) == _bits(want["descriptors"])
    sift.close()


def test_mifd_of_one_keypoint_a_side_is_nan_with_the_references_warning():
    from hive_amd.features import mifd
    picture = sift_cases.pair(6, 70, 0)[0]
    assert len(sift_cases.restated(6, 70, 0)["keypoints"]) == 1
    with pytest.warns(UserWarning, match="Not enough descriptors for k=2, only got 1 and 1"):
        want = R.mifd(picture, picture, with_matches=True)
    with pytest.warns(UserWarning, match="Not enough descriptors for k=2, only got 1 and 1"):
        got = mifd(picture, picture, sift=_sift(), return_matches=True)
    assert np.isnan(want[0]) and np.isnan(got[0]) and got[1] == want[1] == 0


def test_the_ratio_test_is_strict_on_an_exact_tie():
    """ratio_threshold = 0.5.  Query 0 has squared distances 4 and 16 to its two nearest: 2 < 0.5 * 4 is false, it is rejected.  Query 1 has 4 and 17: kept.  The
    score is the one distance of query 1 to its match; score and count equal the restatement's bit for bit."""
    import torch
    from hive_amd.features import score_pairs
    sift = _sift()
    cap = sift.capacity
    query = np.zeros((2, 128), dtype=np.uint8)
    query[1, 5] = 200
    train = np.zeros((4, 128), dtype=np.uint8)
    train[0, 0] = 2                      # 4 from query 0
    train[1, 1] = 4                      # 16 from query 0
    train[2], train[3] = query[1], query[1]
    train[2, 0] = 2                      # 4 from query 1
    train[3, 1], train[3, 2] = 4, 1      # 17 from query 1
    rng = np.random.default_rng(11)
    kq, kt = (np.concatenate([rng.uniform(1.0, 90.0, (n, 2)), np.ones((n, 4))], axis=1).astype(np.float32) for n in (2, 4))
    idx, dist = R.knn(query, train)
    assert idx.tolist() == [[0, 1], [2, 3]] and dist.tolist() == [[2.0, 4.0], [2.0, float(np.sqrt(np.float32(17)))]]
    want = R.mifd_from_features(kq, query, kt, train, ratio_threshold=0.5)
    assert want[1] == 1 and want[0] == float(np.sqrt(np.sum((kq[1, :2] - kt[2, :2]).astype(np.float64) ** 2)))
    kps, desc, counts = np.zeros((2, cap, 6), np.float32), np.zeros((2, cap, 128), np.uint8), np.zeros((2, 3), np.int32)
    kps[0, :2], kps[1, :4], desc[0, :2], desc[1, :4], counts[:, 2] = kq, kt, query, train, (2, 4)
    features = tuple(torch.from_numpy(a).cuda() for a in (kps, desc, counts))
    scores, matches, idx_d, dist_d = score_pairs(sift, features, 0, 1, 1, sift._context(features[0].device), ratio_threshold=0.5)
    assert (idx_d[0, :2].cpu().numpy() == idx).all() and _bits(dist_d[0, :2].cpu().numpy()) == _bits(dist)
    assert int(matches.cpu().numpy()[0]) == want[1] and _bits(scores.cpu().numpy()[0]) == _bits(np.float64(want[0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        both = R.mifd_from_features(kq, query, kt, train, ratio_threshold=0.51)
    assert both[1] == 2
    scores, matches, _, _ = score_pairs(sift, features, 0, 1, 1, sift._context(features[0].device), ratio_threshold=0.51)
    assert int(matches.cpu().numpy()[0]) == 2 and _bits(scores.cpu().numpy()[0]) == _bits(np.float64(both[0]))
