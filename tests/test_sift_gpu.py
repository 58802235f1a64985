"""SIFT, the exact matcher and MIFD on the GPU (csrc/sift.hip behind hive_amd.features and hive_amd.evaluation) against the numpy float32 restatement of their
rules (tests/sift_restatement.py), bit for bit at every stage: the Gaussian layers of every octave, the refined candidates, the oriented keypoints, the
descriptors, the matches, the score.  The cases are those of tests/sift_cases.py, which tests/test_sift_cpu.py proves not to be empty.

This file runs the default parameters (nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10, sigma 1.6: blurs of 11 to 27 taps) at 48 x 64, 61 x 83 and
96 x 128.  tests/test_sift_edges_gpu.py compares the rest in the same way: nOctaveLayers 1 to 5 as (1, 0.58), (2, 1.4), (3, 2.0), (4, 1.6), (5, 1.6), the first three
with a last blur of 33 taps; contrastThreshold 0, 0.09 and 6 / 255; edgeThreshold 2 and 50; a combined set; a mask and nfeatures at five layers; the shapes 6 x 6,
6 x 70, 70 x 6, 7 x 9, 11 | 12 x 40, 22 | 23 x 40, 45 | 46 x 50 and 240 x 320; pictures built for the descriptor radius clamp, a candidate in octave 4 and a descriptor
byte of 255; a capacity met exactly and missed by one, chunked batches, a remade native detector, one keypoint a side, the ratio test on an exact tie.  Stated as
unreached by any case (sift_cases.UNREACHED): the refinement's 2^29 guard, and an angle folded from 360 to 0 (it needs bins 35 and 1 of the smoothed histogram
equal to the bit).  A `3` for nOctaveLayers in the DoG threshold cannot show in any stage (tests/test_sift_cpu.py says why)."""
import warnings

import numpy as np
import pytest

import sift_cases
import sift_restatement as R
from test_sift_cpu import SHIFT_BOUND

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _sift(**kw):
    from hive_amd.features import SIFT
    return _once(("sift", tuple(sorted(kw.items()))), lambda: SIFT(capacity=512, **kw))


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _gpu_pair(H, W, seed, noise):
    """The device's stages of the case's two pictures, run as one batch of two: per picture (keypoints, descriptors), the candidates, the layers."""
    def make():
        import torch
        sift = _sift()
        ref, est = sift_cases.pair(H, W, seed, noise)
        kps, desc, counts = sift.detect_device(torch.from_numpy(np.stack([ref, est])).cuda())
        counts = counts.cpu().numpy()
        sift.check_counts(counts)
        found = [(kps[i, :k].cpu().numpy(), desc[i, :k].cpu().numpy()) for i, k in enumerate(counts[:, 2])]
        cand = sift.read_candidates().cpu().numpy()
        layers = [[sift.read_layer(o, l).cpu().numpy() for l in range(6)] for o in range(R.octave_count(H, W))]
        return dict(found=found, counts=counts, cand=cand, layers=layers)
    return _once(("pair", H, W, seed, noise), make)


def _cand_table(words, count):
    """The device's candidate words of one picture as rows of eight int32, sorted."""
    rows = np.ascontiguousarray(words[:count]).view(np.int32).reshape(count, 8)
    return rows[np.lexsort(rows.T[::-1])]


def _restated_cand_table(cand):
    rows = np.zeros((len(cand), 8), dtype=np.int32)
    for k, name in enumerate(("x", "y", "size", "response")):
        rows[:, k] = cand[name].view(np.int32)
    for k, name in enumerate(("octave", "layer", "r", "c")):
        rows[:, 4 + k] = cand[name]
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("H,W,seed,noise", [sift_cases.CASES[0], sift_cases.CASES[2]])
def test_gaussian_layers_bit_for_bit(H, W, seed, noise):
    """Every layer of every octave at 48 x 64 and at the odd 61 x 83: the floor in the halving, and the border that folds several times in the last octaves."""
    g = _gpu_pair(H, W, seed, noise)
    for i, which in enumerate(("ref", "est")):
        pyr = sift_cases.restated(H, W, seed, noise, which)["pyramid"]
        assert len(pyr) == len(g["layers"])
        for o, octave in enumerate(pyr):
            for l in range(6):
                got = g["layers"][o][l][i]
                assert got.shape == octave[l].shape and got.dtype == np.float32
                assert _bits(got) == _bits(octave[l]), f"octave {o} layer {l} of {which}: {np.abs(got - octave[l]).max()}"


@pytest.mark.parametrize("H,W,seed,noise", sift_cases.CASES)
def test_candidates_keypoints_descriptors_bit_for_bit(H, W, seed, noise):
    g = _gpu_pair(H, W, seed, noise)
    for i, which in enumerate(("ref", "est")):
        want = sift_cases.restated(H, W, seed, noise, which)
        n_cand = int(g["counts"][i, 0])
        assert n_cand == len(want["candidates"]) > 0
        assert (_cand_table(g["cand"][i], n_cand) == _restated_cand_table(want["candidates"])).all()
        kps, desc = g["found"][i]
        assert kps.dtype == np.float32 and desc.dtype == np.uint8
        assert kps.shape == want["keypoints"].shape and len(kps) >= sift_cases.MINIMA[(H, W)][0]
        assert _bits(kps) == _bits(want["keypoints"]), np.abs(kps - want["keypoints"]).max(axis=0)
        assert desc.shape == want["descriptors"].shape
        assert _bits(desc) == _bits(want["descriptors"]), np.abs(desc.astype(int) - want["descriptors"].astype(int)).max()
        assert int(g["counts"][i, 2]) == len(kps) <= int(g["counts"][i, 1])


def test_same_bits_alone_in_a_batch_and_across_runs():
    """A picture alone, first and last in a batch of 5, and in a second run: the same keypoints, descriptors and layers."""
    H, W, seed, noise = sift_cases.CASES[2]
    sift = _sift()
    ref, est = sift_cases.pair(H, W, seed, noise)
    others = [sift_cases.pair(H, W, s, False)[0] for s in (5, 6, 7)]
    alone = sift.detect_and_compute(ref)
    layer_alone = sift.read_layer(2, 3).cpu().numpy()[0]
    first = sift.detect_and_compute(np.stack([ref] + others + [est]))
    layer_first = sift.read_layer(2, 3).cpu().numpy()[0]
    last = sift.detect_and_compute(np.stack([est] + others + [ref]))
    layer_last = sift.read_layer(2, 3).cpu().numpy()[4]
    again = sift.detect_and_compute(np.stack([est] + others + [ref]))
    want = sift_cases.restated(H, W, seed, noise, "ref")
    for kps, desc in (alone, first[0], last[4], again[4]):
        assert _bits(kps) == _bits(want["keypoints"]) and _bits(desc) == _bits(want["descriptors"])
    for a, b in zip(last, again):
        assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])
    assert _bits(layer_alone) == _bits(layer_first) == _bits(layer_last) == _bits(want["pyramid"][2][3])
    assert _bits(first[4][0]) == _bits(last[0][0]) and _bits(first[4][1]) == _bits(last[0][1])  # the estimate, last and first


def test_mask_drops_the_restatements_keypoints():
    import torch
    H, W, seed, noise = sift_cases.CASES[4]
    ref = sift_cases.pair(H, W, seed, noise)[0]
    mask = sift_cases.mask_for(H, W)
    want = sift_cases.restated(H, W, seed, noise, "ref", mask=True)
    full = sift_cases.restated(H, W, seed, noise, "ref")
    assert 0 < len(want["keypoints"]) < len(full["keypoints"])
    kps, desc = _sift().detect_and_compute(ref, mask)
    assert _bits(kps) == _bits(want["keypoints"]) and _bits(desc) == _bits(want["descriptors"])
    # device tensors in, a batch with one masked and one open picture
    both = _sift().detect_and_compute(torch.from_numpy(np.stack([ref, ref])).cuda(), torch.from_numpy(np.stack([mask, np.ones_like(mask)])).cuda())
    assert _bits(both[0][0]) == _bits(want["keypoints"]) and _bits(both[1][0]) == _bits(full["keypoints"])


def test_nfeatures_keeps_the_restatements_set():
    H, W, seed, noise = sift_cases.CASES[4]
    ref = sift_cases.pair(H, W, seed, noise)[0]
    want = sift_cases.restated(H, W, seed, noise, "ref", nfeatures=10)
    full = sift_cases.restated(H, W, seed, noise, "ref")
    assert 0 < len(want["keypoints"]) < len(full["keypoints"])
    kps, desc = _sift(nfeatures=10).detect_and_compute(ref)
    assert _bits(kps) == _bits(want["keypoints"]) and _bits(desc) == _bits(want["descriptors"])


def test_nfeatures_ties_are_all_kept():
    """Two copies of one picture side by side have the responses away from the seam twice (64 columns are a whole number of samples in every octave): the
    seventh and eighth largest are such a pair, so nfeatures = 7 keeps eight candidates."""
    ref = sift_cases.pair(48, 64, 1)[0]
    wide = np.ascontiguousarray(np.concatenate([ref, ref], axis=1))
    want = R.detect_and_compute(wide, nfeatures=7, stages=True)
    assert len(R.retain_best(want["candidates"], 7)) == 8
    kps, desc = _sift(nfeatures=7).detect_and_compute(wide)
    assert len(want["keypoints"]) >= 8
    assert _bits(kps) == _bits(want["keypoints"]) and _bits(desc) == _bits(want["descriptors"])


def test_knn_match_bit_for_bit():
    """Real descriptors, and a crafted set with ties where neither Q = 70 nor T = 130 is a multiple of the tile of 64; one train descriptor alone."""
    import torch
    from hive_amd.features import knn_match
    H, W, seed, noise = sift_cases.CASES[5]
    a, b = sift_cases.restated(H, W, seed, noise, "ref")["descriptors"], sift_cases.restated(H, W, seed, noise, "est")["descriptors"]
    rng = np.random.default_rng(3)
    train = rng.integers(0, 256, (130, 128)).astype(np.uint8)
    train[100] = train[7]
    train[129] = train[64]
    train[65] = train[63]
    query = np.concatenate([train[[7, 64, 63, 129]], rng.integers(0, 256, (66, 128)).astype(np.uint8)])
    extreme = np.stack([np.zeros(128, np.uint8), np.full(128, 255, np.uint8)])
    for q, t in ((a, b), (b, a), (query, train), (train, query), (query, train[:1]), (extreme, extreme[::-1].copy()), (query[:1], train[:64])):
        idx, dist = knn_match(q, t)
        want_idx, want_dist = R.knn(q, t)
        assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == (len(q), 2)
        assert (idx == want_idx).all() and _bits(dist) == _bits(want_dist)
    idx, dist = knn_match(query, train)
    assert idx[:4].tolist() == [[7, 100], [64, 129], [63, 65], [64, 129]] and (dist[:4] == 0).all()
    idx_d, dist_d = knn_match(torch.from_numpy(query).cuda(), torch.from_numpy(train).cuda())
    assert idx_d.is_cuda and (idx_d.cpu().numpy() == idx).all() and _bits(dist_d.cpu().numpy()) == _bits(dist)
    with pytest.raises(ValueError):
        knn_match(query[:, :64], train)


def _colour_pair(H, W, seed, noise, n=1):
    """Colour pictures whose gray planes are the case's pictures; the estimate has a white block so that the masked reference differs."""
    ref, est = sift_cases.pair(H, W, seed, noise)
    est = est.copy()
    est[H // 3:H // 3 + 9, W // 2:W // 2 + 14] = 255
    return sift_cases.gray_to_bgr(ref), sift_cases.gray_to_bgr(est)


@pytest.mark.parametrize("H,W,seed,noise", [sift_cases.CASES[1], sift_cases.CASES[4]])
def test_image_similarity_gives_the_restatements_score(H, W, seed, noise):
    from hive_amd.evaluation import image_similarity
    ref, est = _colour_pair(H, W, seed, noise)
    flat = np.full_like(ref, 90)
    refs, ests = np.stack([ref, flat, est]), np.stack([est, flat, est])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = image_similarity(refs, ests, mask_background=True)
        r = image_similarity(refs, ests, mask_background=True, mifd=_sift())
        masked_ref = np.where(est[..., 0] == 255, 255, ref[..., 0]).astype(np.uint8)
        want = R.mifd(ref[..., 0], est[..., 0], with_matches=True)
        want_masked = R.mifd(masked_ref, est[..., 0], with_matches=True)
        same = R.mifd(est[..., 0], est[..., 0], with_matches=True)
    assert base.mifd is None and base.mifd_matches is None and base.mifd_masked is None
    for name in ("ssim", "psnr", "ms_ssim", "sse", "ssim_masked", "psnr_masked", "ms_ssim_masked", "sse_masked"):
        assert _bits(getattr(base, name)) == _bits(getattr(r, name)), name
    assert r.gray_ref is None and r.ssim_map is None
    assert r.mifd.dtype == np.float64 and r.mifd.shape == (3,) and r.mifd_masked.shape == (3,)
    assert np.isfinite(want[0]) and want[1] >= 5 and np.isfinite(want_masked[0])
    assert _bits(np.float64(r.mifd[0])) == _bits(np.float64(want[0])) and int(r.mifd_matches[0]) == want[1]
    assert _bits(np.float64(r.mifd_masked[0])) == _bits(np.float64(want_masked[0]))
    assert np.isnan(r.mifd[1]) and np.isnan(r.mifd_masked[1]) and r.mifd_matches[1] == 0
    assert r.mifd[2] == 0.0 == same[0] and int(r.mifd_matches[2]) == same[1]
    with pytest.warns(UserWarning, match="Could not extract any features"):
        image_similarity(flat, flat, mifd=_sift())


def test_compare_images_returns_the_score():
    from hive_amd.evaluation import compare_images
    from hive_amd.features import SIFT
    H, W, seed, noise = sift_cases.CASES[4]
    ref, est = (sift_cases.gray_to_bgr(p) for p in sift_cases.pair(H, W, seed, noise))
    sift = SIFT()
    out = compare_images(ref, est, return_mifd=True, sift=sift)
    sift.close()
    want = sift_cases.restated_score(H, W, seed, noise)[0]
    print(f"compare_images at 96 x 128: mifd {out[3]!r}, restated {want!r}")
    assert len(out) == 4 and np.isfinite(out[3]) and abs(out[3] - 5.0) <= SHIFT_BOUND
    assert _bits(np.float64(out[3])) == _bits(np.float64(want))
    plain = compare_images(ref, est, return_mifd=True)
    assert np.isnan(plain[3]) and plain[:2] == out[:2]
    assert len(compare_images(ref, est, sift=_sift())) == 3


def test_mifd_function_matches_the_restatement():
    from hive_amd.features import mifd
    H, W, seed, noise = sift_cases.CASES[3]
    ref, est = sift_cases.pair(H, W, seed, noise)
    a, b = sift_cases.restated(H, W, seed, noise, "ref"), sift_cases.restated(H, W, seed, noise, "est")
    args = (a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"])
    want = R.mifd_from_features(*args)
    assert mifd(ref, est, sift=_sift(), return_matches=True) == want
    assert mifd(ref, est) == want[0]
    assert mifd(ref, est, ratio_threshold=0.5, sift=_sift(), return_matches=True) == R.mifd_from_features(*args, ratio_threshold=0.5)
    assert mifd(ref, est, log_residual=True, sift=_sift()) == R.mifd_from_features(*args, log_residual=True)[0]
    other = sift_cases.pair(48, 64, 0)[0]  # two sizes in one call
    o = sift_cases.restated(48, 64, 0, False, "ref")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_other = R.mifd_from_features(a["keypoints"], a["descriptors"], o["keypoints"], o["descriptors"])
        got_other = mifd(ref, other, sift=_sift(), return_matches=True)
    assert _bits(np.float64(got_other[0])) == _bits(np.float64(want_other[0])) and got_other[1] == want_other[1]
    with pytest.warns(UserWarning, match="Not enough matches"):
        assert np.isnan(mifd(ref, est, min_matches=want[1] + 1, sift=_sift()))
    flat = np.full((48, 64), 110, dtype=np.uint8)
    with pytest.warns(UserWarning, match="Could not extract any features"):
        assert np.isnan(mifd(flat, ref, sift=_sift()))
    with pytest.raises(ValueError, match="k = 2"):
        mifd(ref, est, k=3)


def test_a_capacity_too_small_raises_with_the_count():
    from hive_amd import _lib
    from hive_amd.features import SIFT
    H, W, seed, noise = sift_cases.CASES[0]
    ref = sift_cases.pair(H, W, seed, noise)[0]
    count = len(sift_cases.restated(H, W, seed, noise, "ref")["candidates"])
    assert count > 4
    small = SIFT(capacity=4)
    with pytest.raises(_lib.HiveError, match=f"{count} refined candidates"):
        small.detect_and_compute(ref)
    small.close()
    with pytest.raises(ValueError):
        SIFT(capacity=0)


def test_compare_renders_rows_carry_the_scores_only_with_a_sift():
    """The rows' MIFD are ``image_similarity``'s scores of the frames against the renders, plain and masked; without a SIFT object the rows are what they were."""
    import render_cases as C
    from hive_amd.evaluation import compare_renders, image_similarity
    H, W = 48, 64
    pose = C.general_pose()
    K, quad = C.quad_scene(H, W, pose=pose)
    _, fan = C.fan_scene(H, W)
    fan = dict(fan, vertices=C.to_world(fan["vertices"], pose))
    frames = np.stack([sift_cases.gray_to_bgr(sift_cases.pair(H, W, k)[0]) for k in range(2)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        renders, rows = compare_renders(K, [pose, pose], frames, [(fan,), (fan, quad)], size=(H, W), mifd=_sift())
        direct = image_similarity(frames, renders, mask_background=True, mifd=_sift())
        _, bare = compare_renders(K, [pose, pose], frames, [(fan,), (fan, quad)], size=(H, W))
    for k in range(2):
        assert _bits(np.float64(rows[k]["mifd"])) == _bits(direct.mifd[k]) and _bits(np.float64(rows[k]["mifd_masked"])) == _bits(direct.mifd_masked[k])
        assert "mifd" not in bare[k] and "mifd_masked" not in bare[k]
        assert {key: _bits(np.float64(v)) if isinstance(v, float) else v for key, v in bare[k].items()} == {
            key: _bits(np.float64(v)) if isinstance(v, float) else v for key, v in rows[k].items() if not key.startswith("mifd")}


def test_entry_points_refuse_bad_arguments_with_a_message(gpu_ctx):
    """NULL pointers, a picture below 6 x 6, too many taps, N outside 1 .. max_images, a layer outside the pyramid and Q = 0 return HIVE_ERR_INVALID with a
    message; nothing is launched."""
    import ctypes

    import torch
    from hive_amd import _lib
    from hive_amd._lib import ptr
    lib = gpu_ctx.lib
    sift = _sift()
    handle = sift._handle(gpu_ctx, 48, 64, 2)
    count = len(sift.taps)
    taps = (ctypes.c_void_p * count)(*(t.ctypes.data for t in sift.taps))
    good = (ctypes.c_int * count)(*(len(t) for t in sift.taps))
    long_ = (ctypes.c_int * count)(*([35] * count))
    out = ctypes.c_void_p()
    create = lambda h, w, n, layers, tap_counts, cap: lib.hive_sift_create(gpu_ctx.handle, h, w, n, 0, layers, 0.04, 10.0, 1.6, taps, tap_counts, cap, ctypes.byref(out))
    gray = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((2, 512, 6), dtype=torch.float32, device="cuda")
    desc = torch.zeros((2, 512, 128), dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 3), 7, dtype=torch.int32, device="cuda")
    idx = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    dist = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
    for what, call in (("6 x 6", lambda: create(5, 64, 1, 3, good, 16)), ("taps", lambda: create(48, 64, 1, 3, long_, 16)), ("max_images", lambda: create(48, 64, 0, 3, good, 16)),
                       ("capacity", lambda: create(48, 64, 1, 3, good, 0)), ("nOctaveLayers", lambda: create(48, 64, 1, 6, good, 16)),
                       ("NULL", lambda: lib.hive_sift_detect(handle, None, None, 1, ptr(kps), ptr(desc), ptr(counts))),
                       ("N = 9999", lambda: lib.hive_sift_detect(handle, ptr(gray), None, 9999, ptr(kps), ptr(desc), ptr(counts))),
                       ("layer 6", lambda: lib.hive_sift_read_layer(handle, 0, 6, 1, ptr(kps))), ("octave 9", lambda: lib.hive_sift_read_layer(handle, 9, 0, 1, ptr(kps))),
                       ("stage", lambda: lib.hive_sift_set_last_stage(handle, 3)),
                       ("Q = 0", lambda: lib.hive_knn_match(gpu_ctx.handle, ptr(desc), 0, ptr(desc), 4, ptr(idx), ptr(dist))),
                       ("NULL", lambda: lib.hive_mifd(gpu_ctx.handle, ptr(kps), ptr(desc), None, 512, 0, 1, 1, 0.7, 1, ptr(idx), ptr(dist), ptr(dist), ptr(idx))),
                       ("pairs", lambda: lib.hive_mifd(gpu_ctx.handle, ptr(kps), ptr(desc), ptr(counts), 512, 0, 1, 0, 0.7, 1, ptr(idx), ptr(dist), ptr(dist), ptr(idx)))):
        assert call() == _lib.ERR_INVALID, what
        assert what.split()[0] in lib.hive_last_error(gpu_ctx.handle).decode(), (what, lib.hive_last_error(gpu_ctx.handle))
    assert (counts.cpu().numpy() == 7).all() and out.value is None
