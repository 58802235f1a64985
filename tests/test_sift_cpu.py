"""The numpy restatement of SIFT, the exact matcher and MIFD (tests/sift_restatement.py) alone: that the committed cases of tests/sift_cases.py are not empty
(so the GPU tests cannot pass on empty lists), what the score does on known pairs, and the pieces the kernels share with it: the polynomial exp / atan2 /
sin / cos, the folded reflect-101 border, the matcher's tie rule."""
import warnings

import numpy as np
import pytest

import sift_cases
import sift_restatement as R

# Twice the largest |score - 5| the restatement shows over sift_cases.CASES (0.0308, at 48 x 64, seed 1, with noise; the others: 0.0001, 0.0000, 0.0265,
# 0.0152, 0.0008): the bound of every "the shifted pair scores near 5" check, here and on the GPU.
SHIFT_BOUND = 0.062


@pytest.mark.parametrize("H,W,seed,noise", sift_cases.CASES)
def test_cases_are_not_empty(H, W, seed, noise):
    """Every committed case has at least 8 keypoints a picture and 5 ratio-test survivors (25 and 15 at 96 x 128), descriptors of the right kind, keypoints in
    the stated order without duplicates."""
    min_kp, min_matches = sift_cases.MINIMA[(H, W)]
    for which in ("ref", "est"):
        s = sift_cases.restated(H, W, seed, noise, which)
        kps, desc = s["keypoints"], s["descriptors"]
        assert len(kps) >= min_kp and kps.dtype == np.float32 and kps.shape[1] == 6
        assert desc.dtype == np.uint8 and desc.shape == (len(kps), 128)
        order = np.lexsort(kps.T[::-1])
        assert (order == np.arange(len(kps))).all() and (np.diff(kps, axis=0) != 0).any(axis=1).all()
        assert (kps[:, 0] >= 0).all() and (kps[:, 0] < W).all() and (kps[:, 1] >= 0).all() and (kps[:, 1] < H).all()
        assert ((kps[:, 3] >= 0) & (kps[:, 3] < 360)).all() and (kps[:, 4] > 0).all()
        assert len(s["pyramid"]) == R.octave_count(H, W)
    score, kept = sift_cases.restated_score(H, W, seed, noise)
    print(f"{H} x {W} seed {seed} noise {noise}: score {score!r}, survivors {kept}")
    assert kept >= min_matches


@pytest.mark.parametrize("H,W,seed,noise", sift_cases.CASES)
def test_shifted_pair_scores_near_five(H, W, seed, noise):
    """The estimate is the reference moved by (3, 4): matched keypoints lie 5 apart.  |score - 5| <= SHIFT_BOUND = 0.062, twice the largest deviation the
    restatement shows over the committed cases (0.0308)."""
    score, _ = sift_cases.restated_score(H, W, seed, noise)
    print(f"{H} x {W} seed {seed} noise {noise}: |score - 5| = {abs(score - 5.0)!r}")
    assert abs(score - 5.0) <= SHIFT_BOUND


def test_a_picture_against_itself_scores_zero():
    H, W, seed, noise = sift_cases.CASES[0]
    s = sift_cases.restated(H, W, seed, noise, "ref")
    score, kept = R.mifd_from_features(s["keypoints"], s["descriptors"], s["keypoints"], s["descriptors"])
    assert score == 0.0 and kept == len(s["keypoints"])


def test_flat_and_tiny_pictures_have_no_score():
    flat = np.full((48, 64), 110, dtype=np.uint8)
    with pytest.warns(UserWarning, match="Could not extract any features"):
        assert np.isnan(R.mifd(flat, flat))
    tiny = sift_cases.pair(12, 12, 0)[0]
    with pytest.warns(UserWarning, match="Could not extract any features|Not enough descriptors"):
        assert np.isnan(R.mifd(tiny, tiny))
    with pytest.raises(ValueError):
        R.mifd_from_features(None, None, None, None, k=3)


def test_min_matches_and_log_residual():
    H, W, seed, noise = sift_cases.CASES[0]
    a, b = sift_cases.restated(H, W, seed, noise, "ref"), sift_cases.restated(H, W, seed, noise, "est")
    args = (a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"])
    _, kept = sift_cases.restated_score(H, W, seed, noise)
    with pytest.warns(UserWarning, match="Not enough matches"):
        score, kept_again = R.mifd_from_features(*args, min_matches=kept + 1)
    assert np.isnan(score) and kept_again == kept
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        logged, _ = R.mifd_from_features(*args, log_residual=True)
    assert 0.0 < logged < 1.0  # log10 of positions a few pixels apart


def test_knn_ties_go_to_the_lower_index():
    train = np.zeros((5, 128), dtype=np.uint8)
    train[0, 0], train[1, 1], train[2, 0], train[3, 2], train[4, 3] = 3, 3, 3, 4, 200
    query = np.zeros((2, 128), dtype=np.uint8)
    query[1, 3] = 200
    idx, dist = R.knn(query, train)
    assert idx.tolist() == [[0, 1], [4, 0]] and idx.dtype == np.int32
    assert dist.dtype == np.float32 and dist.tolist() == [[3.0, 3.0], [0.0, float(np.sqrt(np.float32(200 * 200 + 9)))]]
    idx, dist = R.knn(query, train[:1])
    assert idx.tolist() == [[0, -1], [0, -1]] and np.isinf(dist[:, 1]).all()


def test_polynomial_exp_atan2_sincos_are_within_their_stated_error():
    """exp: relative error below 2^-21 on [-87, 10] (a degree-7 Taylor remainder of 0.3466^8 / 8! = 5e-9 and eight roundings of at most 2^-24 each).  atan2:
    within 0.3 degrees, the accuracy cv2 states for this form.  sin / cos: absolute error below 2^-21 (remainders below 1e-9, about seven roundings)."""
    x = np.linspace(-87.0, 10.0, 200001).astype(np.float32)
    exact = np.exp(x.astype(np.float64))
    got = R.sift_exp(x)
    assert got.dtype == np.float32
    rel = np.max(np.abs(got.astype(np.float64) - exact) / exact)
    g = np.linspace(-3.0, 3.0, 601).astype(np.float32)
    yy, xx = np.meshgrid(g, g)
    a = R.sift_atan2_deg(yy, xx).astype(np.float64)
    want = np.degrees(np.arctan2(yy.astype(np.float64), xx.astype(np.float64))) % 360.0
    d = np.abs(a - want)
    off = np.minimum(d, 360.0 - d).max()
    worst = 0.0
    for deg in np.linspace(0.0, 360.0, 2881).astype(np.float32):
        c, s = R.sift_sincos_deg(deg)
        rad = np.radians(float(deg))
        worst = max(worst, abs(float(c) - np.cos(rad)), abs(float(s) - np.sin(rad)))
    print(f"exp rel {rel!r}, atan2 degrees {off!r}, sin / cos {worst!r}")
    assert rel < 2.0 ** -21 and off <= 0.3 and worst < 2.0 ** -21
    assert R.sift_atan2_deg(np.float32(0), np.float32(0)) == 0 and R.sift_atan2_deg(np.float32(1), np.float32(0)) == 90


def test_reflect_101_folds_as_often_as_needed():
    """Radius 12 on 3 samples (a 3 x 4 octave under a 25-tap blur): the index folds six times; numpy's own reflect padding agrees, and the blur of such a plane
    equals the direct float32 sums."""
    assert (R.reflect101(np.arange(-12, 15), 3) == np.pad(np.arange(3), 12, mode="reflect")).all()
    assert (R.reflect101(np.arange(-5, 6), 1) == 0).all()
    rng = np.random.default_rng(0)
    img = rng.uniform(0, 255, (3, 4)).astype(np.float32)
    taps = R.gaussian_taps(3.0)
    assert len(taps) == 25 and taps.dtype == np.float32
    got = R.blur(img, taps)
    padded = np.pad(img, 12, mode="reflect")
    rows = np.zeros((27, 4), dtype=np.float32)
    for r in range(27):
        for c in range(4):
            acc = taps[0] * padded[r, c]
            for k in range(1, 25):
                acc = acc + taps[k] * padded[r, c + k]
            rows[r, c] = acc
    want = np.zeros((3, 4), dtype=np.float32)
    for r in range(3):
        for c in range(4):
            acc = taps[0] * rows[r, c]
            for k in range(1, 25):
                acc = acc + taps[k] * rows[r + k, c]
            want[r, c] = acc
    assert got.dtype == np.float32 and (got == want).all()


def test_base_picture_is_exact_and_octaves_halve():
    gray = sift_cases.pair(61, 83, 0)[0]
    base = R.base_image(gray)
    assert base.shape == (122, 166) and (base * 16 == np.rint(base * 16)).all()  # weights 1/16, 3/16, 9/16 of bytes
    assert base[0, 0] == gray[0, 0] and base[1, 1] == np.float32(0.5625) * gray[0, 0] + np.float32(0.1875) * (int(gray[0, 1]) + int(gray[1, 0])) + np.float32(0.0625) * gray[1, 1]
    shapes = [o.shape for o in sift_cases.restated(61, 83, 0, False, "ref")["pyramid"]]
    assert shapes == [(6, 122, 166), (6, 61, 83), (6, 30, 41), (6, 15, 20), (6, 7, 10), (6, 3, 5)]


def test_mask_and_nfeatures_keep_what_they_should():
    H, W, seed, noise = sift_cases.CASES[4]
    full = sift_cases.restated(H, W, seed, noise, "ref")
    masked = sift_cases.restated(H, W, seed, noise, "ref", mask=True)
    m = sift_cases.mask_for(H, W)
    assert 0 < len(masked["keypoints"]) < len(full["keypoints"])
    for x, y in masked["keypoints"][:, :2]:
        assert m[int(y + np.float32(0.5)), int(x + np.float32(0.5))] == 1
    few = sift_cases.restated(H, W, seed, noise, "ref", nfeatures=10)
    resp = np.sort(full["candidates"]["response"])[::-1]
    assert len(few["candidates"]) == len(full["candidates"]) and 0 < len(few["keypoints"]) < len(full["keypoints"])
    assert (few["keypoints"][:, 4] >= resp[9]).all() and len(set(few["keypoints"][:, 4])) >= min(10, len(set(resp[:10])))
