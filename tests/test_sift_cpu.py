"""The numpy restatement of SIFT, the exact matcher and MIFD (tests/sift_restatement.py) alone: that the committed cases of tests/sift_cases.py are not empty
(so the GPU tests cannot pass on empty lists), what the score does on known pairs, and the pieces the kernels share with it: the polynomial exp / atan2 /
sin / cos, the folded reflect-101 border, the matcher's tie rule.

The second half proves the cases of tests/test_sift_edges_gpu.py: every parameter set, shape and built picture of tests/sift_cases.py holds what is recorded
beside it, their union reaches every branch the restatement's census names (but the two stated as unreached), and a restatement with one rule deliberately wrong
-- a `3` where nOctaveLayers belongs, a 33-tap blur without its last tap, a clamped border, a floored octave count -- differs from the right one on the named
new case (and, for the `3`s, on no committed default case: the suite before these cases could not have seen them).  The host side of hive_amd.features that needs
no GPU (octave_sizes, the refusal of 37 taps, SIFT._chunk) is here too."""
import inspect
import types
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


# ---- the cases of tests/test_sift_edges_gpu.py ----
@pytest.mark.parametrize("name", sift_cases.PARAMETER_SETS)
def test_parameter_sets_are_not_empty(name):
    """Both pictures of every parameter set have the recorded candidates and keypoints, candidates in every layer 1 .. nOctaveLayers, and blurs of the recorded
    lengths (33 taps at "L1", "L2" and "L3"), by the restatement and by hive_amd.features alike."""
    from hive_amd import features
    kw = sift_cases.PARAMETER_SETS[name]
    L, sigma = kw.get("nOctaveLayers", 3), kw.get("sigma", 1.6)
    taps = sift_cases.PARAMETER_TAPS.get(name, sift_cases.DEFAULT_TAPS)
    assert tuple(len(R.gaussian_taps(s)) for s in R.blur_sigmas(L, sigma)) == taps
    assert tuple(len(features.gaussian_taps(s)) for s in features.blur_sigmas(L, sigma)) == taps
    for which, (n_cand, n_kps) in zip(("ref", "est"), sift_cases.PARAMETER_COUNTS[name]):
        s = sift_cases.restated(*sift_cases.PARAMETER_CASE, which, params=name)
        print(f"{name} {which}: {len(s['candidates'])} candidates, {s['raw']} raw keypoints, {len(s['keypoints'])} keypoints")
        assert (len(s["candidates"]), len(s["keypoints"])) == (n_cand, n_kps) and n_cand >= 7 and n_kps >= 17
        assert set(s["candidates"]["layer"].tolist()) == set(range(1, L + 1))
        assert all(octave.shape[0] == L + 3 for octave in s["pyramid"])
    for third in ("L4", "L5"):
        if name == third:
            assert len(sift_cases.restated(*sift_cases.THIRD_CASE, "ref", params=name)["keypoints"]) >= 17


@pytest.mark.parametrize("H,W", sift_cases.SHAPES)
def test_shapes_hold_what_is_recorded(H, W):
    """The octave planes, candidates, raw keypoints and keypoints of every shape; 6 x 70 and 7 x 9 have exactly one keypoint, 6 x 6 and 70 x 6 none."""
    planes, n_cand, n_raw, n_kps = sift_cases.SHAPE_COUNTS[(H, W)]
    s = sift_cases.restated(H, W, 0)
    assert tuple(o.shape[1:] for o in s["pyramid"]) == planes and len(planes) == R.octave_count(H, W)
    assert (len(s["candidates"]), s["raw"], len(s["keypoints"])) == (n_cand, n_raw, n_kps)
    if (H, W) == (240, 320):
        assert set((s["candidates"]["octave"] & 255).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sift_cases.BUILT)
def test_built_pictures_reach_their_branch(name):
    _, key, _ = sift_cases.BUILT[name]
    n_cand, n_kps, octaves, reached = sift_cases.BUILT_COUNTS[name]
    s = sift_cases.restated_built(name)
    assert (len(s["candidates"]), len(s["keypoints"])) == (n_cand, n_kps)
    assert tuple(sorted(set((s["candidates"]["octave"] & 255).tolist()))) == octaves
    if key is not None:
        assert s["census"][key] == reached >= 1
    if name == "octave 4":
        assert min(octaves) >= 4
    if name == "byte 255":
        assert s["descriptors"].max() == 255


def test_the_new_cases_reach_every_branch_but_two():
    """The census summed over every new case: each count that sift_cases.CENSUS records is >= 1 (refinements of 0 to 4 moves, a move between layers, every way out
    -- the zero pivot among them, at contrastThreshold 0 -- several orientation peaks, cut windows of both kinds, the radius clamp, the 0.2 clip, a byte of 255),
    candidates lie in octaves 0 to 4, and the two of sift_cases.UNREACHED are reached by none."""
    total, octaves = {}, set()
    for _, s in sift_cases.new_cases():
        for key, count in s["census"].items():
            total[key] = total.get(key, 0) + count
        octaves |= set((s["candidates"]["octave"] & 255).tolist())
    print(dict(sorted(total.items())), sorted(octaves))
    for key in sift_cases.CENSUS:
        assert total.get(key, 0) >= 1, key
    assert {key: total[key] for key in sift_cases.CENSUS} == sift_cases.CENSUS  # the recorded figures are the measured ones
    assert all(total.get(key, 0) == 0 for key in sift_cases.UNREACHED)
    assert octaves == {0, 1, 2, 3, 4}


# ---- a wrong rule must show ----
def _wrong(*patches):
    """tests/sift_restatement.py with pieces of its text replaced ((old, new, occurrences) each): a module of its own."""
    source = inspect.getsource(R)
    for old, new, count in patches:
        assert source.count(old) == count, old
        source = source.replace(old, new)
    module = types.ModuleType("sift_restatement_wrong")
    exec(compile(source, "sift_restatement_wrong", "exec"), module.__dict__)
    return module


# a `3` where nOctaveLayers belongs, one at a time: rule -> (the patch, the stage it is in)
THREES = {
    "contrast": (("abs(contr) * F(L) < ct", "abs(contr) * F(3) < ct", 1), "candidates"),
    "size": (("(F(layer) + xi) / F(L))", "(F(layer) + xi) / F(3))", 1), "candidates"),
    "layer bound": (("layer > L or c < BORDER", "layer > 3 or c < BORDER", 1), "candidates"),
    "seed layer": (("octaves[-1][n_octave_layers][::2, ::2]", "octaves[-1][3][::2, ::2]", 1), "pyramid"),
}
THRESHOLD_THREE = ("0.5 * float(ct) / L * 255.0", "0.5 * float(ct) / 3 * 255.0", 1)


def _stage_differs(wrong, rule_stage, picture, want, kw):
    """Whether the wrong restatement's pyramid (a rule of the pyramid) or candidates on the right pyramid (a rule of the detection) differ from ``want``'s."""
    L, sigma = kw.get("nOctaveLayers", 3), kw.get("sigma", 1.6)
    if rule_stage == "pyramid":
        got = wrong.pyramid(picture, L, sigma)
        return len(got) != len(want["pyramid"]) or any(a.tobytes() != b.tobytes() for a, b in zip(got, want["pyramid"]))
    got = wrong.candidates(want["pyramid"], None, picture.shape, L, kw.get("contrastThreshold", 0.04), kw.get("edgeThreshold", 10), sigma)
    return got.tobytes() != want["candidates"].tobytes()


@pytest.mark.parametrize("rule", THREES)
def test_a_three_for_the_layer_count_shows_at_four_and_five_layers_only(rule):
    """At "L4" and at "L5" the wrong rule changes the stage it is in: on both pictures of the pair for the contrast test, the size exponent and the seed layer; on
    at least one of the pair and the third picture for the layer bound (a move into layer 4 or 5 is rare: at "L4" the pair has none and the third picture has
    one, which is why it was chosen).  On every committed default case it changes nothing."""
    patch, stage = THREES[rule]
    wrong = _wrong(patch)
    for name in ("L4", "L5"):
        kw = sift_cases.PARAMETER_SETS[name]
        shown = []
        for case, which in ((sift_cases.PARAMETER_CASE, "ref"), (sift_cases.PARAMETER_CASE, "est"), (sift_cases.THIRD_CASE, "ref")):
            picture = sift_cases.pair(*case)[0 if which == "ref" else 1]
            shown.append(_stage_differs(wrong, stage, picture, sift_cases.restated(*case, which, params=name), kw))
        print(f"{rule} at {name}: shows on {shown}")
        assert any(shown) if rule == "layer bound" else all(shown[:2])
    for case in sift_cases.CASES:
        for k, which in enumerate(("ref", "est")):
            assert not _stage_differs(wrong, stage, sift_cases.pair(*case)[k], sift_cases.restated(*case, which), {})


def test_a_three_in_the_dog_threshold_cannot_show_in_any_stage():
    """floor(0.5 * 0.04 / L * 255) is 1 for L = 3, 4 and 5 (1.7, 1.275, 1.02): at "L4" and "L5" a `3` there computes the same number, and no test could tell.
    Where the number differs ("L1": 1 for 5, "L2": 1 for 2, "combined": 3 for 2) the wrong rule changes how many extrema start a refinement, so it is wrong,
    but no stage output: the threshold is half the bound of the contrast test that every candidate passes later, |v| / 255 against |contr|, and no picture here
    has an extremum between the two thresholds whose refined contrast passes.  (A search over thirteen pictures and twelve contrast thresholds from 0.1 to 0.7
    at five layers, where the wrong threshold is the higher one, found none either.)  The rule is therefore pinned here on the census alone."""
    wrong = _wrong(THRESHOLD_THREE)
    for L in (3, 4, 5):
        assert np.floor(0.5 * float(np.float32(0.04)) / L * 255.0) == 1.0
    for name, differs in (("L1", True), ("L2", True), ("L4", False), ("L5", False), ("combined", True)):
        kw = sift_cases.PARAMETER_SETS[name]
        for k, which in enumerate(("ref", "est")):
            want = sift_cases.restated(*sift_cases.PARAMETER_CASE, which, params=name)
            picture = sift_cases.pair(*sift_cases.PARAMETER_CASE)[k]
            census = {}
            got = wrong.candidates(want["pyramid"], None, picture.shape, kw["nOctaveLayers"], kw.get("contrastThreshold", 0.04), kw.get("edgeThreshold", 10), kw["sigma"],
                                   census=census)
            print(f"{name} {which}: {want['census']['extrema']} starting extrema, {census['extrema']} with the wrong threshold")
            assert (census["extrema"] != want["census"]["extrema"]) == differs
            assert got.tobytes() == want["candidates"].tobytes()


@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_a_blur_without_its_33rd_tap_shows(name):
    """A blur that stops after 32 taps (a halo one sample short at radius 16) changes the layers behind the 33-tap blur, and the candidates."""
    wrong = _wrong(("for k in range(1, len(taps)):", "for k in range(1, min(len(taps), 32)):", 2))
    kw = sift_cases.PARAMETER_SETS[name]
    assert sift_cases.PARAMETER_TAPS[name][-1] == 33 and max(sift_cases.PARAMETER_TAPS[name][:-1]) < 33
    picture = sift_cases.pair(*sift_cases.PARAMETER_CASE)[0]
    want = sift_cases.restated(*sift_cases.PARAMETER_CASE, "ref", params=name)
    got = wrong.detect_and_compute(picture, stages=True, **kw)
    last = kw["nOctaveLayers"] + 2
    for a, b in zip(got["pyramid"], want["pyramid"]):
        assert a[:last].tobytes() == b[:last].tobytes() and a[last].tobytes() != b[last].tobytes()
    assert got["candidates"].tobytes() != want["candidates"].tobytes()
    default = sift_cases.CASES[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(wrong.pyramid(sift_cases.pair(*default)[0]), sift_cases.restated(*default, "ref")["pyramid"]))


@pytest.mark.parametrize("H,W", [(23, 40), (46, 50)])
def test_a_clamped_border_shows_in_the_last_octave(H, W):
    wrong = _wrong(("return np.where(m < n, m, period - m)", "return np.clip(i, 0, n - 1)", 1))
    want = sift_cases.restated(H, W, 0)["pyramid"]
    got = wrong.pyramid(sift_cases.pair(H, W, 0)[0])
    assert len(got) == len(want) and min(want[-1].shape[1:]) == 2
    assert got[-1].shape == want[-1].shape and got[-1].tobytes() != want[-1].tobytes()


def test_a_floored_octave_count_shows_at_the_listed_sizes():
    """The rule is round(log2(min(2H, 2W)) - 2) + 1; its count changes between smaller sides 11 | 12, 22 | 23 and 45 | 46.  With the floor in place of the
    rounding the pyramid loses an octave at 12, 23 and 46 and keeps its length at 11, 22 and 45: over the shapes, exactly at the ones listed below."""
    wrong = _wrong(("int(np.rint(np.log(float(2 * min(H, W))) / np.log(2.0) - 2.0)) + 1", "int(np.floor(np.log(float(2 * min(H, W))) / np.log(2.0) - 2.0)) + 1", 1))
    changed = set()
    for H, W in sift_cases.SHAPES:
        want = len(sift_cases.SHAPE_COUNTS[(H, W)][0])
        got = len(wrong.pyramid(sift_cases.pair(H, W, 0)[0]))
        assert got in (want, want - 1)
        if got != want:
            changed.add((H, W))
    assert changed == {(6, 6), (6, 70), (70, 6), (7, 9), (12, 40), (23, 40), (46, 50), (240, 320)}
    assert [R.octave_count(m, 60) for m in (11, 12, 22, 23, 45, 46)] == [3, 4, 4, 5, 5, 6]


# ---- the host side of hive_amd.features that needs no GPU ----
def test_octave_sizes_follow_the_closed_form():
    """For every smaller side m from 6 to 300: round(log2(2 m) - 2) is the largest k with 2^(2 k + 3) <= (2 m)^2 (log2(2 m) - 2 is never half an integer), so the
    count is ((4 m^2).bit_length() - 4) // 2 + 1 in integers, and octave o is (2H >> o, 2W >> o).  The restatement's count is the same, and the planes of its
    pyramids at the shapes of sift_cases.SHAPES are these sizes."""
    from hive_amd import features
    for m in range(6, 301):
        count = ((4 * m * m).bit_length() - 4) // 2 + 1
        for h, w in ((m, m), (m, m + 7), (m + 50, m)):
            assert features.octave_sizes(h, w) == [(2 * h >> o, 2 * w >> o) for o in range(count)] and R.octave_count(h, w) == count
    for (H, W), (planes, _, _, _) in sift_cases.SHAPE_COUNTS.items():
        assert tuple(features.octave_sizes(H, W)) == planes


def test_37_taps_are_refused_on_the_host():
    from hive_amd import features
    assert max(len(R.gaussian_taps(s)) for s in R.blur_sigmas(2, 1.6)) == 37
    with pytest.raises(ValueError, match="37 taps"):
        features.SIFT(nOctaveLayers=2, sigma=1.6)
    for kw in sift_cases.PARAMETER_SETS.values():
        features.SIFT(**kw)


def test_chunk_sizes_of_the_small_workspace():
    """What tests/test_sift_edges_gpu.py assumes: with sift_cases.CHUNK_WORKSPACE two 61 x 83 pictures fit, so five run as 2 + 2 + 1; the default holds all."""
    from hive_amd import features
    H, W = sift_cases.CHUNK_CASE
    small = features.SIFT(capacity=512, workspace_bytes=sift_cases.CHUNK_WORKSPACE)
    per_image = 4 * (4 * H * W) * 9 + 512 * 20 * 4
    assert per_image == 770032 and 2 * per_image <= sift_cases.CHUNK_WORKSPACE < 3 * per_image
    assert [small._chunk(H, W, n) for n in (1, 2, 3, 5)] == [1, 2, 2, 2]
    assert [features.SIFT(capacity=512)._chunk(H, W, n) for n in (1, 3, 5)] == [1, 3, 5]
    assert features.SIFT(capacity=512, workspace_bytes=1)._chunk(H, W, 5) == 1
