"""Seeded pictures for the SIFT tests, shared by the CPU and the GPU tests: Gaussian blobs and boxes on a flat canvas, a window of it as the reference picture and
the window moved by (dy, dx) = (3, 4) as the estimate (so the mean distance between matched keypoints is near 5), optionally with uniform noise of +-3.

``CASES`` run at the default parameters (tests/test_sift_gpu.py).  ``PARAMETER_SETS``, ``SHAPES`` and ``BUILT`` are the cases of tests/test_sift_edges_gpu.py; the
counts recorded beside them and the census of the branches they reach are what the restatement gives, asserted in tests/test_sift_cpu.py.  The three built
pictures reach the descriptor radius clamp, a candidate in octave 4 and a descriptor byte of 255 (the straight step edge across a blob reaches 219 at most in a
48 x 48 picture: sixteen cells share the one gradient direction; in a picture six rows high the border leaves a few samples and two bytes reach 255).  No picture,
seeded or built, reaches the two branches of ``UNREACHED``."""
import numpy as np

MARGIN = 8
SHIFT = (3, 4)  # (dy, dx)
# (H, W, seed, noise): the committed cases; tests/test_sift_cpu.py proves that none of them is empty
CASES = ((48, 64, 0, False), (48, 64, 1, True), (61, 83, 0, False), (61, 83, 2, True), (96, 128, 0, False), (96, 128, 1, True))
# at least this many keypoints per picture and ratio-test survivors per pair
MINIMA = {(48, 64): (8, 5), (61, 83): (8, 5), (96, 128): (25, 15)}

# name -> cv2.SIFT.create() keywords, run on the 96 x 128 seed-0 pair.  The (nOctaveLayers, sigma) pairs: every layer count, three of them with a blur of 33 taps
# (radius 16, the LDS tile of the blur kernel completely full); 6 / 255 is the contrastThreshold at which 0.5 c / L * 255 is 1.0 in real arithmetic.
PARAMETER_SETS = {
    "L1": dict(nOctaveLayers=1, sigma=0.58), "L2": dict(nOctaveLayers=2, sigma=1.4), "L3": dict(nOctaveLayers=3, sigma=2.0),
    "L4": dict(nOctaveLayers=4, sigma=1.6), "L5": dict(nOctaveLayers=5, sigma=1.6),
    "contrast 0": dict(contrastThreshold=0.0), "contrast 0.09": dict(contrastThreshold=0.09), "contrast 6/255": dict(contrastThreshold=6 / 255),
    "edge 2": dict(edgeThreshold=2), "edge 50": dict(edgeThreshold=50),
    "combined": dict(nOctaveLayers=5, sigma=1.6, contrastThreshold=0.09, edgeThreshold=50)}
PARAMETER_CASE = (96, 128, 0, False)
# the lengths of the blurs of each set ([0] the base blur), as hive_amd.features.gaussian_taps and the restatement give them
PARAMETER_TAPS = {"L1": (3, 9, 17, 33), "L2": (9, 13, 17, 23, 33), "L3": (15, 13, 17, 21, 27, 33), "L4": (11, 9, 11, 13, 15, 17, 21),
                  "L5": (11, 9, 9, 11, 13, 15, 15, 19), "combined": (11, 9, 9, 11, 13, 15, 15, 19)}
DEFAULT_TAPS = (11, 11, 13, 17, 21, 27)
# name -> ((candidates, keypoints) of the reference picture, the same of the estimate) by the restatement
PARAMETER_COUNTS = {
    "L1": ((28, 55), (25, 47)), "L2": ((20, 36), (16, 38)), "L3": ((18, 36), (17, 43)), "L4": ((19, 35), (18, 42)), "L5": ((22, 38), (21, 43)),
    "contrast 0": ((41, 51), (44, 60)), "contrast 0.09": ((7, 17), (8, 21)), "contrast 6/255": ((22, 37), (21, 42)), "edge 2": ((13, 27), (14, 34)),
    "edge 50": ((21, 36), (18, 39)), "combined": ((9, 20), (11, 27))}
# (H, W) at the default parameters, seed 0, the reference picture: the smallest picture; three planes one of which is 3 x 35 / 35 x 3; both sides of the three
# sizes at which the octave count changes (11 | 12, 22 | 23, 45 | 46: the pyramids of 23 x 40 and 46 x 50 end in planes of 2 x 5 and 2 x 3); 240 x 320, whose
# doubled base has 15 x 20 blur tiles and whose octaves 0 .. 3 all hold keypoints
SHAPES = ((6, 6), (6, 70), (70, 6), (7, 9), (11, 40), (12, 40), (22, 40), (23, 40), (45, 50), (46, 50), (240, 320))
# (H, W) -> (octave planes, candidates, keypoints before the duplicates leave, keypoints) by the restatement
SHAPE_COUNTS = {
    (6, 6): (((12, 12), (6, 6), (3, 3)), 0, 0, 0), (6, 70): (((12, 140), (6, 70), (3, 35)), 1, 1, 1), (70, 6): (((140, 12), (70, 6), (35, 3)), 0, 0, 0),
    (7, 9): (((14, 18), (7, 9), (3, 4)), 1, 1, 1), (11, 40): (((22, 80), (11, 40), (5, 20)), 0, 0, 0), (12, 40): (((24, 80), (12, 40), (6, 20), (3, 10)), 0, 0, 0),
    (22, 40): (((44, 80), (22, 40), (11, 20), (5, 10)), 4, 4, 4), (23, 40): (((46, 80), (23, 40), (11, 20), (5, 10), (2, 5)), 4, 4, 4),
    (45, 50): (((90, 100), (45, 50), (22, 25), (11, 12), (5, 6)), 5, 11, 11), (46, 50): (((92, 100), (46, 50), (23, 25), (11, 12), (5, 6), (2, 3)), 5, 10, 10),
    (240, 320): (((480, 640), (240, 320), (120, 160), (60, 80), (30, 40), (15, 20), (7, 10), (3, 5)), 193, 358, 358)}
# Built pictures for branches that no seeded picture reaches: name -> (blob_picture's arguments, the census key it must reach or None, what it reaches).
# "octave 4" is checked on the candidates' octave byte.
BUILT = {
    "radius clamp": ((45, 50, 22.3, 24.6, 8.0, 100.0, 110.0), "desc_radius_clamp", "a broad blob found in octave 2 (22 x 25, diagonal 33): the descriptor radius is cut to 33"),
    "octave 4": ((240, 320, 119.4, 160.3, 20.0, 100.0, 110.0), None, "a broad blob found in octave 4 (30 x 40)"),
    "byte 255": ((6, 30, 2.5, 15.0, 1.0, 60.0, 0.0, (12, 190.0)), "desc_saturated", "a step edge beside a blob in a picture six rows high: the border cuts the window to a "
                 "few samples of one gradient direction, the 0.2 clip removes most of the norm and two bytes reach 255"),
}
# name -> (candidates, keypoints, the octaves of the candidates, the count of the census key) by the restatement
BUILT_COUNTS = {"radius clamp": (1, 5, (2,), 5), "octave 4": (1, 8, (4,), None), "byte 255": (1, 1, (0,), 2)}
# The census (the ``census`` argument of tests/sift_restatement.py) summed over every new case (``new_cases``: both pictures of every parameter set, the
# third picture at "L4" and "L5", the masked reference picture at "L5", every shape, every built picture).  tests/test_sift_cpu.py asserts each of these >= 1; the figures are what the restatement counts.
CENSUS = {"extrema": 22700, "moves_0": 1029, "moves_1": 353, "moves_2": 133, "moves_3": 31, "moves_4": 22, "layer_moves": 1255, "out_zero_pivot": 20121,
          "out_overrun": 346, "out_left": 665, "out_contrast": 665, "out_edge": 169, "out_mask": 4, "ori_multi_peak": 306, "ori_window_cut": 191,
          "desc_window_cut": 684, "desc_radius_clamp": 5, "desc_clipped": 10297, "desc_saturated": 2}
# Named by the census and reached by no case, seeded or built: ``out_guard`` (an offset that is not <= 2^29: the 3 x 3 system would have to be singular to
# within float32 rounding without a zero pivot) and ``ori_angle_folded`` (an interpolated orientation bin of exactly 0 needs the smoothed histogram's bins 35
# and 1 equal to the bit; the lane-order sums of a window are not symmetric even where the picture is, and the doubled base puts every axis of symmetry of a
# picture between two samples).  With it the descriptor's own fold of 360 - angle stays unreached.
UNREACHED = ("out_guard", "ori_angle_folded")


def canvas(H, W, seed):
    rng = np.random.default_rng(seed)
    ch, cw = H + 2 * MARGIN, W + 2 * MARGIN
    img = np.full((ch, cw), 110.0)
    yy, xx = np.mgrid[0:ch, 0:cw].astype(np.float64)
    for _ in range(max(12, H * W // 400)):
        cy, cx = rng.uniform(0, ch), rng.uniform(0, cw)
        sigma, amp = rng.uniform(1.2, 5.0), rng.uniform(40.0, 110.0) * rng.choice((-1.0, 1.0))
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    for _ in range(max(4, H * W // 1500)):
        bh, bw = rng.integers(4, 14), rng.integers(4, 14)
        y0, x0 = rng.integers(0, ch - bh), rng.integers(0, cw - bw)
        img[y0:y0 + bh, x0:x0 + bw] += rng.uniform(30.0, 80.0) * rng.choice((-1.0, 1.0))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), rng


def pair(H, W, seed, noise=False):
    """(ref, est): uint8 (H, W) gray pictures."""
    img, rng = canvas(H, W, seed)
    ref = img[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    est = img[MARGIN + SHIFT[0]:MARGIN + SHIFT[0] + H, MARGIN + SHIFT[1]:MARGIN + SHIFT[1] + W]
    if noise:
        est = np.clip(est.astype(np.int64) + rng.integers(-3, 4, size=est.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(ref), np.ascontiguousarray(est)


def mask_for(H, W):
    """A uint8 mask that is zero on the right third and on a band at the top."""
    m = np.ones((H, W), dtype=np.uint8)
    m[:, 2 * W // 3:] = 0
    m[:H // 6] = 0
    return m


def gray_to_bgr(gray):
    """(H, W, 3) whose cv2-style gray conversion gives back ``gray``: three equal channels."""
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=2))


def blob_picture(H, W, cy, cx, sigma, amp, base, step=None):
    """One Gaussian blob on a flat ground; ``step = (x0, height)`` adds ``height`` from column x0 on (a straight vertical edge)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = base + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    if step is not None:
        img = img + step[1] * (xx >= step[0])
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def built(name):
    """The built picture ``name`` of ``BUILT``."""
    return blob_picture(*BUILT[name][0])


_RESTATED = {}


def restated(H, W, seed, noise=False, which="ref", mask=False, nfeatures=0, params=None):
    """tests/sift_restatement.py's stages of one picture of a case (a dict: pyramid, candidates, keypoints, descriptors, raw, census), computed once a
    process.  ``params``: a name of ``PARAMETER_SETS`` (None: the defaults)."""
    key = (H, W, seed, noise, which, mask, nfeatures, params)
    if key not in _RESTATED:
        picture = pair(H, W, seed, noise)[0 if which == "ref" else 1]
        _RESTATED[key] = _stages(picture, mask_for(H, W) if mask else None, nfeatures, params)
    return _RESTATED[key]


def restated_built(name):
    """The same of the built picture ``name``, at the default parameters."""
    key = ("built", name)
    if key not in _RESTATED:
        _RESTATED[key] = _stages(built(name), None, 0, None)
    return _RESTATED[key]


# the third picture of the batches of three at "L4" and "L5": the one 96 x 128 reference picture among seeds 0 .. 3 on which a layer bound of 3 in the
# refinement shows at nOctaveLayers = 4 (a move into layer 4)
THIRD_CASE = (96, 128, 3, False)
# SIFT(capacity=512, workspace_bytes=CHUNK_WORKSPACE) holds two 61 x 83 pictures (770 032 bytes each by SIFT._chunk): five of them run as 2 + 2 + 1
CHUNK_CASE, CHUNK_WORKSPACE = (61, 83), 1_600_000


def new_cases():
    """(label, stages) of every new case: both pictures of every parameter set, the third picture at "L4" and "L5", the masked reference picture at "L5", every
    shape, every built picture."""
    for name in PARAMETER_SETS:
        for which in ("ref", "est"):
            yield f"{name} {which}", restated(*PARAMETER_CASE, which, params=name)
    for name in ("L4", "L5"):
        yield f"{name} third", restated(*THIRD_CASE, "ref", params=name)
    yield "L5 masked", restated(*PARAMETER_CASE, "ref", mask=True, params="L5")
    for H, W in SHAPES:
        yield f"{H} x {W}", restated(H, W, 0)
    for name in BUILT:
        yield name, restated_built(name)


def _stages(picture, mask, nfeatures, params):
    import sift_restatement
    census = {}
    stages = sift_restatement.detect_and_compute(picture, mask, nfeatures=nfeatures, stages=True, census=census, **(PARAMETER_SETS[params] if params else {}))
    stages["census"] = census
    return stages


def restated_score(H, W, seed, noise=False):
    """(score, survivors) of the case by the restatement, without its warnings."""
    import warnings

    import sift_restatement
    a, b = restated(H, W, seed, noise, "ref"), restated(H, W, seed, noise, "est")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return sift_restatement.mifd_from_features(a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"])
