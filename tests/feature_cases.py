"""Cases for the feature-pair tests (tests/test_pairs_cpu.py, tests/test_pairs_gpu.py), built on tests/sift_cases.py.

Two-motion pairs: ``sift_cases.pair(96, 128, seed)``, whose background moves by (dy, dx) = (3, 4), with a 40 x 48 block of another canvas pasted at (row, column)
(19, 32) in the reference picture and at (31, 16) in the estimate -- a dynamic object that moves against the background; the instance masks are 1 on the block.
A depth stack that is smooth and positive except for a zeroed rectangle over two surviving keypoints.  Planted-homography point sets for the RANSAC alone.
Everything the restatements make of a case is computed once a process and shared."""
import numpy as np

import ransac_restatement as RR
import sift_cases
import sift_restatement

H, W = 96, 128
SEEDS = (1, 3)
MIN_FEATURES = 10
BLOCK = (40, 48)
AT_REF, AT_EST = (19, 32), (31, 16)  # (row, column) of the block
BACKGROUND_MOTION = (-float(sift_cases.SHIFT[1]), -float(sift_cases.SHIFT[0]))  # (dx, dy) of a keypoint from the reference picture to the estimate
OBJECT_MOTION = (float(AT_EST[1] - AT_REF[1]), float(AT_EST[0] - AT_REF[0]))
MOTION_TOLERANCE = 1.5  # pixels: the two motions are 19 pixels apart
# at least this many per seed, proved by tests/test_pairs_cpu.py: (survivors, on the background motion, on the object motion) without the masks,
# (survivors, on the background motion) with them
MINIMA = {(1, False): (24, 16, 7), (3, False): (26, 15, 8), (1, True): (18, 17, 0), (3, True): (18, 15, 0)}
MIN_INLIERS = 12

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def two_motion(seed):
    """(ref, est, ref_mask, est_mask): uint8 (96, 128) gray pictures and instance masks."""
    def make():
        ref, est = (p.copy() for p in sift_cases.pair(H, W, seed))
        block = sift_cases.canvas(H, W, seed + 100)[0][10:10 + BLOCK[0], 10:10 + BLOCK[1]]
        masks = []
        for picture, (r, c) in ((ref, AT_REF), (est, AT_EST)):
            picture[r:r + BLOCK[0], c:c + BLOCK[1]] = block
            mask = np.zeros((H, W), dtype=np.uint8)
            mask[r:r + BLOCK[0], c:c + BLOCK[1]] = 1
            masks.append(mask)
        return ref, est, masks[0], masks[1]
    return _once(("two_motion", seed), make)


def frames():
    """The four-frame sequence: seed 1's reference and estimate, then seed 3's.  (gray (4, H, W), masks (4, H, W))."""
    parts = [two_motion(seed) for seed in SEEDS]
    return np.stack([p[k] for p in parts for k in (0, 1)]), np.stack([p[k] for p in parts for k in (2, 3)])


def restated_sift(frame, masked):
    """tests/sift_restatement.py's (keypoints, descriptors) of a frame of ``frames()``; ``masked``: with the SIFT mask ``instance mask == 0``."""
    def make():
        gray, masks = frames()
        return sift_restatement.detect_and_compute(gray[frame], (masks[frame] == 0).astype(np.uint8) if masked else None)
    return _once(("sift", frame, masked), make)


def smooth_depth():
    yy, xx = np.mgrid[0:H, 0:W]
    return (1.0 + 0.01 * yy + 0.005 * xx).astype(np.float32)


def depth_stack(holes=True):
    """float32 (4, H, W): smooth positive depth; with ``holes`` frame 0 has a zeroed rectangle over the two survivors of the masked pair (0, 1) -- background keypoints, which the
    unmasked pair has too -- that lie closest together."""
    def make():
        depth = np.stack([smooth_depth() + np.float32(0.25 * k) for k in range(4)])
        if holes:
            full = restated_match(0, 1, masked=True, holes=False)
            pts = full["points_i"].astype(np.float64)
            d = np.linalg.norm(pts[:, None] - pts[None], axis=2) + 1e9 * np.eye(len(pts))
            a, b = np.unravel_index(np.argmin(d), d.shape)
            x0, x1 = int(np.floor(min(pts[a, 0], pts[b, 0]))) - 1, int(np.ceil(max(pts[a, 0], pts[b, 0]))) + 1
            y0, y1 = int(np.floor(min(pts[a, 1], pts[b, 1]))) - 1, int(np.ceil(max(pts[a, 1], pts[b, 1]))) + 1
            depth[0, max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = 0.0
        return depth
    return _once(("depth", holes), make)


def restated_match(i, j, masked, holes=True, min_features=MIN_FEATURES):
    """``ransac_restatement.match_filter`` of frames i -> j."""
    def make():
        depth = depth_stack(holes)
        (kp_i, d_i), (kp_j, d_j) = restated_sift(i, masked), restated_sift(j, masked)
        return RR.match_filter(kp_i, d_i, kp_j, d_j, depth[i], depth[j], 0.7, min_features)
    return _once(("match", i, j, masked, holes, min_features), make)


def restated_ransac(i, j, masked, holes=True, min_features=MIN_FEATURES, seed=0):
    def make():
        m = restated_match(i, j, masked, holes, min_features)
        return RR.ransac(m["points_i"], m["points_j"], 3.0, 2000, seed, (i, j), min_count=min_features)
    return _once(("ransac", i, j, masked, holes, min_features, seed), make)


def restated_feature_set(pairs, masked, holes=True, min_features=MIN_FEATURES, seed=0):
    """What ``FeatureExtractor.extract_feature_points`` must return for ``pairs`` of ``frames()``: a dict of index_i, points_i, depth_i, index_j, points_j,
    depth_j, and ``kept`` the rows of every pair."""
    cols = dict(index_i=[], points_i=[], depth_i=[], index_j=[], points_j=[], depth_j=[])
    kept = []
    for i, j in pairs:
        m, r = restated_match(i, j, masked, holes, min_features), restated_ransac(i, j, masked, holes, min_features, seed)
        keep = r["mask"].astype(bool)
        if m["survivors"] < min_features or r["count"] < min_features:
            keep = np.zeros(len(keep), dtype=bool)
        kept.append(int(keep.sum()))
        cols["index_i"].append(np.full(kept[-1], i, np.int64)), cols["index_j"].append(np.full(kept[-1], j, np.int64))
        for name in ("points_i", "points_j", "depth_i", "depth_j"):
            cols[name].append(m[name][keep])
    out = {k: np.concatenate(v) for k, v in cols.items()}
    out["kept"] = kept
    return out


def on_motion(points_i, points_j, motion):
    """Which correspondences move by ``motion`` = (dx, dy), within MOTION_TOLERANCE."""
    d = np.asarray(points_j, dtype=np.float64) - np.asarray(points_i, dtype=np.float64) - np.asarray(motion)
    return np.hypot(d[:, 0], d[:, 1]) <= MOTION_TOLERANCE


class Dataset:
    """A stand-in for HiveDataset over ``frames()``: RGB pictures with three equal channels (their gray conversion gives the gray picture back)."""

    def __init__(self, holes=True):
        gray, masks = frames()
        self.rgb_dataset = [sift_cases.gray_to_bgr(g) for g in gray]
        self.mask_dataset = [m.copy() for m in masks]
        self.depth_dataset = list(depth_stack(holes))
        self.num_frames = len(gray)
        self.camera_matrix = np.array([[120.0, 0.0, W / 2], [0.0, 120.0, H / 2], [0.0, 0.0, 1.0]], dtype=np.float32)


# ---- planted homographies ----
PLANTED_H = np.array([[0.98, 0.05, 12.0], [-0.04, 1.02, -7.5], [1.5e-5, -2.0e-5, 1.0]])
SECOND_H = np.array([[1.01, -0.03, -40.0], [0.02, 0.97, 55.0], [-1.0e-5, 2.5e-5, 1.0]])
# name -> (grid side, outliers, noise in pixels, seed)
PLANTED = {"small": (6, 10, 0.0, 0), "medium": (8, 40, 0.0, 1), "noisy": (9, 60, 0.5, 2)}


def project(Hm, pts):
    p = np.concatenate([np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))], axis=1) @ np.asarray(Hm).T
    return p[:, :2] / p[:, 2:]


def grid(side, width=640.0, height=480.0):
    xs, ys = np.linspace(40.0, width - 40.0, side), np.linspace(40.0, height - 40.0, side)
    return np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)


def planted(name):
    """(points_i, points_j, inliers): float32 (M, 2) twice and the planted mask; grid points mapped by PLANTED_H (plus uniform noise), rounded to float32, and
    uniform outliers, in a seeded order."""
    def make():
        side, outliers, noise, seed = PLANTED[name]
        rng = np.random.default_rng(seed)
        src = grid(side)
        dst = project(PLANTED_H, src) + rng.uniform(-noise, noise, src.shape)
        out_i, out_j = rng.uniform(0, (640, 480), (outliers, 2)), rng.uniform(0, (640, 480), (outliers, 2))
        order = rng.permutation(len(src) + outliers)
        pi, pj = np.concatenate([src, out_i])[order].astype(np.float32), np.concatenate([dst, out_j])[order].astype(np.float32)
        return pi, pj, (order < len(src))
    return _once(("planted", name), make)


def two_models(side=5):
    """Two disjoint planted models of equal size, interleaved: (points_i, points_j, which model)."""
    a, b = grid(side), grid(side) + 7.0
    pi = np.stack([a, b], axis=1).reshape(-1, 2)
    pj = np.stack([project(PLANTED_H, a), project(SECOND_H, b)], axis=1).reshape(-1, 2)
    return pi.astype(np.float32), pj.astype(np.float32), np.arange(len(pi)) % 2


def restated_planted(name, **kw):
    pi, pj, _ = planted(name)
    return _once(("restated_planted", name, tuple(sorted(kw.items()))), lambda: RR.ransac(pi, pj, **kw))
