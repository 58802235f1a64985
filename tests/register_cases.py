"""Cases for the frame-registration tests (tests/test_register_cpu.py, tests/test_register_gpu.py) and the figures measured on the CPU with the restatement
(tests/rigid_restatement.py).  Point sets for the Horn solver alone, planted transforms with outliers for the RANSAC, and a synthetic orbit: the 12 poses of
``tracking_cases.corner_orbit`` looking at seeded points on the room's floor and two walls.  Everything is computed once a process and shared."""
import numpy as np

import rigid_restatement as GR
import tracking_cases

# ---- measured on the CPU (tests/test_register_cpu.py prints each figure before it asserts) ----
# Sweeps of the cyclic Jacobi after which the off-diagonal norm is at most 2^-52 of the Frobenius norm on every matrix of ``horn_matrices()``; the kernel and the
# restatement run two more (RG_SWEEPS = SWEEPS = SWEEPS_MEASURED + 2).
SWEEPS_MEASURED = 5
# largest |v_jacobi -+ v_eigh| (the eigenvector of the largest eigenvalue, up to sign) over ``horn_matrices()``; the test asserts four times that
EIGENVECTOR_DEVIATION = 1.78e-13
# largest |A_horn - A_svd| and |t_horn - t_svd| over HORN_CASES (the restated solver against SVD Kabsch / Umeyama); the test asserts four times that
KABSCH_DEVIATION = 5.69e-14
# largest |R_horn - R_scipy| over the rotation-only HORN_CASES (scipy.spatial.transform.Rotation.align_vectors); the test asserts four times that
ALIGN_VECTORS_DEVIATION = 4.06e-15
# largest |T - planted| per case of PLANTED (the restated RANSAC, entries of the 3 x 4 part: the float32 rounding of the rows, and the planted noise of
# "noisy"); the tests allow four times that
PLANTED_DEVIATION = dict(camera=1.09e-8, clean=9.70e-9, forty=1.51e-8, noisy=9.56e-4, seventy=1.40e-8, similar=2.96e-8)
# ATE RMSE (metres, camera centres, anchored at the first pose) of the restated RANSAC + chain_pairs on the orbit; the test asserts four times that
ORBIT_ATE = 2.65e-8
# largest |t - (dx d / fx, dy d / fy, 0)| and |R - I| of the restated pipeline (restated SIFT, match, rigid RANSAC) on the blob frames over a constant-depth
# plane; the GPU test allows four times that
SHIFT_DEVIATION = 9.60e-5  # the translation; the rotation deviates by 1.11e-5

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def rotation(axis, degrees):
    """Rodrigues: float64 (3, 3)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def transform(R, t, s=1.0):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * np.asarray(R), t
    return T


# ---- the solver alone: name -> (points, axis, degrees, translation, scale, noise, seed, kind) ----
HORN_CASES = {
    "identity": (40, (0, 0, 1), 0.0, (0.0, 0.0, 0.0), 1.0, 0.0, 0, "cloud"),
    "small": (40, (1, 2, 3), 3.0, (0.02, -0.01, 0.03), 1.0, 0.0, 1, "cloud"),
    "quarter": (33, (0, 0, 1), 90.0, (0.5, 0.25, -1.0), 1.0, 0.0, 2, "cloud"),
    "large": (64, (1, -1, 0.5), 170.0, (-0.3, 0.8, 0.1), 1.0, 0.0, 3, "cloud"),
    "half_turn": (50, (1, 0, 0), 180.0, (0.0, 0.0, 0.0), 1.0, 0.0, 4, "cloud"),
    "scaled": (45, (2, -1, 1), 40.0, (0.1, 0.2, 0.3), 2.5, 0.0, 5, "cloud"),
    "shrunk": (45, (0, 1, 1), 75.0, (1.0, -2.0, 0.5), 0.5, 0.0, 6, "cloud"),
    "noisy": (200, (3, 1, -2), 25.0, (0.2, 0.1, -0.4), 1.0, 0.01, 7, "cloud"),
    "mirrored": (60, (0, 0, 1), 0.0, (0.0, 0.0, 0.0), 1.0, 0.0, 8, "mirror"),
    "planar": (36, (1, 1, 0), 35.0, (0.0, 0.3, 0.0), 1.0, 0.0, 9, "plane"),
    "minimal": (3, (1, 0, 2), 60.0, (0.4, 0.0, -0.2), 1.0, 0.0, 10, "cloud"),
    "far": (80, (0, 1, 0), 12.0, (5.0, -3.0, 2.0), 1.0, 0.001, 11, "far"),
}


def horn_case(name):
    """(p, q, T, with_scale): float32-rounded (M, 3) point sets as float64, the planted 4 x 4 and whether the case fits a scale."""
    def make():
        M, axis, deg, t, s, noise, seed, kind = HORN_CASES[name]
        rng = np.random.default_rng(100 + seed)
        p = rng.uniform(-1.0, 1.0, (M, 3)) + np.array([0.0, 0.0, 2.5])
        if kind == "plane":
            p[:, 2] = 2.0
        if kind == "far":
            p = p + np.array([100.0, -50.0, 30.0])
        T = transform(rotation(axis, deg), t, s)
        q = p @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((M, 3))
        if kind == "mirror":
            q = p * np.array([-1.0, 1.0, 1.0])
        return p.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64), T, s != 1.0
    return _once(("horn", name), make)


def centred(p, q):
    """The centroids and the centred sums of whole point sets in plain numpy sums (the solver's input; the order of the sums is not the matter of these cases)."""
    cp, cq = p.mean(axis=0), q.mean(axis=0)
    dp, dq = p - cp, q - cq
    return cp, cq, dp.T @ dq, float((dp * dp).sum()), float((dq * dq).sum())


# ---- planted transforms with outliers: name -> (points, outlier share, noise, with camera, with scale, seed) ----
PLANTED = {
    "clean": (120, 0.0, 0.0, False, False, 0),
    "forty": (150, 0.4, 0.0, False, False, 1),
    "seventy": (200, 0.7, 0.0, False, False, 2),
    "camera": (160, 0.4, 0.0, True, False, 3),
    "similar": (140, 0.4, 0.0, False, True, 4),
    "noisy": (180, 0.4, 0.004, False, False, 5),
}
PLANTED_T = transform(rotation((1, -2, 0.5), 14.0), (0.12, -0.05, 0.2))
PLANTED_S = transform(rotation((1, -2, 0.5), 14.0), (0.12, -0.05, 0.2), 1.6)
CAMERA = (525.0, 525.0, 319.5, 239.5)


def planted(name):
    """(rows float32 (M, 6), camera or None, T, inliers, with_scale).  Without a camera a row is X_i Y_i Z_i X_j Y_j Z_j; with one x_i y_i x_j y_j depth_i depth_j:
    the projections of the points, rounded to float32 (the back-projection of rounded pixels is the only noise then)."""
    def make():
        M, share, noise, with_camera, with_scale, seed = PLANTED[name]
        rng = np.random.default_rng(200 + seed)
        T = PLANTED_S if with_scale else PLANTED_T
        p = rng.uniform((-0.8, -0.6, 1.0), (0.8, 0.6, 3.0), (M, 3))
        q = p @ T[:3, :3].T + T[:3, 3] + noise * rng.standard_normal((M, 3))
        n_out = int(round(share * M))
        out = rng.permutation(M)[:n_out]
        q[out] = rng.uniform((-0.8, -0.6, 1.0), (0.8, 0.6, 3.0), (n_out, 3))
        inl = np.ones(M, dtype=bool)
        inl[out] = False
        if with_camera:
            fx, fy, cx, cy = CAMERA
            px = lambda a: np.stack([a[:, 0] / a[:, 2] * fx + cx, a[:, 1] / a[:, 2] * fy + cy], axis=1)
            rows = np.concatenate([px(p), px(q), p[:, 2:3], q[:, 2:3]], axis=1).astype(np.float32)
        else:
            rows = np.concatenate([p, q], axis=1).astype(np.float32)
        return rows, (CAMERA if with_camera else None), T, inl, with_scale
    return _once(("planted", name), make)


def restated_planted(name, **kw):
    rows, camera, _, _, with_scale = planted(name)
    return _once(("restated_planted", name, tuple(sorted(kw.items()))), lambda: GR.ransac(rows, camera, with_scale=with_scale, **kw))


def mixed(M, seed=5, words=6, share=0.25):
    """M rows (points layout, ``words`` wide; words past the sixth hold 7) of PLANTED_T, the first quarter replaced by outliers (none below 9 rows)."""
    rng = np.random.default_rng(seed + M)
    p = rng.uniform((-0.8, -0.6, 1.0), (0.8, 0.6, 3.0), (M, 3))
    q = p @ PLANTED_T[:3, :3].T + PLANTED_T[:3, 3]
    n_out = int(share * M) if M > 8 else 0
    q[:n_out] = rng.uniform((-0.8, -0.6, 1.0), (0.8, 0.6, 3.0), (n_out, 3))
    rows = np.full((M, words), 7.0, dtype=np.float32)
    rows[:, :3], rows[:, 3:6] = p, q
    return rows


def horn_matrices():
    """Horn's 4 x 4 matrices of every committed case, (K, 4, 4): the whole point sets of HORN_CASES and the minimal samples of the first 256 trials of PLANTED."""
    def make():
        import ransac_restatement as RR
        mats = [GR.horn_matrix(centred(*horn_case(name)[:2])[2][None]) for name in sorted(HORN_CASES)]
        for name in sorted(PLANTED):
            rows, camera, _, _, _ = planted(name)
            p, q = GR.back_project(rows, camera)
            sample = GR.draw3(RR.base_key(0, (0, 0)), np.arange(256), len(rows))
            sp, sq = p[sample], q[sample]
            cp, cq = sp.mean(axis=1, keepdims=True), sq.mean(axis=1, keepdims=True)
            mats.append(GR.horn_matrix(np.einsum("tka,tkb->tab", sp - cp, sq - cq)))
        return np.concatenate(mats)
    return _once("horn_matrices", make)


# ---- the synthetic orbit ----
ORBIT_HW = (480, 640)
ORBIT_POINTS, ORBIT_SEED, ORBIT_OUTLIERS, ORBIT_TRIALS, ORBIT_MIN_INLIERS = 360, 21, 0.4, 512, 20


def orbit():
    """A dict: ``poses`` (12, 4, 4) world -> camera (the truth), ``K``, ``pairs`` (hierarchical), ``rows`` a list of float32 (M_p, 8) rows of the kind
    ``match_pairs`` writes -- the projections of seeded points on the floor and the two walls at the corner, positions and depths rounded to float32, 40 % of every
    pair's rows replaced by outliers -- and ``frames``: per frame (pixels float32 (N, 2), depth float32 (N,), visible (N,))."""
    def make():
        from hive_amd.pose_optimisation import FrameSamplingMode, sample_frame_pairs
        c2w = tracking_cases.corner_orbit(12)
        w2c = np.linalg.inv(c2w)
        H, W = ORBIT_HW
        K = tracking_cases.intrinsics(H, W).astype(np.float64)
        rng = np.random.default_rng(ORBIT_SEED)
        hi, n = tracking_cases.ROOM_HI, ORBIT_POINTS // 3
        u, v = rng.uniform(hi - 0.9, hi, (3, n)), rng.uniform(hi - 0.9, hi, (3, n))
        world = np.concatenate([np.stack([u[0], np.full(n, hi), v[0]], axis=1), np.stack([np.full(n, hi), u[1], v[1]], axis=1),
                                np.stack([u[2], v[2], np.full(n, hi)], axis=1)])
        frames = []
        for G in w2c:
            cam = world @ G[:3, :3].T + G[:3, 3]
            x, y = cam[:, 0] / cam[:, 2] * K[0, 0] + K[0, 2], cam[:, 1] / cam[:, 2] * K[1, 1] + K[1, 2]
            visible = (cam[:, 2] > 0.1) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            frames.append((np.stack([x, y], axis=1).astype(np.float32), cam[:, 2].astype(np.float32), visible))
        pairs = sample_frame_pairs(FrameSamplingMode.Hierarchical, 12)
        rows = []
        for i, j in pairs:
            both = np.nonzero(frames[i][2] & frames[j][2])[0]
            r = np.zeros((len(both), 8), dtype=np.float32)
            r[:, 0:2], r[:, 2:4], r[:, 4], r[:, 5] = frames[i][0][both], frames[j][0][both], frames[i][1][both], frames[j][1][both]
            r[:, 6:8] = both[:, None].astype(np.int32).view(np.float32)
            out = rng.permutation(len(both))[:int(ORBIT_OUTLIERS * len(both))]
            r[out, 2:4] = rng.uniform((0, 0), (W - 1, H - 1), (len(out), 2))
            r[out, 5] = rng.uniform(0.4, 1.6, len(out))
            rows.append(r)
        return dict(poses=w2c, K=K, pairs=pairs, rows=rows, frames=frames)
    return _once("orbit", make)


def restated_orbit():
    """The restated RANSAC of every orbit pair and ``chain_pairs`` of them: (fits, poses, depth_scale, lost)."""
    def make():
        from hive_amd.registration import chain_pairs
        o = orbit()
        camera = GR.camera_of(o["K"])
        fits = [GR.ransac(r, camera, trials=ORBIT_TRIALS, pair_key=key, min_count=ORBIT_MIN_INLIERS) for r, key in zip(o["rows"], o["pairs"])]
        T, scale = np.stack([f["T"] for f in fits]), np.array([f["scale"] for f in fits])
        result = np.array([[f["trial"], f["winner_count"], f["count"]] for f in fits])
        return (fits,) + chain_pairs(12, o["pairs"], T, scale, result, min_inliers=ORBIT_MIN_INLIERS, first_pose=o["poses"][0])
    return _once("restated_orbit", make)


def ate_rmse(poses, truth):
    """Root mean square distance of the camera centres of two world -> camera trajectories (no alignment: both are anchored at the first pose)."""
    centre = lambda G: -np.einsum("nji,nj->ni", G[:, :3, :3], G[:, :3, 3])
    d = centre(np.asarray(poses)) - centre(np.asarray(truth))
    return float(np.sqrt((d * d).sum(axis=1).mean()))


# ---- the blob frames over a constant-depth plane: a pure pixel shift ----
SHIFT_DEPTH, SHIFT_PAIR = 2.0, (0, 1)


class ShiftDataset:
    """``feature_cases.Dataset`` with every depth map the constant SHIFT_DEPTH: with the instance masks applied, frames 0 and 1 differ by the background's pixel
    shift alone, which a fronto-parallel plane at depth d turns into the translation (dx d / fx, dy d / fy, 0) and no rotation."""

    def __init__(self):
        import feature_cases
        base = feature_cases.Dataset(holes=False)
        self.rgb_dataset, self.mask_dataset, self.num_frames, self.camera_matrix = base.rgb_dataset, base.mask_dataset, base.num_frames, base.camera_matrix
        self.depth_dataset = [np.full((feature_cases.H, feature_cases.W), SHIFT_DEPTH, dtype=np.float32) for _ in range(self.num_frames)]


def shift_expected():
    import feature_cases
    K = feature_cases.Dataset(holes=False).camera_matrix.astype(np.float64)
    dx, dy = feature_cases.BACKGROUND_MOTION
    return np.array([dx * SHIFT_DEPTH / K[0, 0], dy * SHIFT_DEPTH / K[1, 1], 0.0])


def restated_shift():
    """The restated pipeline on the pair SHIFT_PAIR of ``ShiftDataset`` with the masks applied: (match, fit) of ``ransac_restatement.match_filter`` and
    ``rigid_restatement.ransac``."""
    def make():
        import feature_cases
        import ransac_restatement as RR
        i, j = SHIFT_PAIR
        data = ShiftDataset()
        (kp_i, d_i), (kp_j, d_j) = feature_cases.restated_sift(i, True), feature_cases.restated_sift(j, True)
        m = RR.match_filter(kp_i, d_i, kp_j, d_j, data.depth_dataset[i], data.depth_dataset[j], 0.7, feature_cases.MIN_FEATURES)
        rows = np.concatenate([m["points_i"], m["points_j"], m["depth_i"][:, None], m["depth_j"][:, None]], axis=1).astype(np.float32)
        fit = GR.ransac(rows, GR.camera_of(data.camera_matrix), pair_key=(i, j), min_count=feature_cases.MIN_FEATURES)
        return m, fit
    return _once("restated_shift", make)
