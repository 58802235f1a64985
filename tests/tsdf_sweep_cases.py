"""Scenes for the fused TSDF sweep's oracle tests (test_tsdf_sweep_cases_cpu.py, test_tsdf_sweep_gpu.py), and a Python restatement of how
``hive_tsdf_integrate_batch`` groups the frames of a batch into sweeps.  numpy only: nothing here touches the GPU library, so the premises
of the GPU tests (which groups form, which cameras are where, what the oracle updates) are checked on any machine.

Every generator is seeded and deterministic; a scene is a dict with ``bounds`` (3, 2), ``voxel``, ``K`` (3, 3) float32, ``poses`` (N, 4, 4)
camera-to-world, ``color`` (N, H, W, 3) uint8, ``depth`` {kind: (N, H, W) float32} and, where the generator decides them, the intended
``lengths`` of the groups."""
import numpy as np

BOUNDS = np.array([[-1.0, 1.1], [-0.8, 1.0], [0.2, 2.6]])

# (voxel, dims, (H, W), fx, fy): the three configurations of the random pose groups; cx = W/2 - 0.3, cy = H/2 + 0.7 (fx != fy, principal
# point off centre).  X*Y % 4 == 2 in the first (the work list's last quad of rows is ragged); W % 4 != 0 in the first and the third (scalar
# frame pre-pass); Z < 64 and odd in the third (every row is one ragged segment).
CONFIGS = [
    dict(name="v030", voxel=0.03, dims=(70, 61, 80), image=(37, 53), fx=40.0, fy=46.0, seed=100),
    dict(name="v050", voxel=0.05, dims=(42, 36, 48), image=(48, 64), fx=47.0, fy=46.0, seed=104),
    dict(name="v041", voxel=0.041, dims=(52, 44, 59), image=(61, 45), fx=54.0, fy=46.0, seed=102),
]
# A fourth one for the per-row far cut only.  The cut reads a 3 x 3-dilated table of per-tile depth maxima (32-pixel tiles); the images
# above have 2 x 2 tiles, where every dilated entry is the frame's maximum and the cut can never beat the frame-wide one.  Five tile
# columns leave it room: a row whose image segment stays in the near columns is cut at their depth.
WIDE = dict(name="wide", voxel=0.05, dims=(42, 36, 48), image=(33, 131), fx=110.0, fy=46.0, seed=103)

FUSE_COS = 0.809017  # cos 36 degrees: largest angle between the optical axes of a frame and its group's first frame
FUSE_DIST = 0.25     # largest camera distance to the group's first frame, in longest grid sides
MAXF = 4             # frames per fused sweep


def dims_of(bounds, voxel):
    """Voxels per axis, the library's rule: ceil((max - min) / voxel) in double."""
    b = np.asarray(bounds, np.float64)
    return tuple(int(np.ceil((b[a, 1] - b[a, 0]) / float(voxel))) for a in range(3))


def longest_side(bounds, voxel):
    """Longest side of the grid in metres as the host computes it: voxels x the float32 voxel size."""
    return float(max(dims_of(bounds, voxel))) * float(np.float32(voxel))


def fuse_measures(pose_first, pose_other, side):
    """(angle between the optical axes in degrees, camera distance in longest grid sides) of a frame against a group's first frame."""
    a, b = np.asarray(pose_first, np.float64), np.asarray(pose_other, np.float64)
    za, zb = a[:3, 2], b[:3, 2]
    c = float(za @ zb) / (np.linalg.norm(za) * np.linalg.norm(zb))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(a[:3, 3] - b[:3, 3])) / side


def fusable(pose_first, pose_other, side):
    """`fusable` of hive_tsdf_integrate_batch, restated."""
    a, b = np.asarray(pose_first, np.float64), np.asarray(pose_other, np.float64)
    za, zb = a[:3, 2], b[:3, 2]
    d = a[:3, 3] - b[:3, 3]
    return bool(za @ zb >= FUSE_COS * np.sqrt(za @ za) * np.sqrt(zb @ zb) and d @ d <= FUSE_DIST * FUSE_DIST * side * side)


def predict_groups(poses, side):
    """Greedy grouping: a group grows to at most MAXF frames, while the next frame is fusable with the group's FIRST frame."""
    n, f, groups = len(poses), 0, []
    while f < n:
        nf = 1
        while nf < MAXF and f + nf < n and fusable(poses[f], poses[f + nf], side):
            nf += 1
        groups.append(nf)
        f += nf
    return groups


def decisions(poses, side):
    """Every fusable / not-fusable decision the greedy rule takes on these poses: (first frame, tested frame, angle, distance, outcome)."""
    n, f, out = len(poses), 0, []
    while f < n:
        nf = 1
        while nf < MAXF and f + nf < n:
            ok = fusable(poses[f], poses[f + nf], side)
            out.append((f, f + nf) + fuse_measures(poses[f], poses[f + nf], side) + (ok,))
            if not ok:
                break
            nf += 1
        f += nf
    return out


def group_starts(groups):
    return [int(s) for s in np.cumsum([0] + list(groups[:-1]))]


def lanes_along_y(pose):
    """The host's choice of the work list's row decomposition, from a sweep's first pose (launch_integrate_multi)."""
    return abs(pose[0, 1]) > abs(pose[1, 1])


def rotvec_matrix(v):
    """Rodrigues' formula."""
    v = np.asarray(v, np.float64)
    th = float(np.linalg.norm(v))
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def random_rotation(rng):
    """Uniform over SO(3): a normalised Gaussian quaternion."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_pose(R, t):
    p = np.eye(4)
    p[:3, :3], p[:3, 3] = R, t
    return p


def intrinsics(cfg):
    H, W = cfg["image"]
    return np.array([[cfg["fx"], 0, W / 2 - 0.3], [0, cfg["fy"], H / 2 + 0.7], [0, 0, 1]], np.float32)


def _lengths_ok(lengths):
    has_all = set(lengths) == {1, 2, 3, 4}
    lone = any(lengths[i] == 1 and lengths[i - 1] > 1 and lengths[i + 1] > 1 for i in range(1, len(lengths) - 1))
    three = any(g == 3 for g in lengths[:-1])
    return has_all and lone and three


def draw_lengths(rng, frames=24):
    """Group lengths from 1..4 until about `frames` frames, redrawn until the list has every length, a 1 between two longer groups and a 3
    that is not the last group."""
    while True:
        lengths = []
        while sum(lengths) < frames:
            lengths.append(int(rng.integers(1, MAXF + 1)))
        if _lengths_ok(lengths):
            return lengths


def noise_depth(rng, n, H, W):
    d = rng.uniform(0.2, 4.0, (n, H, W)).astype(np.float32)
    d[rng.random((n, H, W)) < 0.15] = 0.0
    return d


def patchy_depth(rng, n, H, W, near_columns=None):
    """Most 32-pixel tiles all zero, a few near tiles at 0.3 .. 0.8 m (in `near_columns` of the tile grid if given), one far pixel at 4 m
    (in the last tile column if `near_columns` is given)."""
    d = np.zeros((n, H, W), np.float32)
    ty, tx = (H + 31) // 32, (W + 31) // 32
    for i in range(n):
        cols = range(tx) if near_columns is None else near_columns
        tiles = [(a, b) for a in range(ty) for b in cols]
        picks = [t for t in tiles if rng.random() < 0.3] or [tiles[int(rng.integers(len(tiles)))]]
        for a, b in picks:
            blk = d[i, 32 * a:32 * a + 32, 32 * b:32 * b + 32]
            blk[:] = rng.uniform(0.3, 0.8, blk.shape).astype(np.float32)
        far_x = int(rng.integers(W)) if near_columns is None else int(rng.integers(32 * (tx - 1), W))
        d[i, int(rng.integers(H)), far_x] = 4.0
    return d


_scene_cache = {}


def random_pose_scene(cfg):
    """Groups of frames around random base poses.  Base: rotation uniform over SO(3), position uniform in [-1.5, 1.5]^3 + (0, 0, 1);
    followers: the base turned by a rotation vector of sigma 0.12 rad and moved by sigma 0.08 m.  A base is redrawn until every decision
    the greedy rule can take on it has margin (see test_tsdf_sweep_cases_cpu.py): not fusable with the previous group's first frame, with
    no angle in [30, 45] degrees and no distance in [0.2, 0.3] sides; followers are redrawn until they are within 30 degrees and 0.2
    sides of their base.  In the first group of four the second frame's depth is all zero (a frame that updates nothing inside a group)."""
    if cfg["name"] in _scene_cache:
        return _scene_cache[cfg["name"]]
    rng = np.random.default_rng(cfg["seed"])
    H, W = cfg["image"]
    side = longest_side(BOUNDS, cfg["voxel"])
    lengths = draw_lengths(rng)
    poses, prev_first = [], None
    for g in lengths:
        while True:
            base = make_pose(random_rotation(rng), rng.uniform(-1.5, 1.5, 3) + np.array([0.0, 0.0, 1.0]))
            if prev_first is None:
                break
            ang, dist = fuse_measures(prev_first, base, side)
            if (ang > 45.0 or dist > 0.3) and not (30.0 <= ang <= 45.0) and not (0.2 <= dist <= 0.3):
                break
        poses.append(base)
        for _ in range(g - 1):
            while True:
                p = make_pose(base[:3, :3] @ rotvec_matrix(rng.normal(scale=0.12, size=3)), base[:3, 3] + rng.normal(scale=0.08, size=3))
                ang, dist = fuse_measures(base, p, side)
                if ang < 30.0 and dist < 0.2:
                    break
            poses.append(p)
        prev_first = base
    poses = np.stack(poses)
    n = len(poses)
    wide = cfg["name"] == "wide"
    depth = {"noise": noise_depth(rng, n, H, W), "patchy": patchy_depth(rng, n, H, W, near_columns=(0, 1) if wide else None)}
    zero_frame = group_starts(lengths)[lengths.index(4)] + 1
    for d in depth.values():
        d[zero_frame] = 0.0
    scene = dict(name=cfg["name"], bounds=BOUNDS, voxel=cfg["voxel"], K=intrinsics(cfg), poses=poses, depth=depth, lengths=lengths,
                 color=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), zero_frame=zero_frame)
    _scene_cache[cfg["name"]] = scene
    return scene


def chunk_straddle_scene():
    """135 frames of 24 x 32 into [0, 1.6]^3 at 0.05 (32^3): three frames at one base pose, 132 at a second one 60 degrees and 0.9 sides
    away, each with small jitter.  Groups [3] + [4] * 33: the group at frame 127 straddles frame 128, the end of the first prepared chunk."""
    rng = np.random.default_rng(7)
    bounds = np.array([[0.0, 1.6], [0.0, 1.6], [0.0, 1.6]])
    H, W, n = 24, 32, 135
    K = np.array([[26.0, 0, W / 2 - 0.5], [0, 25.0, H / 2 - 0.5], [0, 0, 1]], np.float32)
    base_a = make_pose(np.eye(3), [0.8, 0.8, -0.6])
    base_b = make_pose(rotvec_matrix([0.0, np.radians(60.0), 0.0]), [-0.5, 0.8, 0.0])
    poses = []
    for i in range(n):
        b = base_a if i < 3 else base_b
        poses.append(make_pose(b[:3, :3] @ rotvec_matrix(rng.normal(scale=0.01, size=3)), b[:3, 3] + rng.normal(scale=0.005, size=3)))
    depth = rng.uniform(0.3, 2.5, (n, H, W)).astype(np.float32)
    depth[rng.random((n, H, W)) < 0.1] = 0.0
    return dict(name="straddle", bounds=bounds, voxel=0.05, K=K, poses=np.stack(poses), depth={"noise": depth}, lengths=[3] + [4] * 33,
                color=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8))


SPECIAL_VALUES = {"nan": np.float32(np.nan), "inf": np.float32(np.inf), "neg": np.float32(-0.05), "negzero": np.float32(-0.0)}
SPECIAL_BLOCKS = {"nan": (20, 30), "inf": (8, 50), "neg": (36, 10), "negzero": (6, 6)}  # top-left corner of each 4 x 4 block
SPECIAL_PLANE = 0.5  # depth of every other pixel, metres


def special_depth_scene(kind):
    """A 48 x 64 frame of 0.5 m with a 4 x 4 block of a special value (`kind` in SPECIAL_VALUES: the block at rows 20..23, columns 30..33;
    "all": the four blocks of SPECIAL_BLOCKS together), identity rotation, camera at (0.05, 0.1, 0) in front of the volume; four copies under
    small jitter, so that frames [:2] are a fused pair and [:4] a fused four.  A NaN depth passes the contract's tests (`depth != 0`,
    `!(diff < -trunc)`) and updates EVERY voxel in front of the camera that rounds to the pixel, with dist = fminf(1, NaN) = 1; +inf the same."""
    rng = np.random.default_rng(11)
    H, W = 48, 64
    K = np.array([[50.0, 0, 31.5], [0, 50.0, 23.5], [0, 0, 1]], np.float32)
    frame = np.full((H, W), SPECIAL_PLANE, np.float32)
    if kind == "all":
        for k, (r, c) in SPECIAL_BLOCKS.items():
            frame[r:r + 4, c:c + 4] = SPECIAL_VALUES[k]
    else:
        frame[20:24, 30:34] = SPECIAL_VALUES[kind]
    base = make_pose(np.eye(3), [0.05, 0.1, 0.0])
    poses = [base] + [make_pose(rotvec_matrix(rng.normal(scale=0.01, size=3)), base[:3, 3] + rng.normal(scale=0.01, size=3)) for _ in range(3)]
    return dict(name="special_" + kind, bounds=BOUNDS, voxel=0.05, K=K, poses=np.stack(poses), depth={"plane": np.stack([frame] * 4)},
                color=rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8))


def degenerate_scene():
    """A volume of 5 x 3 x 3 voxels (X*Y odd, Z < 4: one ragged quad per row, one ragged quad of rows; every quotient exact in binary),
    four frames in front of it that see all of it."""
    rng = np.random.default_rng(13)
    bounds = np.array([[0.0, 0.625], [0.0, 0.375], [0.5, 0.875]])
    H, W = 24, 32
    K = np.array([[30.0, 0, 15.2], [0, 28.0, 12.3], [0, 0, 1]], np.float32)
    base = make_pose(np.eye(3), [0.3, 0.2, -0.2])
    poses = [base] + [make_pose(rotvec_matrix(rng.normal(scale=0.03, size=3)), base[:3, 3] + rng.normal(scale=0.02, size=3)) for _ in range(3)]
    depth = rng.uniform(0.6, 1.3, (4, H, W)).astype(np.float32)
    depth[rng.random((4, H, W)) < 0.1] = 0.0
    return dict(name="degenerate", bounds=bounds, voxel=0.125, K=K, poses=np.stack(poses), depth={"noise": depth},
                color=rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------
# The oracle's side, computed once per (scene, depth kind, round mode, weights) and shared read-only between the tests of a session.
_oracle_cache = {}


def oracle_run(oracle, scene, kind, round_mode=1, weights=(1.0,), frames=None):
    """The frames (all, or `frames`) integrated once per weight in `weights`, in order, by the C oracle.  Returns a dict: `passes` = the three
    planes (tsdf, color, weight) after each pass, `n_updated` = voxels written per frame (of the first pass: the count does not depend on
    the volume's state).  Cached: callers must not modify what they get."""
    frames = list(range(len(scene["poses"]))) if frames is None else list(frames)
    key = (scene["name"], kind, int(round_mode), tuple(float(w) for w in weights), tuple(frames))
    if key not in _oracle_cache:
        ora = oracle.TSDFVolume(scene["bounds"], scene["voxel"], round_mode=round_mode)
        passes, counts = [], []
        for k, w in enumerate(weights):
            for i in frames:
                ora.integrate(scene["color"][i], scene["depth"][kind][i], scene["K"], scene["poses"][i], obs_weight=w)
                if k == 0:
                    counts.append(int(ora.last_n_updated))
            passes.append((ora._tsdf.copy(), ora._color.copy(), ora._weight.copy()))
        _oracle_cache[key] = dict(passes=passes, n_updated=counts, dims=tuple(int(v) for v in ora._vol_dim), origin=ora._vol_origin.copy())
    return _oracle_cache[key]


def camera_depth_of_voxels(scene, pose):
    """cam_z of every voxel centre for `pose` (float64; for counting voxels beyond a depth, not for bit parity)."""
    dims = dims_of(scene["bounds"], scene["voxel"])
    o = np.asarray(scene["bounds"], np.float64)[:, 0]
    g = np.meshgrid(*[o[a] + np.arange(dims[a]) * scene["voxel"] for a in range(3)], indexing="ij")
    p = np.stack(g, -1) - pose[:3, 3]
    return p @ pose[:3, 2]


# ---------------------------------------------------------------------------------------------
# A volume far from the world origin.  The work list's analytic row clip (tsdf.hip clip_row) turns a cut position tz into a voxel index
# through `lo + T[2] - oz`: at z ~ 131072 m that sum rounds to 2^-6 m = a quarter of a 62.5 mm voxel (an error of up to an eighth), more than
# the half pixel by which the clip's image bounds are padded wherever a voxel step moves the projection by more than four pixels (cam_z
# below ~0.7 m here).  What keeps such rows whole is the clip's last safety margin, the widening of the voxel interval by 2 / 3 voxels; no
# scene near the origin needs it (updates_outside_clip below counts none for them).  The voxel centres themselves stay exact: 2^-4 m apart.
FAR_OFFSET_BOUNDS = np.array([[-1.0, 1.5], [-0.75, 1.5], [131072.0, 131075.0]])  # 40 x 36 x 48 voxels of 0.0625: every quotient exact in binary


def far_offset_scene():
    """Three groups of four frames (random rotations, cameras in and around the volume, small jitter inside a group), 48 x 64 noise depth."""
    rng = np.random.default_rng(21)
    H, W, voxel = 48, 64, 0.0625
    side = longest_side(FAR_OFFSET_BOUNDS, voxel)
    lo, hi = FAR_OFFSET_BOUNDS[:, 0] - 0.3, FAR_OFFSET_BOUNDS[:, 1] + 0.3
    poses, prev = [], None
    for _ in range(3):
        while True:
            base = make_pose(random_rotation(rng), rng.uniform(lo, hi))
            if prev is None:
                break
            ang, dist = fuse_measures(prev, base, side)
            if (ang > 45.0 or dist > 0.3) and not (30.0 <= ang <= 45.0) and not (0.2 <= dist <= 0.3):
                break
        poses.append(base)
        for _ in range(3):
            poses.append(make_pose(base[:3, :3] @ rotvec_matrix(rng.normal(scale=0.05, size=3)), base[:3, 3] + rng.normal(scale=0.03, size=3)))
        prev = base
    n = len(poses)
    K = np.array([[47.0, 0, W / 2 - 0.3], [0, 46.0, H / 2 + 0.7], [0, 0, 1]], np.float32)
    return dict(name="far_offset", bounds=FAR_OFFSET_BOUNDS, voxel=voxel, K=K, poses=np.stack(poses), depth={"noise": noise_depth(rng, n, H, W)},
                color=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), lengths=[4, 4, 4])


def clip_rows(scene, pose, far, widen=True):
    """tsdf.hip clip_row restated in float32 numpy for every (x, y) row of the scene's volume, frame-wide far cut only (`far` = the
    frame's largest depth): the half-open voxel interval [z0, z1) per row, with or without the final widening by 2 / 3 voxels."""
    f32 = np.float32
    X, Y, Z = dims_of(scene["bounds"], scene["voxel"])
    H, W = scene["depth"][next(iter(scene["depth"]))].shape[1:]
    o = np.asarray(scene["bounds"], np.float64)[:, 0].astype(f32)
    vs, trunc = f32(scene["voxel"]), f32(5.0 * scene["voxel"])
    K = np.asarray(scene["K"], f32)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P = np.asarray(pose, np.float64).astype(f32)
    R, T = P[:3, :3], P[:3, 3]
    tx = ((o[0] + np.arange(X, dtype=f32) * vs) - T[0])[:, None]
    ty = ((o[1] + np.arange(Y, dtype=f32) * vs) - T[1])[None, :]
    ax, ay, az = R[0, 0] * tx + R[1, 0] * ty, R[0, 1] * tx + R[1, 1] * ty, R[0, 2] * tx + R[1, 2] * ty
    bx, by, bz = R[2, 0], R[2, 1], R[2, 2]
    lo = np.full((X, Y), (o[2] - T[2]) - vs, f32)
    hi = np.full((X, Y), ((o[2] + f32(Z) * vs) - T[2]) + vs, f32)
    empty = np.zeros((X, Y), bool)

    def cut(alpha, beta):  # keep alpha + beta * tz >= 0
        nonlocal lo, hi, empty
        alpha = np.broadcast_to(np.asarray(alpha, f32), (X, Y))
        if beta > 0:
            lo = np.maximum(lo, -alpha / f32(beta))
        elif beta < 0:
            hi = np.minimum(hi, -alpha / f32(beta))
        else:
            empty = empty | (alpha < 0)

    far = f32(far)
    one = f32(1.0)
    slack = f32(1.0e-5) * (one + np.abs(az) + far)
    cut(az + slack, bz)
    cut((far + trunc - az) + slack, -bz)
    cut(fx * ax + (cx + one) * az, fx * bx + (cx + one) * bz)
    cut((f32(W) - cx) * az - fx * ax, (f32(W) - cx) * bz - fx * bx)
    cut(fy * ay + (cy + one) * az, fy * by + (cy + one) * bz)
    cut((f32(H) - cy) * az - fy * ay, (f32(H) - cy) * bz - fy * by)
    inv = one / vs
    zf0 = np.floor((lo + T[2] - o[2]) * inv) - (f32(2.0) if widen else f32(0.0))
    zf1 = np.ceil((hi + T[2] - o[2]) * inv) + (f32(3.0) if widen else f32(0.0))
    z0 = np.clip(zf0, 0, Z).astype(np.int64)
    z1 = np.clip(zf1, 0, Z).astype(np.int64)
    dead = empty | ~(lo <= hi)
    z0[dead] = z1[dead] = 0
    return z0, z1


def updates_outside_clip(oracle, scene, kind, frame, widen):
    """Voxels the oracle updates for one frame that lie outside the restated clip of their row."""
    ora = oracle.TSDFVolume(scene["bounds"], scene["voxel"])
    d = scene["depth"][kind][frame]
    ora.integrate(scene["color"][frame], d, scene["K"], scene["poses"][frame])
    z0, z1 = clip_rows(scene, scene["poses"][frame], float(np.max(d)), widen)
    z = np.arange(ora._weight.shape[2])[None, None, :]
    return int(np.count_nonzero((ora._weight > 0) & ((z < z0[..., None]) | (z >= z1[..., None])))), int(ora.last_n_updated)
