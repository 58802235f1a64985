"""Cases for csrc/geometry.hip at the shapes where its guarded code runs (tests/test_geometry_cases_cpu.py proves that they reach it, on the CPU;
tests/test_geometry_edges_gpu.py runs them on the GPU), and the reference's formulas (hive/geometric.py:107-206, the frustum of its fusion library, the depth
hand-off of hive/dataset_adaptors.py:1432-1433 and hive/io.py:1032-1039) in plain numpy.  No GPU, no library of this project."""
import numpy as np

HALF_EVEN, HALF_AWAY = 0, 1

# ---- unprojection --------------------------------------------------------------------------------------------------------------------------------------
UNPROJECT_SIZES = [(1, 1), (5, 7), (37, 53), (33, 31), (1025, 1025)]
TILE = 1024  # pixels per workgroup of unproject_count_kernel / unproject_write_kernel (UP_TILE): the cases place their forced pixels by it


def rotation(axis, angle):
    """Rodrigues' formula, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Wx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Wx + (1.0 - np.cos(angle)) * (Wx @ Wx)


def unproject_case(H, W, seed):
    """float32 depth in [0.5, 5] with ~10 % zeros, a ~90 % mask, uint8 rgb, float32 K, a rotation about a skew axis and a translation.  The last pixel is
    valid, and so is the last pixel of the last whole tile: a lost ragged tail changes the count and the last row, and a tail that overwrote the tile before
    it changes that row."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 5.0, size=(H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.10] = 0.0
    mask = rng.random((H, W)) < 0.9
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    n = H * W
    forced = [n - 1]
    if n > TILE:
        forced.append((n - 1) // TILE * TILE - 1)
    for i in forced:
        depth.reshape(-1)[i] = np.float32(0.75 + 0.5 * (i % 7))
        mask.reshape(-1)[i] = True
    f = np.float32(0.9 * max(H, W) + 1.0)
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f * np.float32(1.0625), (H - 1) / 2.0], [0, 0, 1]], np.float32)
    R = rotation([0.3, -0.5, 0.8], 0.7)
    t = np.array([[0.31], [-0.17], [0.23]], np.float64)
    return dict(depth=depth, mask=mask, rgb=rgb, K=K, R=R, t=t)


def kinv(K):
    """The reference inverts K in K's own dtype (geometric.py:203); the library takes the result widened to float64."""
    return np.ascontiguousarray(np.linalg.inv(K), dtype=np.float64)


def image2world_formula(points, depth, K, R, t, scale_factor=1.0):
    """geometric.py:183-206, as written there."""
    points2d = np.vstack((points.T * scale_factor, np.ones(points.shape[0])))
    points_camera_space = np.linalg.inv(K) @ points2d
    return (R.T @ (depth * points_camera_space - t)).T


def unproject_formula(depth, mask, K, R, t, rgb=None):
    """geometric.py:107-152, as written there -> (points, rgba or None)."""
    valid = (np.ones(depth.shape, bool) if mask is None else mask) & (depth > 0.0)
    V, U = valid.nonzero()
    points = image2world_formula(np.array([U, V]).T, depth[valid], K, R, t)
    if rgb is None:
        return points, None
    colour = np.zeros((len(points), 4), rgb.dtype)
    colour[:, :3] = rgb[valid]
    colour[:, 3] = 255
    return points, colour


def project_formula(points, K, R, t, scale_factor=1.0, integer=True, round_mode=HALF_EVEN):
    """geometric.py:155-180, as written there; ``round_mode`` HALF_AWAY replaces its np.round by C's round()."""
    c = K @ (R @ points.T + t)
    depth = c[2, :]
    uv = c[0:2, :] / depth / scale_factor
    if integer:
        uv = np.round(uv) if round_mode == HALF_EVEN else np.copysign(np.floor(np.abs(uv) + 0.5), uv)
        return np.array(uv.T, dtype=np.int32), depth
    return uv.T.copy(), depth


# ---- projection: exact half-pixel ties -----------------------------------------------------------------------------------------------------------------
# fx, fy powers of two and cx, cy whole numbers: every step of the projection of a tie point is exact in float64
TIE_K = np.array([[64.0, 0.0, 1.0], [0.0, 32.0, 2.0], [0.0, 0.0, 1.0]])
TIE_W, TIE_H = 3, 5  # the image of the bounding-box test: ties at -0.5 on its left and top borders, at 2.5 on its right border
TIE_HALVES = [k + 0.5 for k in range(-3, 4)]
TIE_COUNT = 7 + 7 + 49
NON_TIES = 300


def _world_points(K, u, v, z):
    return np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], axis=1)


def tie_points(K=TIE_K):
    """float64 world points [TIE_COUNT + NON_TIES][3] for the identity pose.  The first TIE_COUNT project exactly onto k + 0.5, k = -3 .. 3: 7 in u alone
    (v = 1.25), 7 in v alone (u = 1.25), 49 in both; depths 1, 2 and 4.  Then NON_TIES seeded points around and inside the image, none of which rounds to
    row 0 or column 0 in either mode, so the ties alone decide the minima of the bounding box."""
    h = np.array(TIE_HALVES)
    u = np.concatenate([h, np.full(7, 1.25), np.repeat(h, 7)])
    v = np.concatenate([np.full(7, 1.25), h, np.tile(h, 7)])
    z = np.array([1.0, 2.0, 4.0])[np.arange(TIE_COUNT) % 3]
    rng = np.random.default_rng(31)
    nu, nv = rng.uniform(-6.0, TIE_W + 6.0, NON_TIES), rng.uniform(-6.0, TIE_H + 6.0, NON_TIES)
    nu = np.where(np.abs(nu) < 0.75, nu + 2.0, nu)
    nv = np.where(np.abs(nv) < 0.75, nv + 2.0, nv)
    nz = rng.uniform(1.0, 4.0, NON_TIES)
    return np.concatenate([_world_points(K, u, v, z), _world_points(K, nu, nv, nz)])


def bbox_of(uv, W, H):
    """{min u, max u, min v, max v, count} of the pixels inside [0, W) x [0, H), as hive_project_bbox returns it."""
    vis = uv[(uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)]
    if len(vis) == 0:
        return [np.iinfo(np.int32).max, np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0]
    return [int(vis[:, 0].min()), int(vis[:, 0].max()), int(vis[:, 1].min()), int(vis[:, 1].max()), len(vis)]


# ---- ICP: every association an exact tie -----------------------------------------------------------------------------------------------------------------
def icp_tie_case():
    """5 x 7, identity poses, K = [[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]] and live_v[v, u] = (u, v, 1): pixel (u, v) projects exactly onto (u + 0.5, v + 0.5).
    Half-even sends it to the even neighbour, half-away to (u + 1, v + 1), which leaves the image in the last column and row.  model_n is set on a
    checkerboard of 2 x 2 cells only (one of single pixels would be all set on the even pixels that half-even picks), so whether a pixel pairs depends on
    where its tie goes.  model_v is off the live vertices by about a pixel, inside dist_thresh = 2."""
    H, W = 5, 7
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    live_v = np.stack([u, v, np.ones_like(u)], axis=-1).astype(np.float32)
    live_n = np.zeros((H, W, 3), np.float32)
    live_n[..., 2] = -1.0
    dz = (0.0625 * ((3 * u + v) % 5)).astype(np.float32)
    model_v = np.stack([u + np.float32(0.125), v - np.float32(0.25), 1.0 + dz], axis=-1).astype(np.float32)
    cells = ((u.astype(int) // 2 + v.astype(int) // 2) % 2) == 0
    model_n = np.zeros((H, W, 3), np.float32)
    model_n[cells, 2] = -1.0
    K = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], np.float32)
    return dict(K=K, live_v=live_v, live_n=live_n, model_v=model_v, model_n=model_n, model_pose=np.eye(4), est_pose=np.eye(4), dist_thresh=2.0,
                cos_thresh=float(np.cos(np.deg2rad(20.0))))


# ---- frusta ----------------------------------------------------------------------------------------------------------------------------------------------
FRUSTUM_SIZES = [(37, 53), (513, 512)]


def frustum_case(H, W):
    """Zeros, the single maximum at the LAST pixel, a smaller positive value at pixel 0; float32 K and a camera-to-world pose."""
    depth = np.zeros((H, W), np.float32)
    depth[0, 0], depth[-1, -1] = 1.5, 4.75
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.95 * W, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    pose = np.eye(4)
    pose[:3, :3] = rotation([-0.2, 0.9, 0.4], 0.5)
    pose[:3, 3] = [0.4, -1.1, 0.6]
    return dict(depth=depth, K=K, pose=pose)


def view_frustum_formula(depth_im, cam_intr, cam_pose):
    """get_view_frustum of the reference's fusion library (call site hive/fusion.py:59), in float64 on the float32 inputs: the apex and the four image
    corners at max(depth), then the rigid transform."""
    im_h, im_w = depth_im.shape
    K = np.asarray(cam_intr, np.float64)
    max_depth = np.float64(np.max(depth_im))
    deps = np.array([0, max_depth, max_depth, max_depth, max_depth])
    pts = np.array([(np.array([0, 0, 0, im_w, im_w]) - K[0, 2]) * deps / K[0, 0], (np.array([0, 0, im_h, 0, im_h]) - K[1, 2]) * deps / K[1, 1], deps])
    xyz_h = np.hstack([pts.T, np.ones((5, 1))])
    return np.dot(np.asarray(cam_pose, np.float64), xyz_h.T)[:3]


# ---- depth hand-off --------------------------------------------------------------------------------------------------------------------------------------
QUANTIZE_SIZE = (37, 53)
QUANTIZE_PLANTED = [-0.0, 0.0004, 0.001, 9.9994, 10.0, 10.0006, 65.535, 65.5354, 66.0]


def quantize_case(H, W):
    """float32 depth over [-1, 70]: half of it k / 1000 as float32 (on the millimetre boundaries), half uniform, shuffled; the planted values at the
    front, 66.0 (saturating) once more at the last pixel; a ~20 % mask that leaves the planted pixels alone."""
    rng = np.random.default_rng(41)
    n = H * W
    on = (rng.integers(-1000, 70001, n // 2) / 1000.0).astype(np.float32)
    off = rng.uniform(-1.0, 70.0, n - n // 2).astype(np.float32)
    d = rng.permutation(np.concatenate([on, off]))
    d[:len(QUANTIZE_PLANTED)] = np.array(QUANTIZE_PLANTED, np.float32)
    d[-1] = 66.0
    mask = rng.random(n) < 0.2
    mask[:len(QUANTIZE_PLANTED)] = False
    mask[-1] = False
    return dict(depth=d.reshape(H, W), mask=mask.reshape(H, W))


def depth_quantize_formula(depth_m, depth_scale=1.0 / 1000.0, max_depth=10.0, mask=None):
    """dataset_adaptors.py:1432-1433 (x 1000, astype(np.uint16)), io.py:1032-1039 (x depth_scale in float32, > max_depth -> 0), fusion.py:121 (mask -> 0).
    astype of a float outside [0, 65535] is undefined in the reference (numpy wraps on x86, saturates on ARM); the library defines it as saturation, which is
    the np.clip here.  Inside the range the clip does nothing."""
    mm = np.clip(np.asarray(depth_m, np.float32) * np.float32(1000.0), np.float32(0.0), np.float32(65535.0)).astype(np.uint16)
    m = np.float32(depth_scale) * mm.astype(np.float32)
    m[m > np.float32(max_depth)] = 0.0
    if mask is not None:
        m[np.asarray(mask) != 0] = 0.0
    return mm, m
