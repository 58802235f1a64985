"""Restatements, in numpy / torch on the CPU, of the two foreground stages behind ``--billboard`` and ``--fts_num_epochs`` (hive/pipeline.py:439-447,
hive/pose_optimisation.py:1618-1711), written afresh for the tests: the billboard map in the library's stated operation order and in the reference's literal
matrix form, the chunking rule, the smoothing loss in two independent float64 formulations (quaternion products, rotation matrices) and the whole Adam loop with
``torch.optim.Adam`` -- with float64 parameters (the yardstick) and with the reference's float32 parameters."""
import numpy as np

U = 2.0 ** -53  # unit round-off of float64


# ------------------------------------------------------------------------------------------------ billboard
def camera_z_ordered(vertices, R, t):
    """Third row of R (p + t) in the library's order, element-wise numpy operations (which never fuse a multiply with an add)."""
    x, y, z = (vertices[:, k] + t[k] for k in range(3))
    return (R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z


def billboard_ordered(vertices, R, t):
    """The billboard map in the operation order include/hive_mi355x.h states; returns (flattened vertices, median depth)."""
    vertices = np.asarray(vertices, np.float64)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    x, y, z = (vertices[:, k] + t[k] for k in range(3))
    c0 = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) - t[0]
    c1 = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) - t[1]
    m = np.median((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z)
    c2 = m - t[2]
    out = np.stack([(R[0, j] * c0 + R[1, j] * c1) + R[2, j] * c2 for j in range(3)], axis=1)
    return out, m


def billboard_literal(vertices, R, t):
    """The three lines of the reference as they stand (matrix products: BLAS may fuse and reorder the dot products)."""
    vertices = np.asarray(vertices, np.float64)
    rotation, translation = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)
    camera_space_points = rotation @ (vertices.T + translation)
    camera_space_points[2, :] = np.median(camera_space_points[2, :])
    return (rotation.T @ (camera_space_points - translation)).T


def literal_bound(vertices, t):
    """16 u M, M = max_i |p_i + t| + |t|: what the literal form may differ by from any other evaluation order (see tests/test_billboard_gpu.py)."""
    t = np.asarray(t, np.float64).reshape(3)
    return 16 * U * (np.linalg.norm(np.asarray(vertices, np.float64) + t, axis=1).max() + np.linalg.norm(t))


# ------------------------------------------------------------------------------------------------ centroids
CENTROID_SIZES = ((5, 7), (64, 65), (130, 97))  # less than a wave; a full tile and a tile of 64 pixels; four tiles: the frame's butterfly has live lanes


def _block_sum(s):
    """s (..., 256, k), one row a thread -> (..., k), what thread 0 holds: in every wave the butterfly s = s + s[lane ^ off], off = 32 .. 1, then the four waves
    left to right.  numpy adds element-wise and never contracts."""
    s = s.reshape(s.shape[:-2] + (4, 64, s.shape[-1]))
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ off, :]
    w = s[..., 0, :]
    return ((w[..., 0, :] + w[..., 1, :]) + w[..., 2, :]) + w[..., 3, :]


def centroids_ordered(depth, masks, K_inv):
    """``hive_fg_centroids`` in the order include/hive_mi355x.h states, numpy float64: tiles of 4096 pixels, thread t of a tile adds its 16 pixels
    tile + j * 256 + t with j ascending, the block sum, then the tiles likewise (thread k takes tiles k, k + 256, ..), one division.  Returns (centroids float64
    (n, 3), counts int64 (n,)); ``np.sum`` over the same terms as the second pair, for the test that the order matters."""
    depth, K_inv = np.asarray(depth, np.float32), np.asarray(K_inv, np.float64).reshape(3, 3)
    n, h, w = depth.shape
    tiles = -(-h * w // 4096)
    i = np.arange(tiles * 4096)
    pu, pv = (i % w).astype(np.float64), (i // w).astype(np.float64)
    rays = [(K_inv[r, 0] * pu + K_inv[r, 1] * pv) + K_inv[r, 2] for r in range(3)]
    out, counts, plain = np.zeros((n, 3)), np.zeros(n, np.int64), np.zeros((n, 3))
    for f in range(n):
        z = np.zeros(tiles * 4096)
        z[:h * w] = depth[f].reshape(-1).astype(np.float64)
        valid = np.zeros(tiles * 4096, bool)
        valid[:h * w] = (np.asarray(masks[f]).reshape(-1) != 0) & (depth[f].reshape(-1) > 0)
        terms = np.stack([np.where(valid, z * ray, 0.0) for ray in rays] + [valid.astype(np.float64)], axis=1).reshape(tiles, 16, 256, 4)
        s = np.zeros((tiles, 256, 4))
        for j in range(16):
            s = s + terms[:, j]
        partial = _block_sum(s)  # (tiles, 4)
        s = np.zeros((256, 4))
        for t in range(tiles):
            s[t % 256] = s[t % 256] + partial[t]
        total = _block_sum(s)
        counts[f] = int(total[3])
        if total[3] > 0:
            out[f] = total[:3] / total[3]
            plain[f] = np.sum(terms.reshape(-1, 4)[:, :3], axis=0) / total[3]
    return out, counts, plain


def centroid_order_case(size, seed=4):
    """A batch of three H x W frames whose depths are drawn over 2^-6 .. 2^6, so that the order of the additions shows in the last bits; 70 % of the pixels
    masked in, some without depth, the middle frame's mask empty.  Returns (depth float32, masks uint8, K float64)."""
    h, w = size
    rng = np.random.default_rng(seed + 1000 * h + w)
    depth = (2.0 ** rng.uniform(-6.0, 6.0, (3, h, w))).astype(np.float32)
    depth[rng.random((3, h, w)) < 0.05] = 0.0
    masks = (rng.random((3, h, w)) < 0.7).astype(np.uint8) * rng.integers(1, 4, (3, h, w), dtype=np.uint8)
    masks[1] = 0
    return depth, masks, np.array([[525.0, 0.0, 0.5 * w - 0.5], [0.0, 520.0, 0.5 * h - 0.5], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------------------------------------ chunks
def chunks_of(counts, min_chunk_size=3):
    """Runs of consecutive frames with points, at least ``min_chunk_size`` long, as lists of frame indices (the form the reference keeps them in)."""
    out, run = [], []
    for i, c in enumerate(counts):
        if c > 0:
            run.append(i)
            continue
        if len(run) >= min_chunk_size:
            out.append(run)
        run = []
    if len(run) >= min_chunk_size:
        out.append(run)
    return out


# ------------------------------------------------------------------------------------------------ loss
def _hamilton(a, b):
    """Hamilton product of (N, 4) scalar-last quaternions."""
    import torch
    ax, ay, az, aw = a.unbind(1)
    bx, by, bz, bw = b.unbind(1)
    return torch.stack((aw * bx + ax * bw + ay * bz - az * by,
                        aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx,
                        aw * bw - ax * bx - ay * by - az * bz), dim=1)


def world_centroids(q, t, c):
    """conj(q / |q|) (c - t, 0) (q / |q|), vector part: quaternion products, the reference's formulation.  q (N, 4), t (N, 3) of one dtype (float32 or float64), c (N, 3)
    float64: the normalisation happens in the parameters' dtype, everything after the subtraction in float64, as torch's promotion makes it in the reference."""
    import torch
    n = q / torch.linalg.norm(q, ord=2, dim=1, keepdim=True)
    conj = n * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=n.dtype)
    v = c - t
    pure = torch.cat((v, torch.zeros((v.shape[0], 1), dtype=v.dtype)), dim=1)
    return _hamilton(_hamilton(conj, pure), n)[:, :3]


def world_centroids_matrix(q, t, c):
    """The same through rotation matrices: R(q / |q|)^T (c - t) -- an independent formulation for the CPU cross-check."""
    import torch
    n = q / torch.linalg.norm(q, ord=2, dim=1, keepdim=True)
    x, y, z, w = n.unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)
    return torch.einsum("nji,nj->ni", R.to(c.dtype), c - t)


def loss(q, t, c, gt, chunks, world=world_centroids, start=None):
    """The loss of one epoch; ``chunks`` lists of frame indices; ``start``: the tensor the terms are added to in place (the reference starts from a float32 zero)."""
    import torch
    total = torch.zeros((), dtype=torch.float64) if start is None else start
    for chunk in chunks:
        tc = t[chunk]
        geom = torch.mean(torch.norm(gt[chunk] - world(q[chunk], tc, c[chunk]), dim=1))
        temp = torch.norm(tc[:-2] - 2 * tc[1:-1] + tc[2:])
        vel = torch.norm(tc[:-1] - tc[1:])
        total = total + (0.01 * geom + 0.1 * temp + 0.1 * vel)
    return total


def loss_and_gradient(params, gt_params, centroids, chunks, world=world_centroids):
    """float64 loss at ``params`` (N, 7) with gt taken at ``gt_params``, and its gradient (N, 7), by autograd; also gt and the world-space centroids at ``params``."""
    import torch
    p = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    g = torch.tensor(np.asarray(gt_params, np.float64))
    c = torch.tensor(np.asarray(centroids, np.float64))
    with torch.no_grad():
        gt = world(g[:, :4], g[:, 4:], c)
    value = loss(p[:, :4], p[:, 4:], c, gt, chunks, world)
    if value.requires_grad:
        value.backward()
    grad = np.zeros(p.shape) if p.grad is None else p.grad.numpy().copy()
    with torch.no_grad():
        w = world(p[:, :4], p[:, 4:], c)
    return float(value.detach()), grad, gt.numpy(), w.numpy()


def conditioning(gt, w, chunks):
    """kappa = max_i (|gt_i| + |w_i|) / |gt_i - w_i| over the frames of the chunks: what the direction of the residual loses in ANY float64 evaluation."""
    idx = [i for chunk in chunks for i in chunk]
    r = np.linalg.norm(gt[idx] - w[idx], axis=1)
    return float(np.max((np.linalg.norm(gt[idx], axis=1) + np.linalg.norm(w[idx], axis=1)) / r))


# ------------------------------------------------------------------------------------------------ the whole run
def run(trajectory32, centroids, chunks, learning_rate=1e-5, num_epochs=100, dtype="float64"):
    """The Adam loop with ``torch.optim.Adam(lr, weight_decay=1e-4)``.  ``trajectory32`` (N, 7) float32 start values; parameters of ``dtype``: 'float64' (the yardstick)
    or 'float32' (what the reference does).  Returns (raw parameters (N, 7) float64, the loss before every step and after the last one)."""
    import torch
    dt = {"float64": torch.float64, "float32": torch.float32}[dtype]
    start = torch.tensor(np.asarray(trajectory32, np.float32))
    q = torch.nn.Parameter(start[:, :4].clone().to(dt))
    t = torch.nn.Parameter(start[:, 4:].clone().to(dt))
    c = torch.tensor(np.asarray(centroids, np.float64))
    optimiser = torch.optim.Adam([q, t], lr=learning_rate, weight_decay=1e-4)
    with torch.no_grad():
        gt = world_centroids(q, t, c)
    first = (lambda: torch.tensor(0.0)) if dtype == "float32" else (lambda: None)
    losses = []
    for _ in range(num_epochs):
        optimiser.zero_grad()
        value = loss(q, t, c, gt, chunks, start=first())
        if value.requires_grad:  # (without a chunk the loss is a constant: only the decay acts)
            value.backward()
        else:
            q.grad, t.grad = torch.zeros_like(q), torch.zeros_like(t)
        optimiser.step()
        losses.append(float(value.detach()))
    with torch.no_grad():
        losses.append(float(loss(q, t, c, gt, chunks)))
    return np.hstack((q.detach().numpy().astype(np.float64), t.detach().numpy().astype(np.float64))), np.array(losses)


def jittery_case(num_frames=60, seed=0, empty=(20, 21, 22, 25, 45)):
    """A synthetic sequence for the whole-run tests: a smooth camera path with jitter on the rotations and positions, object centroids a few metres in front of the
    camera, and point counts that are 0 on ``empty`` (with the default: three chunks, a run of two that is dropped and five frames that belong to none).  Returns
    (float32 trajectory (N, 7), centroids float64 (N, 3), counts (N,))."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, num_frames)
    angles = np.stack([0.3 * s, 0.2 * np.sin(2 * s), 0.1 * s], axis=1) + 0.01 * rng.standard_normal((num_frames, 3))
    quats = Rotation.from_euler("xyz", angles).as_quat()
    positions = np.stack([0.5 * s, 0.1 * np.sin(3 * s), 0.3 * s * s], axis=1) + 0.005 * rng.standard_normal((num_frames, 3))
    centroids = np.stack([0.4 * np.cos(4 * s), 0.3 * np.sin(5 * s), 2.5 + 0.5 * s], axis=1) + 0.02 * rng.standard_normal((num_frames, 3))
    counts = np.full(num_frames, 1000, np.int64)
    counts[list(empty)] = 0
    centroids[list(empty)] = 0.0
    return np.hstack((quats, positions)).astype(np.float32), centroids, counts
