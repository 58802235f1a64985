"""Restatements, in torch / numpy on the CPU, of the PoseOptimiser loop (hive/pose_optimisation.py:1256-1519) as hive_amd builds it -- projected Adam, see the
module docstring of hive_amd/pose_optimisation.py -- written afresh for the tests: the loss in two independent float64 formulations (quaternion products,
rotation matrices), the projected loop with ``torch.optim.Adam``, torch's ``ReduceLROnPlateau`` and the ``EarlyStopping`` rule for float64 and float32
parameters, the clip in the order include/hive_mi355x.h states and as the reference's literal sequential loop, and the common case of the tests."""
import numpy as np

U = 2.0 ** -53  # unit round-off of float64

DEFAULTS = dict(learning_rate=1e-2, l2_regularisation=0.5, min_loss_delta=1e-4, lr_scheduler_patience=50, early_stopping_patience=75, pose_t_reg=0.5,
                pose_r_reg=1.0, position_only=False)


# ------------------------------------------------------------------------------------------------ the common case
def hierarchical_pairs(n):
    pairs, step = [], 1
    while step < n:
        pairs += [(a, a + step) for a in range(0, n, step) if a + step < n]
        step *= 2
    return pairs


def rotate(q, v):
    """u v conj(u) for scalar-last unit quaternions q (..., 4) and vectors v (..., 3), numpy float64."""
    a, s = q[..., :3], q[..., 3:]
    return (s * s - np.sum(a * a, -1, keepdims=True)) * v + 2 * np.sum(a * v, -1, keepdims=True) * a + 2 * s * np.cross(a, v)


def make_case(n=12, seed=0, counts=(1, 63, 64, 65, 257), skip_frames=(7,), step=0.015, walk_t=0.006, walk_r=0.006, fps=30.0, pairs=None, depth_range=(2.0, 5.0), lateral=1.0, turn=1.0):
    """``n`` frames on a smooth path, ``step`` metres a frame; hierarchical pairs without the pairs of ``skip_frames``; per-pair correspondence counts cycling
    through ``counts``; exact correspondences -- world points projected into both frames, depth = camera-space z, rounded to float32 as a FeatureSet holds them --
    in shuffled row order; start poses that DRIFT from the truth: a random walk of ``walk_t`` metres and ``walk_r`` radians a frame from frame 0 (which is pinned
    and stays at the truth), so that the start trajectory's steps stay inside clip_distance / fps = 1 / 30 m (asserted).  World-to-camera poses:
    camera = u p conj(u) + t."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    s = np.arange(n, dtype=np.float64)
    angles = turn * np.stack([0.01 * s, 0.015 * np.sin(0.5 * s), 0.005 * s], axis=1)
    truth = np.hstack((Rotation.from_euler("xyz", angles).as_quat(), np.stack([step * 0.8 * s, step * 0.3 * np.sin(0.7 * s), step * 0.5 * s], axis=1)))
    fx, fy, cx, cy = 525.0, 520.0, 319.5, 239.5
    pairs = [p for p in (hierarchical_pairs(n) if pairs is None else pairs) if p[0] not in skip_frames and p[1] not in skip_frames]
    rows = []
    for number, (i, j) in enumerate(pairs):
        m = counts[number % len(counts)]
        world = np.stack([lateral * rng.uniform(-1.0, 1.0, m), lateral * rng.uniform(-0.8, 0.8, m), rng.uniform(*depth_range, m)], axis=1)
        side = []
        for f in (i, j):
            c = rotate(truth[f, :4], world) + truth[f, 4:]
            side += [fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy, c[:, 2]]
        rows.append(np.column_stack([np.full(m, i), np.full(m, j)] + side))
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(len(rows))]
    drift_t, drift_r = np.cumsum(walk_t * rng.standard_normal((n, 3)), axis=0), np.cumsum(walk_r * rng.standard_normal((n, 3)), axis=0)
    start = truth.copy()
    start[:, 4:] += drift_t - drift_t[0]
    start[:, :4] = (Rotation.from_rotvec(drift_r - drift_r[0]) * Rotation.from_quat(truth[:, :4])).as_quat()
    start = start.astype(np.float32)
    assert np.linalg.norm(np.diff(start[:, 4:].astype(np.float64), axis=0), axis=1).max() < 0.95 / fps, "the start trajectory leaves the clip distance"
    return dict(n=n, fps=fps, K=(fx, fy, cx, cy), pairs=pairs, truth=truth, start=start,
                index_i=rows[:, 0].astype(np.int64), index_j=rows[:, 1].astype(np.int64),
                points_i=rows[:, 2:4].astype(np.float32), depth_i=rows[:, 4].astype(np.float32),
                points_j=rows[:, 5:7].astype(np.float32), depth_j=rows[:, 7].astype(np.float32))


def constrained_case(seed=0):
    """The common case for the tests that run the loop to its end: EVERY frame in a pair of at least 63 correspondences (the single-correspondence pairs are
    redundant ones), and the points close to the cameras (0.6 .. 1.6 m deep, +-0.8 m wide).  Why both:
      * a frame whose rotation the correspondences do not hold -- in no pair, or in one pair of one point -- is moved by Adam's sign-like steps along the
        regulariser's radial gradient (1 - (r_a . r_b)^2 falls as |r| grows), lr a component an epoch, and drags its neighbours with it: on the common case the
        float64 loop with the smoothing terms RAISES the largest rotation error from 0.04 to 0.5 rad before it stops;
      * with the points 2 .. 5 m away a rotation and a translation nearly cancel in the residuals, and the absolute min_loss_delta = 1e-4 ends the run while the
        poses are still 0.03 .. 0.6 mm off, depending on the epoch the learning rate happens to fall at: 30 to 700 times better than the start, on either side
        of the hundredfold the optimisation test asks of the restatement.  Close points separate the two: 2 000 to 100 000 times better over three seeds and
        both parameter dtypes."""
    return make_case(seed=seed, skip_frames=(), counts=(63, 64, 65, 257, 1), depth_range=(0.6, 1.6), lateral=0.8)


def camera_matrix(case):
    fx, fy, cx, cy = case["K"]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def pose_errors(params, truth):
    """(position RMSE, largest rotation angle) of ``params`` (N, 7) against the true poses."""
    from scipy.spatial.transform import Rotation
    rmse = float(np.sqrt(np.mean(np.sum((params[:, 4:7] - truth[:, 4:]) ** 2, axis=1))))
    q = params[:, :4] / np.linalg.norm(params[:, :4], axis=1, keepdims=True)
    angle = float(np.max((Rotation.from_quat(q) * Rotation.from_quat(truth[:, :4]).inv()).magnitude()))
    return rmse, angle


# ------------------------------------------------------------------------------------------------ the loss, twice
def _hamilton(a, b):
    import torch
    ax, ay, az, aw = a.unbind(1)
    bx, by, bz, bw = b.unbind(1)
    return torch.stack((aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                        aw * bw - ax * bx - ay * by - az * bz), dim=1)


def _apply_quaternion(q, v, inverse):
    """u v conj(u) (or conj(u) v u) with u = q / |q|: quaternion products."""
    import torch
    u = q / torch.linalg.norm(q, ord=2, dim=1, keepdim=True)
    conj = u * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=u.dtype, device=u.device)
    pure = torch.cat((v, torch.zeros((v.shape[0], 1), dtype=v.dtype, device=v.device)), dim=1)
    first, second = (conj, u) if inverse else (u, conj)
    return _hamilton(_hamilton(first, pure), second)[:, :3]


def _apply_matrix(q, v, inverse):
    """The same through rotation matrices."""
    import torch
    x, y, z, w = (q / torch.linalg.norm(q, ord=2, dim=1, keepdim=True)).unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)
    return torch.einsum("nji,nj->ni" if inverse else "nij,nj->ni", R, v)


def _mean_or_zero(x):
    """A mean over nothing (fewer than four frames) is 0 here, as the kernel states; torch.mean gives NaN."""
    import torch
    return torch.mean(x) if x.numel() else torch.zeros((), dtype=x.dtype, device=x.device)


def world_points(q, t, scale, shift, data, side, affine=False, apply=_apply_quaternion):
    """conj(u) (c - t) u for the correspondences' ``side`` ('i' or 'j'), c the unprojected pixel; the parameters' dtype is the dtype of the arithmetic."""
    import torch
    fx, fy, cx, cy = data["K"]
    index, depth = data["index_" + side], data["depth_" + side].to(q.dtype)
    if affine:
        depth = 1.0 / (scale[index] * (1.0 / depth) + shift[index])
    u, v = data["points_" + side].to(q.dtype).unbind(1)
    camera = torch.stack(((u - cx) * depth / fx, (v - cy) * depth / fy, depth), dim=1)
    return apply(q[index], camera - t[index], True)


def project(q, t, data, p, apply=_apply_quaternion):
    """The pixel of the world points ``p`` in the correspondences' frame j."""
    import torch
    fx, fy, cx, cy = data["K"]
    j = data["index_j"]
    x, y, z = (apply(q[j], p, False) + t[j]).unbind(1)
    return torch.stack(((fx * x + cx * z) / z, (fy * y + cy * z) / z), dim=1)


def residuals(q, t, scale, shift, data, residual_type="World3D", affine=False, apply=_apply_quaternion):
    """(M, 3) or (M, 2) residuals.  ``data``: the correspondence tensors (``tensors_of``)."""
    p = world_points(q, t, scale, shift, data, "i", affine, apply)
    if residual_type == "World3D":
        return p - world_points(q, t, scale, shift, data, "j", affine, apply)
    return data["points_j"].to(q.dtype) - project(q, t, data, p, apply)


def loss(q, t, scale, shift, data, residual_type="World3D", affine=False, smooth=True, options=DEFAULTS, apply=_apply_quaternion):
    import torch
    value = torch.mean(torch.linalg.norm(residuals(q, t, scale, shift, data, residual_type, affine, apply), ord=2, dim=1))
    if smooth:
        d1 = t[:-1] - t[1:]
        d2 = t[:-2] - 2 * t[1:-1] + t[2:]
        d3 = d2[:-1] - d2[1:]
        for d in (d1, d2, d3):
            value = value + options["pose_t_reg"] * _mean_or_zero(torch.sum(torch.square(d), dim=1))
        value = value + options["pose_r_reg"] * _mean_or_zero(1 - torch.square(torch.einsum("ij,ij->i", q[:-1], q[1:])))
    if affine:
        l2 = options["l2_regularisation"]
        value = value + l2 * torch.mean(torch.square(1.0 / scale - 1.0)) + 2 * l2 * torch.mean(torch.square(shift))
    return value


def tensors_of(case):
    import torch
    out = {k: torch.from_numpy(np.ascontiguousarray(case[k])) for k in ("index_i", "index_j", "points_i", "points_j", "depth_i", "depth_j")}
    out["K"] = case["K"]
    return out


def pin(grad_q, grad_t, position_only):
    """Frame 0 is pinned; with ``position_only`` every rotation."""
    grad_t[0] = 0.0
    if position_only:
        grad_q[:] = 0.0
    else:
        grad_q[0] = 0.0


def loss_and_gradient(params, scale, shift, case, residual_type="World3D", affine=False, smooth=True, options=DEFAULTS, apply=_apply_quaternion):
    """float64 loss at ``params`` (N, 7) (no projection applied) and its gradient (N, 9) = d/d(q, t, scale, shift) with the pins applied, by autograd."""
    import torch
    p = np.asarray(params, np.float64)
    q, t = torch.tensor(p[:, :4], requires_grad=True), torch.tensor(p[:, 4:7], requires_grad=True)
    sc, sh = torch.tensor(np.asarray(scale, np.float64), requires_grad=True), torch.tensor(np.asarray(shift, np.float64), requires_grad=True)
    value = loss(q, t, sc, sh, tensors_of(case), residual_type, affine, smooth, options, apply)
    value.backward()
    pin(q.grad, t.grad, options["position_only"])
    zero = torch.zeros(len(p), dtype=torch.float64)
    grad = torch.cat((q.grad, t.grad, (sc.grad if sc.grad is not None else zero)[:, None], (sh.grad if sh.grad is not None else zero)[:, None]), dim=1)
    return float(value.detach()), grad.numpy().copy()


def conditioning(params, scale, shift, case, residual_type="World3D", affine=False):
    """kappa = max_k (|a_k| + |b_k|) / |a_k - b_k| over the correspondences, a - b the residual's final subtraction (the two world points, or the pixel and the
    projection): what the direction of a residual loses in ANY float64 evaluation."""
    import torch
    p = torch.tensor(np.asarray(params, np.float64))
    data = tensors_of(case)
    q, t, sc, sh = p[:, :4], p[:, 4:7], torch.tensor(np.asarray(scale, np.float64)), torch.tensor(np.asarray(shift, np.float64))
    a = world_points(q, t, sc, sh, data, "i", affine)
    if residual_type == "World3D":
        b = world_points(q, t, sc, sh, data, "j", affine)
    else:
        a, b = data["points_j"].double(), project(q, t, data, a)
    return float(torch.max((torch.linalg.norm(a, dim=1) + torch.linalg.norm(b, dim=1)) / torch.linalg.norm(a - b, dim=1)))


# ------------------------------------------------------------------------------------------------ the projection
def normalise_rows(q):
    """q / sqrt(((x^2 + y^2) + z^2) + w^2), numpy in the array's dtype: the stated order."""
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return q / n[:, None]


def clip_stated(t, max_frame_distance):
    """The clip in the stated order: d_i = t_i - t_{i-1} of the INPUT; |d_i| = sqrt((dx^2 + dy^2) + dz^2); where |d_i| > max, d_i becomes (max / |d_i|) d_i;
    frames before the first such i are untouched, from it on t'_i = t'_{i-1} + d_i, one frame after the other."""
    t = np.array(t, copy=True)
    d = t[1:] - t[:-1]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    over = dist > max_frame_distance
    if not over.any():
        return t
    s = np.asarray(max_frame_distance, t.dtype) / dist[over]
    d[over] = s[:, None] * d[over]
    first = int(np.argmax(over)) + 1
    for i in range(first, len(t)):
        t[i] = t[i - 1] + d[i - 1]
    return t


def clip_literal(t, max_frame_distance):
    """The reference's loop as it stands (:1353-1378): clip a frame, then shift every later frame by the correction."""
    p = np.array(t, copy=True)
    for i in range(1, len(p)):
        current = p[i].copy()
        diff = current - p[i - 1]
        distance = np.linalg.norm(diff)
        if distance > max_frame_distance:
            p[i] = p[i - 1] + max_frame_distance * (diff / distance)
            if i + 1 < len(p):
                p[i + 1:] += p[i] - current
    return p


# ------------------------------------------------------------------------------------------------ scheduler and stop
class EarlyStopping:
    def __init__(self, patience, min_difference):
        self.patience, self.min_difference, self.best, self.calls, self.should_stop = patience, min_difference, float("inf"), 0, False

    def step(self, value):
        if value < self.best and abs(value - self.best) > self.min_difference:
            self.best, self.calls = value, 0
        else:
            self.calls += 1
        if self.calls > self.patience:
            self.should_stop = True
        return self.should_stop


def replay(losses, options=DEFAULTS):
    """torch's ReduceLROnPlateau and the EarlyStopping rule fed with ``losses``: (learning rate after each loss, the number of epochs run)."""
    import torch
    dummy = torch.nn.Parameter(torch.zeros(1))
    optimiser = torch.optim.Adam([dummy], lr=options["learning_rate"])
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimiser, patience=options["lr_scheduler_patience"], mode="min",
                                                           threshold=options["min_loss_delta"], threshold_mode="abs")
    stop = EarlyStopping(options["early_stopping_patience"], options["min_loss_delta"])
    rates = []
    for value in losses:
        scheduler.step(float(value))
        stop.step(float(value))
        rates.append(optimiser.param_groups[0]["lr"])
        if stop.should_stop:
            break
    return np.array(rates), len(rates)


# ------------------------------------------------------------------------------------------------ the whole run
def run(case, num_epochs, residual_type="World3D", affine=False, smooth=True, options=DEFAULTS, dtype="float64", max_frame_distance=None, start=None):
    """The projected loop: every epoch normalises the quaternions and clips the positions IN PLACE, then Adam steps the same parameters; torch's scheduler and
    the stop rule see every loss.  Returns (raw parameters (N, 9) float64, losses, learning rates, epochs run)."""
    import torch
    dt = {"float64": torch.float64, "float32": torch.float32}[dtype]
    first = torch.tensor(np.asarray(case["start"] if start is None else start, np.float32))
    q, t = torch.nn.Parameter(first[:, :4].clone().to(dt)), torch.nn.Parameter(first[:, 4:].clone().to(dt))
    scale, shift = torch.nn.Parameter(torch.ones(len(first), dtype=dt)), torch.nn.Parameter(torch.zeros(len(first), dtype=dt))
    optimiser = torch.optim.Adam([q, t] + ([scale, shift] if affine else []), lr=options["learning_rate"])
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimiser, patience=options["lr_scheduler_patience"], mode="min",
                                                           threshold=options["min_loss_delta"], threshold_mode="abs")
    stop = EarlyStopping(options["early_stopping_patience"], options["min_loss_delta"])
    data = tensors_of(case)
    losses, rates = [], []
    for _ in range(num_epochs):
        with torch.no_grad():
            q.copy_(torch.from_numpy(normalise_rows(q.numpy())))
            if max_frame_distance is not None:
                t.copy_(torch.from_numpy(clip_stated(t.numpy(), max_frame_distance)))
        optimiser.zero_grad()
        value = loss(q, t, scale, shift, data, residual_type, affine, smooth, options)
        value.backward()
        pin(q.grad, t.grad, options["position_only"])
        optimiser.step()
        scheduler.step(float(value.detach()))
        stop.step(float(value.detach()))
        losses.append(float(value.detach()))
        rates.append(optimiser.param_groups[0]["lr"])
        if stop.should_stop:
            break
    out = torch.cat((q, t, scale[:, None], shift[:, None]), dim=1).detach().numpy().astype(np.float64)
    return out, np.array(losses), np.array(rates), len(losses)


# ------------------------------------------------------------------------------------------------ what the GPU tests' bounds are made of
def _apply_as_given(q, v, inverse):
    """q v conj(q) (or conj(q) v q) WITHOUT the normalisation: its gradient is d/du of the unit quaternion, before the projection onto the tangent space."""
    import torch
    conj = q * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=q.dtype, device=q.device)
    pure = torch.cat((v, torch.zeros((v.shape[0], 1), dtype=v.dtype, device=v.device)), dim=1)
    first, second = (conj, q) if inverse else (q, conj)
    return _hamilton(_hamilton(first, pure), second)[:, :3]


def gradient_term_magnitudes(params, scale, shift, case, residual_type="World3D", affine=False, smooth=True, options=DEFAULTS):
    """S (N, 9): the magnitude a rounding error of the gradient is relative to.  For the translation, scale and shift components sum_k |d(|r_k| / M) / dtheta|
    (autograd's per-correspondence Jacobian) + |d(regularisers) / dtheta|.  A quaternion component is (G_j - u_j (u . G)) / |q| with G = d/du of the UNIT
    quaternion, a difference that cancels where u is close to a coordinate axis, so its error is relative to the parts, not to the result:
    sum_k (|G_kj| + |u_j| sum_i |u_i| |G_ki|) / |q|."""
    import torch
    p = np.asarray(params, np.float64)
    data = tensors_of(case)
    m, index = len(case["index_i"]), np.concatenate([case["index_i"], case["index_j"]])
    own = dict(data, index_i=torch.arange(m), index_j=m + torch.arange(m))

    def per_correspondence(quaternions, apply):
        # every correspondence gets its own copy of its two frames' parameters: one backward pass then gives the per-correspondence Jacobian
        rows = torch.tensor(np.hstack((quaternions[index], p[index, 4:7], np.asarray(scale, np.float64)[index, None], np.asarray(shift, np.float64)[index, None])),
                            requires_grad=True)
        r = residuals(rows[:, :4], rows[:, 4:7], rows[:, 7], rows[:, 8], own, residual_type, affine, apply)
        (torch.linalg.norm(r, ord=2, dim=1) / m).sum().backward()
        return rows.grad.abs().numpy()

    total = np.zeros((len(p), 9))
    np.add.at(total, index, per_correspondence(p[:, :4], _apply_quaternion))
    norm = np.linalg.norm(p[:, :4], axis=1, keepdims=True)
    unit = np.abs(p[:, :4] / norm)
    parts = per_correspondence(p[:, :4] / norm, _apply_as_given)[:, :4]
    parts = (parts + unit[index] * np.sum(unit[index] * parts, axis=1, keepdims=True)) / norm[index]
    unprojected = np.zeros((len(p), 4))
    np.add.at(unprojected, index, parts)
    total[:, :4] = np.maximum(total[:, :4], unprojected)
    with_reg = loss_and_gradient(p, scale, shift, case, residual_type, affine, smooth, options)[1]
    main_only = loss_and_gradient(p, scale, shift, case, residual_type, affine, False, dict(options, l2_regularisation=0.0))[1]
    pinned = (with_reg == 0.0) & (main_only == 0.0)
    return np.where(pinned, 0.0, total + np.abs(with_reg - main_only))


def clip_trajectory(n, limit, seed=0):
    """Poses for the projection tests: raw quaternions of any length, and positions on a 2^-20 grid (so that the differences are exact) whose steps are below the
    limit, exactly AT it (an axis-aligned step of ``limit``: not clipped), above it, and, from 70 frames on, a run of five consecutive violations.  Returns
    (poses (n, 7) float64, the kinds of step present)."""
    rng = np.random.default_rng(seed + n)
    kinds = []
    for f in range(1, n):
        if n == 2 or (n == 3 and f == 2):
            kinds.append("above")
        elif n == 3:
            kinds.append("at")
        elif n // 2 <= f < n // 2 + 5 or f % 10 == 6:
            kinds.append("above")
        else:
            kinds.append("at" if f % 10 == 3 else "below")
    t = np.zeros((n, 3))
    t[0] = [0.5, -0.25, 1.0]
    for f, kind in enumerate(kinds, start=1):
        direction = rng.standard_normal(3)
        direction /= np.linalg.norm(direction)
        length = {"below": rng.uniform(0.2, 0.95), "above": rng.uniform(1.2, 3.0), "at": 1.0}[kind] * limit
        t[f] = t[f - 1] + (np.array([limit, 0.0, 0.0]) if kind == "at" else np.round(length * direction * 2 ** 20) / 2 ** 20)
    q = rng.standard_normal((n, 4)) * rng.uniform(0.1, 10.0, (n, 1))
    return np.hstack((q, t)), sorted(set(kinds))
