"""The tracker's rules (include/hive_mi355x.h, above hive_frame_maps and hive_icp_step) in numpy, literally: what csrc/track.hip must reproduce -- the pyramid
and the maps bit for bit in float32, the ICP terms in float64 per pixel, the sums in the kernel's order.  Then ``icp_align`` and the track-and-fuse loop of
hive_amd/tracking.py restated on the host over an oracle volume and the ray-cast restatement."""
import numpy as np

import raycast_restatement as rc
import tracking_cases as tc

f32 = np.float32
HALF_EVEN, HALF_AWAY = 0, 1
BLOCK = 256


# ---- hive_frame_maps ----------------------------------------------------------------------------------------------------------------------------------
def pyr_down(depth, delta):
    d = np.asarray(depth, f32)
    H, W = d.shape[0] // 2, d.shape[1] // 2
    s = [d[0:2 * H:2, 0:2 * W:2], d[0:2 * H:2, 1:2 * W:2], d[1:2 * H:2, 0:2 * W:2], d[1:2 * H:2, 1:2 * W:2]]  # row-major order of the block
    valid = [x > f32(0) for x in s]
    m = np.full((H, W), f32(np.inf), f32)
    for x, ok in zip(s, valid):
        m = np.where(ok & (x < m), x, m)
    total, count = np.zeros((H, W), f32), np.zeros((H, W), f32)
    with np.errstate(invalid="ignore"):
        for x, ok in zip(s, valid):
            take = ok & (x - m <= f32(delta))
            total = np.where(take, total + x, total)
            count = np.where(take, count + f32(1), count)
    return np.where(count > 0, total / np.where(count > 0, count, f32(1)), f32(0)).astype(f32)


def level_intrinsics(K, levels):
    K = np.asarray(K, f32).reshape(3, 3)
    fx, fy, cx, cy = (np.float64(K[0, 0]), np.float64(K[1, 1]), np.float64(K[0, 2]), np.float64(K[1, 2]))
    out = []
    for l in range(levels):
        if l > 0:
            fx, fy, cx, cy = fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0
        out.append(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64).astype(f32))
    return np.stack(out)


def vertex_normal(depth, K):
    d = np.asarray(depth, f32)
    H, W = d.shape
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    u, v = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    V = np.stack([(d * (u - cx)) / fx, (d * (v - cy)) / fy, d], axis=-1).astype(f32)
    N = np.zeros((H, W, 3), f32)
    if H > 1 and W > 1:
        P, A, B = V[:-1, :-1], V[:-1, 1:] - V[:-1, :-1], V[1:, :-1] - V[:-1, :-1]
        ok = (d[:-1, :-1] > 0) & (d[:-1, 1:] > 0) & (d[1:, :-1] > 0)
        x = A[..., 1] * B[..., 2] - A[..., 2] * B[..., 1]
        y = A[..., 2] * B[..., 0] - A[..., 0] * B[..., 2]
        z = A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]
        with np.errstate(all="ignore"):
            length = np.sqrt((x * x + y * y) + z * z)
            ok &= (length > 0) & (length < f32(np.inf))
            n = np.stack([x, y, z], axis=-1) / np.where(ok, length, f32(1))[..., None]
            dot = (n[..., 0] * P[..., 0] + n[..., 1] * P[..., 1]) + n[..., 2] * P[..., 2]
        n = np.where((dot > 0)[..., None], -n, n)
        N[:-1, :-1] = np.where(ok[..., None], n, f32(0))
    V = np.where((d > 0)[..., None], V, f32(0)).astype(f32)
    return V, N


def frame_maps(depth, K, levels=3, delta=0.05):
    """-> per level lists (depth, vertex, normal) and K float32 (levels, 3, 3)."""
    Ks = level_intrinsics(K, levels)
    depths, Vs, Ns = [np.asarray(depth, f32)], [], []
    for l in range(1, levels):
        depths.append(pyr_down(depths[-1], delta))
    for l in range(levels):
        V, N = vertex_normal(depths[l], Ks[l])
        Vs.append(V), Ns.append(N)
    return depths, Vs, Ns, Ks


# ---- hive_icp_step ------------------------------------------------------------------------------------------------------------------------------------
def invert_pose(pose):
    """[R^T | -((R^T[r][0] t_0 + R^T[r][1] t_1) + R^T[r][2] t_2)]"""
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    Rt, t = pose[:3, :3].T.copy(), pose[:3, 3]
    return Rt, np.array([-((Rt[r, 0] * t[0] + Rt[r, 1] * t[1]) + Rt[r, 2] * t[2]) for r in range(3)])


def _round(x, mode):
    return np.rint(x) if mode == HALF_EVEN else np.copysign(np.floor(np.abs(x) + 0.5), x)


def icp_terms(K, live_v, live_n, model_v, model_n, model_pose, est_pose, dist_thresh, cos_thresh, round_mode=HALF_EVEN):
    """-> terms float64 (H W, 29) (28 sums' terms and the pair flag) and the pair mask bool (H, W)."""
    H, W = live_v.shape[:2]
    K = np.asarray(K, f32).reshape(3, 3).astype(np.float64)
    est = np.asarray(est_pose, np.float64).reshape(4, 4)
    R, t = est[:3, :3], est[:3, 3]
    Mi, Mt = invert_pose(model_pose)
    V, N = live_v.reshape(-1, 3).astype(np.float64), live_n.reshape(-1, 3).astype(np.float64)
    mv, mn = model_v.reshape(-1, 3).astype(np.float64), model_n.reshape(-1, 3).astype(np.float64)
    keep = (N[:, 0] != 0) | (N[:, 1] != 0) | (N[:, 2] != 0)
    q = [((R[r, 0] * V[:, 0] + R[r, 1] * V[:, 1]) + R[r, 2] * V[:, 2]) + t[r] for r in range(3)]
    n = [(R[r, 0] * N[:, 0] + R[r, 1] * N[:, 1]) + R[r, 2] * N[:, 2] for r in range(3)]
    c = [((Mi[r, 0] * q[0] + Mi[r, 1] * q[1]) + Mi[r, 2] * q[2]) + Mt[r] for r in range(3)]
    keep &= c[2] > 0
    with np.errstate(all="ignore"):
        pu = _round(K[0, 0] * (c[0] / c[2]) + K[0, 2], round_mode)
        pv = _round(K[1, 1] * (c[1] / c[2]) + K[1, 2], round_mode)
        keep &= (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    at = np.where(keep, pv, 0).astype(np.int64) * W + np.where(keep, pu, 0).astype(np.int64)
    Nm, Vm = mn[at], mv[at]
    keep &= (Nm[:, 0] != 0) | (Nm[:, 1] != 0) | (Nm[:, 2] != 0)
    d = [Vm[:, r] - q[r] for r in range(3)]
    dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    cosine = (n[0] * Nm[:, 0] + n[1] * Nm[:, 1]) + n[2] * Nm[:, 2]
    keep &= (dist <= np.float64(f32(dist_thresh))) & (cosine >= np.float64(f32(cos_thresh)))
    r = (Nm[:, 0] * d[0] + Nm[:, 1] * d[1]) + Nm[:, 2] * d[2]
    J = [q[1] * Nm[:, 2] - q[2] * Nm[:, 1], q[2] * Nm[:, 0] - q[0] * Nm[:, 2], q[0] * Nm[:, 1] - q[1] * Nm[:, 0], Nm[:, 0], Nm[:, 1], Nm[:, 2]]
    cols = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r, np.ones_like(r)]
    terms = np.where(keep[:, None], np.stack(cols, axis=1), 0.0)
    return terms, keep.reshape(H, W)


def icp_sums(terms):
    """The kernel's order: workgroups of 256 consecutive pixels, the tree x[t] += x[t + off] for off = 128 .. 1, then the workgroups in ascending order."""
    n = terms.shape[0]
    rows = -(-n // BLOCK)
    x = np.zeros((rows * BLOCK, terms.shape[1]), np.float64)
    x[:n] = terms
    x = x.reshape(rows, BLOCK, -1)
    off = BLOCK // 2
    while off > 0:
        x[:, :off] = x[:, :off] + x[:, off:2 * off]
        off //= 2
    acc = np.zeros(terms.shape[1], np.float64)
    for b in range(rows):
        acc = acc + x[b, 0]
    return acc[:28], int(acc[28])


def icp_step(K, live_v, live_n, model_v, model_n, model_pose, est_pose, dist_thresh, cos_thresh, round_mode=HALF_EVEN):
    terms, mask = icp_terms(K, live_v, live_n, model_v, model_n, model_pose, est_pose, dist_thresh, cos_thresh, round_mode)
    sums, pairs = icp_sums(terms)
    return sums, pairs, mask


# ---- hive_amd/tracking.py on the host -----------------------------------------------------------------------------------------------------------------
def se3_exp(xi):
    omega, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    theta = float(np.sqrt(omega @ omega))
    Wx = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if theta < 1e-12:
        R = np.eye(3) + Wx
    else:
        R = np.eye(3) + (np.sin(theta) / theta) * Wx + ((1.0 - np.cos(theta)) / (theta * theta)) * (Wx @ Wx)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, v
    return T


def solve(sums):
    A = np.zeros((6, 6), np.float64)
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    b = np.array(sums[21:27], np.float64)
    if not np.all(np.isfinite(A)) or not np.any(A):
        return None, float("inf")
    cond = float(np.linalg.cond(A))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, cond
    return np.linalg.solve(L.T, np.linalg.solve(L, b)), cond


def raycast_oracle(vol, K, pose, size, **kw):
    """The ray-cast restatement over an oracle volume."""
    return rc.raycast(vol._tsdf, vol._weight, vol._color, vol._vol_origin, f32(vol._voxel_size), f32(vol._trunc_margin), size[0], size[1], K, pose, **kw)


def icp_align(vol, depth, K, model_pose, init_pose=None, levels=3, iterations=(10, 5, 4), dist_thresh=None, angle_deg=20.0, min_pair_share=0.1,
              max_cond=np.inf, pyr_delta=0.05, round_mode=HALF_EVEN):
    """-> dict(pose, ok, pairs, rmse, cond, iterations_run, conds): ``conds`` lists cond(A) of every step that was solved."""
    model_pose = np.asarray(model_pose, np.float64).reshape(4, 4)
    init = model_pose.copy() if init_pose is None else np.array(init_pose, np.float64).reshape(4, 4)
    depths, Vs, Ns, Ks = frame_maps(depth, K, levels, pyr_delta)
    dist = float(2.0 * vol._trunc_margin if dist_thresh is None else dist_thresh)
    cos_min = float(np.cos(np.deg2rad(angle_deg)))
    its = [int(v) for v in iterations]
    its = (its[-levels:] if len(its) >= levels else [its[0]] * (levels - len(its)) + its)[::-1]
    est, pairs, rmse, cond, done, conds = init.copy(), 0, 0.0, float("inf"), 0, []
    for l in range(levels - 1, -1, -1):
        h, w = depths[l].shape
        _, mv, mn, _ = raycast_oracle(vol, Ks[l], model_pose, (h, w))
        for _ in range(its[l]):
            sums, pairs, _ = icp_step(Ks[l], Vs[l], Ns[l], mv, mn, model_pose, est, dist, cos_min, round_mode)
            done += 1
            rmse = float(np.sqrt(sums[27] / pairs)) if pairs else 0.0
            xi, cond = (None, float("inf")) if pairs < min_pair_share * h * w else solve(sums)
            if np.isfinite(cond):
                conds.append(cond)
            if xi is None or not cond <= max_cond:
                return dict(pose=init, ok=False, pairs=pairs, rmse=rmse, cond=cond, iterations_run=done, conds=conds)
            est = se3_exp(xi) @ est
    return dict(pose=est, ok=True, pairs=pairs, rmse=rmse, cond=cond, iterations_run=done, conds=conds)


def track_and_fuse(oracle, color_frames, depth_frames, K, vol_bnds, voxel_size, first_pose, **options):
    """The Tracker loop over an oracle volume -> (volume, camera-to-world poses (n, 4, 4), results)."""
    vol = oracle.TSDFVolume(vol_bnds, voxel_size)
    pose, poses, results = np.array(first_pose, np.float64), [], []
    for i, (color, depth) in enumerate(zip(color_frames, depth_frames)):
        if i == 0:
            res = dict(pose=pose.copy(), ok=True, pairs=0, rmse=0.0, cond=0.0, iterations_run=0, conds=[])
        else:
            res = icp_align(vol, depth, K, pose, **options)
        if res["ok"]:
            vol.integrate(color, depth, K, res["pose"])
            pose = res["pose"].copy()
        results.append(res)
        poses.append(pose.copy())
    return vol, np.stack(poses), results


def icp_scene(oracle, H, W, voxels):
    """The corner scene at H x W: K, an oracle volume with the first orbit frame, the restated model maps at its pose, the live maps of the second orbit frame."""
    orbit, K = tc.corner_orbit(12), tc.intrinsics(H, W)
    vol = tc.fuse_oracle(oracle, orbit[:1], K, H, W, voxels)
    _, model_v, model_n, _ = raycast_oracle(vol, K, orbit[0], (H, W))
    depth = tc.room_depth(orbit[1], K, H, W)[0]
    _, Vs, Ns, _ = frame_maps(depth, K, 1)
    return dict(K=K, vol=vol, voxels=voxels, model_v=model_v, model_n=model_n, live_v=Vs[0], live_n=Ns[0], depth=depth, orbit=orbit)
