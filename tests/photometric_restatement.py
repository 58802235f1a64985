"""The photometric term's rules (include/hive_mi355x.h, above hive_gray_pyramid and hive_rgbd_icp_step) in numpy, literally: what csrc/track.hip must reproduce
-- the intensity pyramid bit for bit in float32, the photometric terms in float64 per pixel, the sums in the kernel's order.  Then ``icp_align`` with colour and
the track-and-fuse loop of hive_amd/tracking.py restated on the host over an oracle volume; the geometric half is tests/tracking_restatement.py as it stands."""
import numpy as np

import tracking_restatement as tr

f32 = np.float32
HALF_EVEN = tr.HALF_EVEN


# ---- hive_gray_pyramid ----------------------------------------------------------------------------------------------------------------------------------
def luma(color):
    """Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 of a uint8 (..., 3) picture, as integers."""
    c = np.asarray(color, np.uint8).astype(np.int64)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16


def gray(color):
    """Y / 255 in float32."""
    return (luma(color).astype(f32) / f32(255)).astype(f32)


def gray_down(I):
    I = np.asarray(I, f32)
    H, W = I.shape[0] // 2, I.shape[1] // 2
    a, b, c, d = I[0:2 * H:2, 0:2 * W:2], I[0:2 * H:2, 1:2 * W:2], I[1:2 * H:2, 0:2 * W:2], I[1:2 * H:2, 1:2 * W:2]
    return (((a + b) + (c + d)) * f32(0.25)).astype(f32)


def gray_pyramid(color, levels):
    out = [gray(color)]
    for _ in range(1, levels):
        out.append(gray_down(out[-1]))
    return out


# ---- the photometric half of hive_rgbd_icp_step ---------------------------------------------------------------------------------------------------------
def photo_terms(K, live_v, live_I, model_I, model_depth, model_pose, est_pose, dist_thresh, details=None):
    """-> terms float64 (H W, 29) (28 sums' terms and the pair flag) and the mask bool (H, W).  ``model_I`` is the model's intensity plane float32 (H, W).
    ``details``: a dict that receives the residual ``r`` (H W) and the Jacobian ``J`` (H W, 6) of every pixel (meaningful where the mask is set)."""
    H, W = live_v.shape[:2]
    K = np.asarray(K, f32).reshape(3, 3).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    est = np.asarray(est_pose, np.float64).reshape(4, 4)
    R, t = est[:3, :3], est[:3, 3]
    Mi, Mt = tr.invert_pose(model_pose)
    Rm = Mi.T
    V = live_v.reshape(-1, 3).astype(np.float64)
    n_px = V.shape[0]
    if H < 4 or W < 4:
        if details is not None:
            details.update(r=np.zeros(n_px), J=np.zeros((n_px, 6)))
        return np.zeros((n_px, 29)), np.zeros((H, W), bool)
    Il = np.asarray(live_I, f32).reshape(-1).astype(np.float64)
    Im = np.asarray(model_I, f32).astype(np.float64)
    Dm = np.asarray(model_depth, f32)
    keep = live_v.reshape(-1, 3)[:, 2] > 0
    q = [((R[r, 0] * V[:, 0] + R[r, 1] * V[:, 1]) + R[r, 2] * V[:, 2]) + t[r] for r in range(3)]
    c = [((Mi[r, 0] * q[0] + Mi[r, 1] * q[1]) + Mi[r, 2] * q[2]) + Mt[r] for r in range(3)]
    keep &= c[2] > 0
    with np.errstate(all="ignore"):
        pu, pv = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        x0f, y0f = np.floor(pu), np.floor(pv)
        keep &= (x0f >= 1) & (x0f <= W - 3) & (y0f >= 1) & (y0f <= H - 3)
        x0, y0 = np.where(keep, x0f, 1).astype(np.int64), np.where(keep, y0f, 1).astype(np.int64)
        a, b = pu - x0f, pv - y0f
    # gradients and usability at every integer model pixel away from the border
    gx, gy, usable = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), bool)
    gx[:, 1:-1] = 0.5 * (Im[:, 2:] - Im[:, :-2])
    gy[1:-1, :] = 0.5 * (Im[2:, :] - Im[:-2, :])
    ok = Dm > 0
    usable[1:-1, 1:-1] = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
    for dy in (0, 1):
        for dx in (0, 1):
            keep &= usable[y0 + dy, x0 + dx]

    def sample(A):
        top = A[y0, x0] + a * (A[y0, x0 + 1] - A[y0, x0])
        bot = A[y0 + 1, x0] + a * (A[y0 + 1, x0 + 1] - A[y0 + 1, x0])
        return top + b * (bot - top)

    with np.errstate(all="ignore"):
        I, sgx, sgy = sample(Im), sample(gx), sample(gy)
        xn, yn = x0 + (a >= 0.5), y0 + (b >= 0.5)
        keep &= np.abs(Dm[yn, xn].astype(np.float64) - c[2]) <= np.float64(f32(dist_thresh))
        r = Il - I
        gfx, gfy = sgx * fx, sgy * fy
        gc = [gfx / c[2], gfy / c[2], -((gfx * c[0] + gfy * c[1]) / (c[2] * c[2]))]
        gw = [(Rm[k, 0] * gc[0] + Rm[k, 1] * gc[1]) + Rm[k, 2] * gc[2] for k in range(3)]
        J = [q[1] * gw[2] - q[2] * gw[1], q[2] * gw[0] - q[0] * gw[2], q[0] * gw[1] - q[1] * gw[0], gw[0], gw[1], gw[2]]
        cols = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r, np.ones_like(r)]
    terms = np.where(keep[:, None], np.stack(cols, axis=1), 0.0)
    if details is not None:
        details.update(r=r, J=np.stack(J, axis=1))
    return terms, keep.reshape(H, W)


def rgbd_icp_step(K, live_v, live_n, live_I, model_v, model_n, model_depth, model_color, model_pose, est_pose, dist_thresh, cos_thresh, round_mode=HALF_EVEN):
    """-> sums float64 [56], (geometric pairs, photometric pairs), (pair mask, photometric mask)."""
    g_terms, g_mask = tr.icp_terms(K, live_v, live_n, model_v, model_n, model_pose, est_pose, dist_thresh, cos_thresh, round_mode)
    p_terms, p_mask = photo_terms(K, live_v, live_I, gray(model_color), model_depth, model_pose, est_pose, dist_thresh)
    g_sums, g_pairs = tr.icp_sums(g_terms)
    p_sums, p_pairs = tr.icp_sums(p_terms)
    return np.concatenate([g_sums, p_sums]), (g_pairs, p_pairs), (g_mask, p_mask)


# ---- hive_amd/tracking.py on the host -------------------------------------------------------------------------------------------------------------------
def combine(sums, weight):
    """The 28 sums of A = A_geo + w^2 A_photo, b = b_geo + w^2 b_photo; the last one stays the geometric sum of r^2."""
    out = np.array(sums[:28], np.float64)
    w2 = float(weight) * float(weight)
    out[:27] = out[:27] + w2 * np.asarray(sums[28:55], np.float64)
    return out


def icp_align(vol, depth, K, model_pose, color=None, photometric_weight=0.0, init_pose=None, levels=3, iterations=(10, 5, 4), dist_thresh=None, angle_deg=20.0,
              min_pair_share=0.1, max_cond=np.inf, pyr_delta=0.05, round_mode=HALF_EVEN):
    """As tracking_restatement.icp_align, which it IS without a colour or with a weight of 0."""
    if color is None or photometric_weight == 0:
        return tr.icp_align(vol, depth, K, model_pose, init_pose, levels, iterations, dist_thresh, angle_deg, min_pair_share, max_cond, pyr_delta, round_mode)
    model_pose = np.asarray(model_pose, np.float64).reshape(4, 4)
    init = model_pose.copy() if init_pose is None else np.array(init_pose, np.float64).reshape(4, 4)
    depths, Vs, Ns, Ks = tr.frame_maps(depth, K, levels, pyr_delta)
    Is = gray_pyramid(color, levels)
    dist = float(2.0 * vol._trunc_margin if dist_thresh is None else dist_thresh)
    cos_min = float(np.cos(np.deg2rad(angle_deg)))
    its = [int(v) for v in iterations]
    its = (its[-levels:] if len(its) >= levels else [its[0]] * (levels - len(its)) + its)[::-1]
    est, pairs, rmse, cond, done, conds = init.copy(), 0, 0.0, float("inf"), 0, []
    for l in range(levels - 1, -1, -1):
        h, w = depths[l].shape
        md, mv, mn, mc = tr.raycast_oracle(vol, Ks[l], model_pose, (h, w))
        for _ in range(its[l]):
            sums, (pairs, _), _ = rgbd_icp_step(Ks[l], Vs[l], Ns[l], Is[l], mv, mn, md, mc, model_pose, est, dist, cos_min, round_mode)
            done += 1
            rmse = float(np.sqrt(sums[27] / pairs)) if pairs else 0.0
            xi, cond = (None, float("inf")) if pairs < min_pair_share * h * w else tr.solve(combine(sums, photometric_weight))
            if np.isfinite(cond):
                conds.append(cond)
            if xi is None or not cond <= max_cond:
                return dict(pose=init, ok=False, pairs=pairs, rmse=rmse, cond=cond, iterations_run=done, conds=conds)
            est = tr.se3_exp(xi) @ est
    return dict(pose=est, ok=True, pairs=pairs, rmse=rmse, cond=cond, iterations_run=done, conds=conds)


def track_and_fuse(oracle, color_frames, depth_frames, K, vol_bnds, voxel_size, first_pose, photometric_weight=0.0, **options):
    """The Tracker loop over an oracle volume -> (volume, camera-to-world poses (n, 4, 4), results); the colour goes to icp_align when the weight is > 0."""
    vol = oracle.TSDFVolume(vol_bnds, voxel_size)
    pose, poses, results = np.array(first_pose, np.float64), [], []
    for i, (color, depth) in enumerate(zip(color_frames, depth_frames)):
        if i == 0:
            res = dict(pose=pose.copy(), ok=True, pairs=0, rmse=0.0, cond=0.0, iterations_run=0, conds=[])
        else:
            res = icp_align(vol, depth, K, pose, color=color if photometric_weight > 0 else None, photometric_weight=photometric_weight, **options)
        if res["ok"]:
            vol.integrate(color, depth, K, res["pose"])
            pose = res["pose"].copy()
        results.append(res)
        poses.append(pose.copy())
    return vol, np.stack(poses), results
