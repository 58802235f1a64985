"""The ray cast's rules (include/hive_mi355x.h, above hive_tsdf_raycast) in numpy float32, literally: what csrc/raycast.hip must reproduce bit for bit.
numpy's element-wise float32 operators round once per operation (no fused multiply-add), like the kernel's build.  All pixels march together; a pixel
that has hit or ended is frozen."""
import numpy as np

f32 = np.float32
MAX_STEPS = 1 << 20


def sample(tsdf, weight, p):
    """S at voxel coordinates p (..., 3) float32 -> (S float32, valid)."""
    X, Y, Z = tsdf.shape
    hi = np.array([X - 1, Y - 1, Z - 1], f32)
    with np.errstate(invalid="ignore"):
        inside = np.all((p >= f32(0)) & (p < hi), axis=-1)
    q = np.where(inside[..., None], p, f32(0))
    b = np.floor(q)
    f = q - b
    i = b.astype(np.int64)
    x0, y0, z0 = i[..., 0], i[..., 1], i[..., 2]
    x0, y0, z0 = np.minimum(x0, max(X - 2, 0)), np.minimum(y0, max(Y - 2, 0)), np.minimum(z0, max(Z - 2, 0))  # (only where not inside)
    x1, y1, z1 = np.minimum(x0 + 1, X - 1), np.minimum(y0 + 1, Y - 1), np.minimum(z0 + 1, Z - 1)
    valid = inside.copy()
    for xs in (x0, x1):
        for ys in (y0, y1):
            for zs in (z0, z1):
                valid &= weight[xs, ys, zs] > f32(0)
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    T = tsdf
    c00 = T[x0, y0, z0] + fz * (T[x0, y0, z1] - T[x0, y0, z0])
    c01 = T[x0, y1, z0] + fz * (T[x0, y1, z1] - T[x0, y1, z0])
    c10 = T[x1, y0, z0] + fz * (T[x1, y0, z1] - T[x1, y0, z0])
    c11 = T[x1, y1, z0] + fz * (T[x1, y1, z1] - T[x1, y1, z0])
    c0 = c00 + fy * (c01 - c00)
    c1 = c10 + fy * (c11 - c10)
    S = c0 + fx * (c1 - c0)
    return np.where(valid, S, f32(0)).astype(f32), valid


def raycast(tsdf, weight, color, origin, voxel_size, trunc, H, W, K, cam_pose, z_near=0.0, z_far=0.0, step_in_trunc=0.5, stats=None):
    """-> depth f32 (H, W), vertex f32 (H, W, 3), normal f32 (H, W, 3), colour u8 (H, W, 3).  ``stats``: a dict that receives how many rays ended on a back
    face, how many samples were invalid and how many rays never entered the box."""
    tsdf, weight = np.asarray(tsdf, f32), np.asarray(weight, f32)
    dim = np.array(tsdf.shape, np.int64)
    o = np.asarray(origin, f32).reshape(3)
    vs, step = f32(voxel_size), f32(step_in_trunc) * f32(trunc)
    K = np.asarray(K, f32).reshape(3, 3)
    pose = np.asarray(cam_pose, np.float64).reshape(4, 4).astype(f32)  # rounded once
    R, t = pose[:3, :3], pose[:3, 3]
    u, v = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    d0, d1 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    w = np.stack([(R[r, 0] * d0 + R[r, 1] * d1) + R[r, 2] for r in range(3)], axis=-1)  # (H, W, 3)
    z_in = np.full((H, W), f32(z_near), f32)
    z_out = np.full((H, W), f32(z_far) if z_far > 0 else f32(np.inf), f32)
    live = np.ones((H, W), bool)
    with np.errstate(all="ignore"):
        for r in range(3):
            g0, gd, hi = (t[r] - o[r]) / vs, w[..., r] / vs, f32(dim[r] - 1)
            nz = gd != f32(0)
            a, b = (f32(0) - g0) / gd, (hi - g0) / gd
            lo_r, hi_r = np.where(a < b, a, b), np.where(a > b, a, b)
            z_in = np.where(nz, np.where(z_in > lo_r, z_in, lo_r), z_in)
            z_out = np.where(nz, np.where(z_out < hi_r, z_out, hi_r), z_out)
            live &= nz | ((g0 >= f32(0)) & (g0 <= hi))
        live &= z_in <= z_out
        span = np.floor((z_out - z_in) / step)
    last = np.where(live, np.where(span < f32(MAX_STEPS), span, f32(MAX_STEPS)), f32(-1)).astype(np.int64)

    def voxel(z):
        return ((z[..., None] * w + t) - o) / vs

    if stats is not None:
        stats.update(back=0, invalid=0, outside=int((~live).sum()))
    hit = np.zeros((H, W), bool)
    z_hit = np.zeros((H, W), f32)
    prev_ok = np.zeros((H, W), bool)
    S_prev, z_prev = np.zeros((H, W), f32), np.zeros((H, W), f32)
    active = live.copy()
    for k in range(int(last.max()) + 1 if live.any() else 0):
        active &= k <= last
        if not active.any():
            break
        with np.errstate(all="ignore"):
            z = z_in + f32(k) * step
            S, ok = sample(tsdf, weight, voxel(z))
            both = active & ok & prev_ok
            front = both & (S_prev > f32(0)) & (S <= f32(0))
            back = both & (S_prev < f32(0)) & (S > f32(0))
            zs = z_prev + (step * S_prev) / (S_prev - S)
        if stats is not None:
            stats["back"] += int(back.sum())
            stats["invalid"] += int((active & ~ok).sum())
        z_hit = np.where(front, zs, z_hit)
        hit |= front
        active &= ~(front | back)
        prev_ok, S_prev, z_prev = np.where(active, ok, prev_ok), np.where(active, S, S_prev), np.where(active, z, z_prev)
    with np.errstate(all="ignore"):
        P = z_hit[..., None] * w + t
        q = (P - o) / vs
        g, ok = [], hit.copy()
        for r in range(3):
            e = np.zeros(3, f32)
            e[r] = 1
            a, va = sample(tsdf, weight, q + e)
            b, vb = sample(tsdf, weight, q - e)
            ok &= va & vb
            g.append(a - b)
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        ok &= length > f32(0)
        normal = np.where(ok[..., None], np.stack(g, axis=-1) / np.where(ok, length, f32(1))[..., None], f32(0)).astype(f32)
        c = np.floor(q + f32(0.5))
    c = np.where(hit[..., None], c, f32(0))
    ci = np.clip(c, 0, (dim - 1).astype(f32)).astype(np.int64)
    packed = np.asarray(color, f32)[ci[..., 0], ci[..., 1], ci[..., 2]].astype(np.uint32)
    rgb = np.stack([packed & 255, (packed >> 8) & 255, packed >> 16], axis=-1).astype(np.uint8)
    rgb = np.where(hit[..., None], rgb, 0).astype(np.uint8)
    depth = np.where(hit, z_hit, f32(0)).astype(f32)
    vertex = np.where(hit[..., None], P, f32(0)).astype(f32)
    return depth, vertex, normal, rgb
