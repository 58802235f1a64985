"""The texturing rules (include/hive_mi355x.h, above hive_texture_select) in plain numpy on top of tests/render_restatement.py: what csrc/texture.hip must
reproduce bit for bit.  numpy's element-wise float64 operators round once per operation (no fused multiply-add), like the kernels' build.

A mesh is a dict: ``vertices`` (V, 3), ``faces`` (F, 3), ``vertex_colors`` uint8 (V, 3+)."""
import numpy as np

import render_restatement as RR

MAX_ATLAS, MAX_VIEWS = 16384, 65535


def layout(nf, S):
    """-> (Wt, Ht, per_row): two faces per S x S block, per_row = ceil(sqrt(blocks)) blocks in a row."""
    if nf < 1 or not 6 <= S <= 64:
        raise ValueError(f"{nf} faces, cell {S}")
    blocks = (nf + 1) // 2
    per_row = int(np.ceil(np.sqrt(blocks)))
    while per_row * per_row < blocks:
        per_row += 1
    while per_row > 1 and (per_row - 1) ** 2 >= blocks:
        per_row -= 1
    rows = -(-blocks // per_row)
    if per_row * S > MAX_ATLAS or rows * S > MAX_ATLAS:
        raise ValueError(f"atlas {per_row * S} x {rows * S} exceeds {MAX_ATLAS}")
    return per_row * S, rows * S, per_row


def corners(f, S, per_row):
    """The three corner texels (col, row) of face f in the atlas."""
    k = f // 2
    col0, row0 = (k % per_row) * S, (k // per_row) * S
    local = [(S - 2, S - 2), (3, S - 2), (S - 2, 3)] if f & 1 else [(1, 1), (S - 4, 1), (1, S - 4)]
    return [(col0 + x, row0 + y) for x, y in local]


def owner(col, row, S, per_row):
    """The face that owns atlas texel (col, row) (possibly >= nf)."""
    x, y = col % S, row % S
    return 2 * ((row // S) * per_row + col // S) + (0 if x + y <= S - 1 else 1)


def barycentrics(col, row, S):
    """(b0, b1, b2) of atlas texels (arrays) under their owner's affine map."""
    x, y = np.asarray(col) % S, np.asarray(row) % S
    even = x + y <= S - 1
    b1 = np.where(even, x - 1, S - 2 - x).astype(np.float64) / np.float64(S - 5)
    b2 = np.where(even, y - 1, S - 2 - y).astype(np.float64) / np.float64(S - 5)
    return (1.0 - b1) - b2, b1, b2


def pose_parts(pose):
    pose = np.asarray(pose, np.float64)
    return pose[:3, :3], pose[:3, 3]


def select(mesh, K, poses, H, W, masks=None, depth_tolerance=0.05, near=0.05, order=None):
    """best uint64 [nf] after every view's vote (``order``: the sequence in which the views vote; the result must not depend on it)."""
    faces = np.asarray(mesh["faces"])
    best = np.zeros(len(faces), np.uint64)
    for view in (range(len(poses)) if order is None else order):
        R, t = pose_parts(poses[view])
        key, _, projected = RR.rasterise([dict(vertices=mesh["vertices"], faces=faces)], K, R, t, H, W, near)
        depth = np.where(key == RR.EMPTY, np.float32(0), (key >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)  # hive_render_resolve's plane
        X, Y, z, keep, _ = projected[0]
        for f, tri in enumerate(faces):
            if not all(keep[v] for v in tri):
                continue
            Xs, Ys = [int(X[v]) for v in tri], [int(Y[v]) for v in tri]
            ok = True
            for k, v in enumerate(tri):
                i, j = (Ys[k] + 128) >> 8, (Xs[k] + 128) >> 8
                if not (0 <= i < H and 0 <= j < W):
                    ok = False
                elif masks is not None and masks[view][i, j] != 0:
                    ok = False
                elif not (depth[i, j] == 0 or np.float64(z[v]) <= np.float64(depth[i, j]) + np.float64(depth_tolerance)):
                    ok = False
                if not ok:
                    break
            area = (Xs[1] - Xs[0]) * (Ys[2] - Ys[0]) - (Xs[2] - Xs[0]) * (Ys[1] - Ys[0])
            if not ok or area == 0:
                continue
            key = (abs(area) << 16) | (65535 - view)
            best[f] = max(int(best[f]), key)
    return best


def views_of(best):
    return np.where(best == 0, -1, 65535 - (best & np.uint64(0xFFFF)).astype(np.int64)).astype(np.int32)


def unweld(mesh, S):
    """-> vertices' (3 nf, 3) float64, faces' (nf, 3) int32, uv (3 nf, 2) float64."""
    faces, V = np.asarray(mesh["faces"]), np.asarray(mesh["vertices"], np.float64)
    nf = len(faces)
    Wt, Ht, per_row = layout(nf, S)
    vertices = V[faces.reshape(-1)]
    uv = np.empty((3 * nf, 2), np.float64)
    for f in range(nf):
        for k, (col, row) in enumerate(corners(f, S, per_row)):
            uv[3 * f + k] = np.float64(col) / np.float64(Wt), 1.0 - np.float64(row) / np.float64(Ht)
    return vertices, np.arange(3 * nf, dtype=np.int32).reshape(nf, 3), uv


def _byte(c):
    return np.minimum(255.0, np.maximum(0.0, np.floor(c + 0.5))).astype(np.uint8)


def _project(P, K, R, t):
    cam = [((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + t[r] for r in range(3)]
    return [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]


def fill(mesh, best, frames, K, poses, S, near=0.05):
    """The atlas uint8 (Ht, Wt, 3)."""
    faces, V = np.asarray(mesh["faces"]), np.asarray(mesh["vertices"], np.float64)
    colors = np.asarray(mesh["vertex_colors"])[:, :3].astype(np.float64)
    frames, K = np.asarray(frames), np.asarray(K, np.float64)
    n, H, W = frames.shape[:3]
    nf = len(faces)
    Wt, Ht, per_row = layout(nf, S)
    atlas = np.zeros((Ht, Wt, 3), np.uint8)
    for k in range((nf + 1) // 2):
        col0, row0 = (k % per_row) * S, (k // per_row) * S
        cols, rows = np.meshgrid(np.arange(col0, col0 + S), np.arange(row0, row0 + S))
        b0, b1, b2 = barycentrics(cols, rows, S)
        even = (cols % S) + (rows % S) <= S - 1
        for f, mine in ((2 * k, even), (2 * k + 1, ~even)):
            if f >= nf:
                continue
            a, b, c = faces[f]
            w0, w1, w2 = b0[mine], b1[mine], b2[mine]
            key = int(best[f])
            view = 65535 - (key & 0xFFFF)
            if key == 0 or view >= n:
                atlas[rows[mine], cols[mine]] = _byte(np.stack([(w0 * colors[a, ch] + w1 * colors[b, ch]) + w2 * colors[c, ch] for ch in range(3)], axis=-1))
                continue
            R, t = pose_parts(poses[view])
            with np.errstate(all="ignore"):
                P = [(w0 * V[a, r] + w1 * V[b, r]) + w2 * V[c, r] for r in range(3)]
                c3 = _project(P, K, R, t)
                behind = ~(c3[2] >= near)
                if behind.any():  # vertex 0, which the draw kept
                    c0 = _project([np.full(w0.shape, V[a, r]) for r in range(3)], K, R, t)
                    c3 = [np.where(behind, c0[r], c3[r]) for r in range(3)]
                u = np.fmin(np.fmax(c3[0] / c3[2], 0.0), np.float64(W - 1))
                v = np.fmin(np.fmax(c3[1] / c3[2], 0.0), np.float64(H - 1))
            fu, fv = np.floor(u), np.floor(v)
            ax, ay = u - fu, v - fv
            j0, i0 = fu.astype(np.int64), fv.astype(np.int64)
            j1, i1 = np.minimum(j0 + 1, W - 1), np.minimum(i0 + 1, H - 1)
            img = frames[view].astype(np.float64)
            c00, c01, c10, c11 = img[i0, j0], img[i0, j1], img[i1, j0], img[i1, j1]
            top = c00 + ax[:, None] * (c01 - c00)
            bottom = c10 + ax[:, None] * (c11 - c10)
            atlas[rows[mine], cols[mine]] = _byte(top + ay[:, None] * (bottom - top))
    return atlas


def texture_mesh(mesh, frames, K, poses, masks=None, cell=8, depth_tolerance=0.05, near=0.05, order=None):
    """-> dict(vertices, faces, uv, texture, views), the restatement of ``hive_amd.texturing.texture_mesh(..., return_views=True)``.  ``poses``: (n, 4, 4)."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    best = select(mesh, K, poses, H, W, masks, depth_tolerance, near, order)
    vertices, faces, uv = unweld(mesh, cell)
    return dict(vertices=vertices, faces=faces, uv=uv, texture=fill(mesh, best, frames, K, poses, cell, near), views=views_of(best))
