"""The rasteriser's rules (include/hive_mi355x.h, above hive_render_clear) in numpy, face by face and literally: what csrc/render.hip must reproduce bit for
bit.  numpy's element-wise float64 operators round once per operation (no fused multiply-add), like the kernels' build.

A mesh is a dict: ``vertices`` (V, 3), ``faces`` (F, 3), and ``vertex_colors`` uint8 (V, 3+) or ``uv`` (V, 2) with ``texture`` uint8 (Ht, Wt, 3)."""
import numpy as np

SUB = 256  # 8 sub-pixel bits
GUARD = 65536.0
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(vertices, K, R, t, near):
    """hive_project's operation order -> (X, Y) snapped int64, z, keep."""
    V = np.asarray(vertices, np.float64)
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all="ignore"):
        cam = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
        c = [(K[r, 0] * cam[0] + K[r, 1] * cam[1]) + K[r, 2] * cam[2] for r in range(3)]
        sx, sy = c[0] / c[2], c[1] / c[2]
        keep = (c[2] >= near) & (np.abs(sx) < GUARD) & (np.abs(sy) < GUARD)
        X = np.where(keep, np.floor(np.where(keep, sx, 0.0) * SUB + 0.5), 0.0).astype(np.int64)
        Y = np.where(keep, np.floor(np.where(keep, sy, 0.0) * SUB + 0.5), 0.0).astype(np.int64)
    return X, Y, c[2], keep


def _setup(X, Y, z, keep, tri):
    """None for a rejected face, else (X[3], Y[3], z[3], |A|, order) with vertices 1 and 2 swapped when the area was negative."""
    a, b, c = (int(v) for v in tri)
    if not (keep[a] and keep[b] and keep[c]):
        return None
    order = [a, b, c]
    Xs, Ys = [int(X[v]) for v in order], [int(Y[v]) for v in order]  # Python integers: exact
    area = (Xs[1] - Xs[0]) * (Ys[2] - Ys[0]) - (Xs[2] - Xs[0]) * (Ys[1] - Ys[0])
    if area == 0:
        return None
    if area < 0:
        order = [a, c, b]
        Xs, Ys = [int(X[v]) for v in order], [int(Y[v]) for v in order]
    return Xs, Ys, [np.float64(z[v]) for v in order], abs(area), order


def _edges(Xs, Ys, px, py):
    """w_e (int64 arrays) at the sample points and the coverage by the top-left rule."""
    w, inside = [], np.ones(np.shape(px), bool)
    for e in range(3):
        p, q = (e + 1) % 3, (e + 2) % 3  # the edge opposite vertex e
        dx, dy = Xs[q] - Xs[p], Ys[q] - Ys[p]
        we = dx * (py - Ys[p]) - dy * (px - Xs[p])
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= (we > 0) | ((we == 0) & top_left)
        w.append(we)
    return w, inside


def rasterise(meshes, K, R, t, H, W, near=0.05):
    """The key plane uint64 (H, W), how often each pixel was covered, and per mesh its projection."""
    key = np.full((H, W), EMPTY, np.uint64)
    cover = np.zeros((H, W), np.int32)
    projected, base = [], 0
    for mesh in meshes:
        X, Y, z, keep = project(mesh["vertices"], K, R, t, near)
        projected.append((X, Y, z, keep, base))
        for f, tri in enumerate(np.asarray(mesh["faces"])):
            s = _setup(X, Y, z, keep, tri)
            if s is None:
                continue
            Xs, Ys, zs, area, _ = s
            j0, j1 = max(0, -(-min(Xs) // SUB)), min(W - 1, max(Xs) // SUB)
            i0, i1 = max(0, -(-min(Ys) // SUB)), min(H - 1, max(Ys) // SUB)
            if j0 > j1 or i0 > i1:
                continue
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(i0, i1 + 1, dtype=np.int64))
            w, inside = _edges(Xs, Ys, jj * SUB, ii * SUB)
            q = [w[e].astype(np.float64) / zs[e] for e in range(3)]
            den = (q[0] + q[1]) + q[2]
            with np.errstate(all="ignore"):
                depth = (1.0 / (den / np.float64(area))).astype(np.float32)
            k = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(base + f)
            sub = key[i0:i1 + 1, j0:j1 + 1]
            sub[inside] = np.minimum(sub[inside], k[inside])
            cover[i0:i1 + 1, j0:j1 + 1] += inside
        base += len(mesh["faces"])
    return key, cover, projected


def render(meshes, K, R, t, H, W, near=0.05, background=(255, 255, 255)):
    """-> colour uint8 (H, W, 3), depth float32 (H, W), face int32 (H, W), cover int32 (H, W)."""
    meshes = [m for m in meshes if m is not None and len(m["faces"]) and len(m["vertices"])]
    key, cover, projected = rasterise(meshes, K, R, t, H, W, near)
    empty = key == EMPTY
    face = np.where(empty, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, np.float32(0), (key >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
    color = np.empty((H, W, 3), np.uint8)
    color[:] = np.asarray(background, np.uint8)
    for mesh, (X, Y, z, keep, base) in zip(meshes, projected):
        faces = np.asarray(mesh["faces"])
        for i, j in zip(*np.nonzero((face >= base) & (face < base + len(faces)))):
            Xs, Ys, zs, _, order = _setup(X, Y, z, keep, faces[face[i, j] - base])
            w, _ = _edges(Xs, Ys, np.int64(j) * SUB, np.int64(i) * SUB)
            q = [np.float64(w[e]) / zs[e] for e in range(3)]
            den = (q[0] + q[1]) + q[2]
            if mesh.get("vertex_colors") is not None:
                a = np.asarray(mesh["vertex_colors"])[order, :3].astype(np.float64)
                c = ((q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]) / den
                color[i, j] = np.minimum(255.0, np.floor(c + 0.5)).astype(np.uint8)
            else:
                uv, tex = np.asarray(mesh["uv"], np.float64)[order], np.asarray(mesh["texture"])
                ht, wt = tex.shape[:2]
                u, v = ((q[0] * uv[0] + q[1] * uv[1]) + q[2] * uv[2]) / den
                col = int(np.clip(np.floor(u * wt + 0.5), 0, wt - 1))
                row = int(np.clip(np.floor((1.0 - v) * ht + 0.5), 0, ht - 1))
                color[i, j] = tex[row, col, :3]
    return color, depth, face, cover
