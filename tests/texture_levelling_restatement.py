"""The exposure-gain and seam-levelling rules (include/hive_mi355x.h, above hive_texture_samples) in plain numpy and Python integers on top of
tests/texturing_restatement.py and tests/texture_smoothing_restatement.py: what csrc/texture_level.hip and hive_texture_fill_adjusted must reproduce bit for bit.
numpy's element-wise float64 operators round once per operation (no fused multiply-add), like the kernels' build; every sum "in order" starts at 0.0."""
import numpy as np

import render_restatement as RR
import texture_smoothing_restatement as SR
import texturing_restatement as TR

UNIT, MIN_Q, MAX_Q, MAX_VIEWS, MAX_SWEEPS = 65536, 16384, 262144, 256, 4096


# ---------------------------------------------------------------------------------------------------------------- samples
def samples(mesh, frames, K, poses, area, near=0.05):
    """uint16 (n, nf, 3): per view and face with area != 0 the per-channel sum of the three vertices' nearest pixels when all nine bytes lie in [1, 254], else 0."""
    faces, frames = np.asarray(mesh["faces"]), np.asarray(frames)
    n, H, W = frames.shape[:3]
    out = np.zeros((n, len(faces), 3), np.uint16)
    for view in range(n):
        R, t = TR.pose_parts(poses[view])
        X, Y, _, _ = RR.project(mesh["vertices"], K, R, t, near)
        for f in np.flatnonzero(np.asarray(area[view]) != 0):
            pixels = [frames[view][(int(Y[v]) + 128) >> 8, (int(X[v]) + 128) >> 8].astype(np.int64) for v in faces[f]]
            if all(((p >= 1) & (p <= 254)).all() for p in pixels):
                out[view, f] = (pixels[0] + pixels[1]) + pixels[2]
    return out


# ---------------------------------------------------------------------------------------------------------------- sums
def sums(table):
    """-> G (3, n, n), D (3, n, n), N (n, n) int64 over the faces valid (all three sums non-zero) in both views of a pair a != b."""
    table = np.asarray(table).astype(np.int64)
    n = table.shape[0]
    valid = (table != 0).all(axis=2)
    G, D, N = np.zeros((3, n, n), np.int64), np.zeros((3, n, n), np.int64), np.zeros((n, n), np.int64)
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            both = valid[a] & valid[b]
            N[a, b] = int(both.sum())
            for c in range(3):
                G[c, a, b] = int((table[a, both, c] * table[b, both, c]).sum())  # (int64: below 2^51, exact in any order)
                D[c, a, b] = int((table[a, both, c] * table[a, both, c]).sum())
    return G, D, N


# ---------------------------------------------------------------------------------------------------------------- solve
def solve(G, D, prior=0.01):
    """-> q uint32 (n, 3), the channels that fell back, and per channel the gains before the renormalisation (None for a channel that fell back)."""
    n, lam = G.shape[1], np.float64(prior)
    q, fallback, raw = np.full((n, 3), UNIT, np.uint32), [], []
    for c in range(3):
        e = [sum(int(D[c, a, b]) for b in range(n)) for a in range(n)]
        M, rhs = np.zeros((n, n)), np.zeros(n)
        for a in range(n):
            if e[a] == 0:
                M[a, a] = rhs[a] = 1.0
                continue
            for b in range(n):
                M[a, b] = np.float64(e[a]) + lam * np.float64(e[a]) if a == b else -np.float64(int(G[c, a, b]))
            rhs[a] = lam * np.float64(e[a])
        try:
            with np.errstate(all="ignore"):
                g = np.linalg.solve(M, rhs)
                before = g.copy()
                if not (np.isfinite(g).all() and (g > 0).all()):  # (the solve's own gains: a renormalisation would turn two negative ones positive)
                    raise np.linalg.LinAlgError
                top = bottom = np.float64(0.0)
                for a in range(n):
                    if e[a] > 0:
                        top, bottom = top + np.float64(e[a]), bottom + np.float64(e[a]) * g[a]
                for a in range(n):
                    if e[a] > 0:
                        g[a] = g[a] * top / bottom
            if not (np.isfinite(g).all() and (g > 0).all()):
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            fallback.append(c)
            raw.append(None)
            continue
        raw.append(before)
        q[:, c] = np.clip(np.floor(g * 65536.0 + 0.5), MIN_Q, MAX_Q).astype(np.uint32)
    return q, fallback, raw


# ---------------------------------------------------------------------------------------------------------------- level
def vertex_colour(P, view, frames, K, poses, q):
    """c(v, l): fill's bilinear sample at the vertex P with view l (unrounded), then (c * q) * 2^-16."""
    K = np.asarray(K, np.float64)
    H, W = frames.shape[1:3]
    R, t = TR.pose_parts(poses[view])
    with np.errstate(all="ignore"):
        c3 = TR._project([np.float64(P[0]), np.float64(P[1]), np.float64(P[2])], K, R, t)
        u = np.fmin(np.fmax(c3[0] / c3[2], 0.0), np.float64(W - 1))
        v = np.fmin(np.fmax(c3[1] / c3[2], 0.0), np.float64(H - 1))
    fu, fv = np.floor(u), np.floor(v)
    ax, ay = u - fu, v - fv
    j0, i0 = int(fu), int(fv)
    j1, i1 = min(j0 + 1, W - 1), min(i0 + 1, H - 1)
    img = frames[view]
    c00, c01, c10, c11 = (img[i, j].astype(np.float64) for i, j in ((i0, j0), (i0, j1), (i1, j0), (i1, j1)))
    top = c00 + ax * (c01 - c00)
    bottom = c10 + ax * (c11 - c10)
    c = top + ay * (bottom - top)
    return (c * np.asarray(q[view]).astype(np.float64)) * np.float64(2.0 ** -16)


def participating(faces, labels, nv, n):
    labels = np.asarray(labels)
    return SR.valid_faces(faces, nv) & (labels >= 0) & (labels < n)


def level(mesh, labels, frames, K, poses, q=None, sweeps=64):
    """-> offsets float64 (nf, 3, 3) per face corner and channel, stats dict(seam_vertices, sweeps, max_offset)."""
    faces, V, frames = np.asarray(mesh["faces"]).astype(np.int64), np.asarray(mesh["vertices"], np.float64), np.asarray(frames)
    n, nf = len(frames), len(faces)
    q = np.full((n, 3), UNIT, np.uint32) if q is None else np.asarray(q)
    part = participating(faces, labels, len(V), n)
    of_node = {}  # (v, l) -> [(f, k)] ascending f
    for f in np.flatnonzero(part):
        for k in range(3):
            of_node.setdefault((int(faces[f, k]), int(labels[f])), []).append((int(f), k))
    labels_of = {}
    for v, l in of_node:
        labels_of.setdefault(v, []).append(l)
    h, fixed = {node: np.zeros(3) for node in of_node}, set()
    seam_vertices = 0
    for v, ls in labels_of.items():
        if len(ls) < 2:
            continue
        seam_vertices += 1
        colour = {l: vertex_colour(V[v], l, frames, K, poses, q) for l in ls}
        total = np.zeros(3)
        for l in sorted(ls):
            total = total + colour[l]
        m = total / np.float64(len(ls))
        for l in ls:
            h[(v, l)] = m - colour[l]
            fixed.add((v, l))
    for _ in range(sweeps):
        after = {}
        for node, corners in of_node.items():
            if node in fixed:
                after[node] = h[node]
                continue
            l, s = node[1], np.zeros(3)
            for f, k in corners:
                s = (s + h[(int(faces[f, (k + 1) % 3]), l)]) + h[(int(faces[f, (k + 2) % 3]), l)]
            after[node] = s / np.float64(2 * len(corners))
        h = after
    offsets = np.zeros((nf, 3, 3))
    for (v, l), corners in of_node.items():
        for f, k in corners:
            offsets[f, k] = h[(v, l)]
    return offsets, dict(seam_vertices=seam_vertices, sweeps=sweeps, max_offset=float(np.abs(offsets).max()) if nf else 0.0)


def seam_nodes(mesh, labels, n):
    """{v: [(f, k)]}: per seam vertex the corners of its participating faces."""
    faces = np.asarray(mesh["faces"]).astype(np.int64)
    part = participating(faces, labels, len(mesh["vertices"]), n)
    corners, seen = {}, {}
    for f in np.flatnonzero(part):
        for k in range(3):
            corners.setdefault(int(faces[f, k]), []).append((int(f), k))
            seen.setdefault(int(faces[f, k]), set()).add(int(labels[f]))
    return {v: c for v, c in corners.items() if len(seen[v]) > 1}


# ---------------------------------------------------------------------------------------------------------------- adjusted fill
def fill_adjusted(mesh, best, frames, K, poses, S, q, offsets, near=0.05):
    """TR.fill with, on a texel with a view, byte(((c * q) * 2^-16) + ((b0 h0 + b1 h1) + b2 h2))."""
    faces, V = np.asarray(mesh["faces"]), np.asarray(mesh["vertices"], np.float64)
    colors = np.asarray(mesh["vertex_colors"])[:, :3].astype(np.float64)
    frames, K, q, offsets = np.asarray(frames), np.asarray(K, np.float64), np.asarray(q), np.asarray(offsets, np.float64)
    n, H, W = frames.shape[:3]
    nf = len(faces)
    Wt, Ht, per_row = TR.layout(nf, S)
    atlas = np.zeros((Ht, Wt, 3), np.uint8)
    for k in range((nf + 1) // 2):
        col0, row0 = (k % per_row) * S, (k // per_row) * S
        cols, rows = np.meshgrid(np.arange(col0, col0 + S), np.arange(row0, row0 + S))
        b0, b1, b2 = TR.barycentrics(cols, rows, S)
        even = (cols % S) + (rows % S) <= S - 1
        for f, mine in ((2 * k, even), (2 * k + 1, ~even)):
            if f >= nf:
                continue
            a, b, c = faces[f]
            w0, w1, w2 = b0[mine], b1[mine], b2[mine]
            key = int(best[f])
            view = 65535 - (key & 0xFFFF)
            if key == 0 or view >= n:
                atlas[rows[mine], cols[mine]] = TR._byte(np.stack([(w0 * colors[a, ch] + w1 * colors[b, ch]) + w2 * colors[c, ch] for ch in range(3)], axis=-1))
                continue
            R, t = TR.pose_parts(poses[view])
            with np.errstate(all="ignore"):
                P = [(w0 * V[a, r] + w1 * V[b, r]) + w2 * V[c, r] for r in range(3)]
                c3 = TR._project(P, K, R, t)
                behind = ~(c3[2] >= near)
                if behind.any():
                    c0 = TR._project([np.full(w0.shape, V[a, r]) for r in range(3)], K, R, t)
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
            colour = top + ay[:, None] * (bottom - top)
            h = offsets[f]
            bend = (w0[:, None] * h[0][None, :] + w1[:, None] * h[1][None, :]) + w2[:, None] * h[2][None, :]
            atlas[rows[mine], cols[mine]] = TR._byte(((colour * q[view].astype(np.float64)[None, :]) * np.float64(2.0 ** -16)) + bend)
    return atlas


# ---------------------------------------------------------------------------------------------------------------- the whole
def texture_mesh(mesh, frames, K, poses, masks=None, cell=8, depth_tolerance=0.05, near=0.05, smoothness=0.0, cull_back_faces=False, exposure=False,
                 exposure_prior=0.01, levelling=False, levelling_sweeps=64):
    """-> dict(vertices, faces, uv, texture, views, stats, gains_q16, offsets, best): ``hive_amd.texturing.texture_mesh`` with ``exposure`` or ``levelling`` (the table
    path); ``stats``: dict(smoothing = the five integers, exposure, levelling)."""
    if not (np.isfinite(exposure_prior) and exposure_prior >= 0) or not 0 <= levelling_sweeps <= MAX_SWEEPS or (exposure and len(frames) > MAX_VIEWS):
        raise ValueError("exposure_prior, levelling_sweeps or the number of frames out of range")
    frames = np.asarray(frames)
    n, H, W = frames.shape[:3]
    area = SR.vote(SR.signed_areas(mesh, K, poses, H, W, masks, depth_tolerance, near), 1 if cull_back_faces else 0)
    adjacency = SR.face_neighbours(mesh["faces"], len(mesh["vertices"]))
    best, labels, five = SR.smooth(area, *adjacency, SR.seam_cost_of(smoothness))
    stats = dict(smoothing=five)
    q = np.full((n, 3), UNIT, np.uint32)
    if exposure:
        G, D, N = sums(samples(mesh, frames, K, poses, area, near))
        q, fallback, _ = solve(G, D, exposure_prior)
        stats["exposure"] = dict(gains=q.astype(np.float64) / 65536.0, pair_counts=N, fallback_channels=fallback)
    offsets = np.zeros((len(mesh["faces"]), 3, 3))
    if levelling:
        offsets, stats["levelling"] = level(mesh, labels, frames, K, poses, q, levelling_sweeps)
    vertices, faces, uv = TR.unweld(mesh, cell)
    return dict(vertices=vertices, faces=faces, uv=uv, texture=fill_adjusted(mesh, best, frames, K, poses, cell, q, offsets, near), views=TR.views_of(best),
                stats=stats, gains_q16=q, offsets=offsets, best=best)


def psnr(a, b, where):
    d = np.asarray(a, np.float64)[where] - np.asarray(b, np.float64)[where]
    return float(10.0 * np.log10(255.0 ** 2 / np.mean(d * d)))
