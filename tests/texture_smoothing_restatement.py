"""The label-smoothing rules (include/hive_mi355x.h, above hive_texture_vote) in plain numpy and Python integers on top of tests/texturing_restatement.py: what
csrc/texture_smooth.hip must reproduce bit for bit.  Everything is an integer; nothing depends on an order of evaluation."""
import collections

import numpy as np

import render_restatement as RR
import texturing_restatement as TR

MAX_ROUNDS, MAX_DEGREE, UNITS_PER_PX2 = 4096, 65535, 131072


def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def seam_cost_of(smoothness):
    """llround(smoothness * 131072): the snapped area A is twice the area in 1/256-pixel units."""
    return int(np.floor(np.float64(smoothness) * UNITS_PER_PX2 + 0.5))


# ---------------------------------------------------------------------------------------------------------------- vote
def signed_areas(mesh, K, poses, H, W, masks=None, depth_tolerance=0.05, near=0.05):
    """int64 (n, nf): the snapped area A of every candidate of ``texturing_restatement.select`` with its sign, 0 for a face that is none."""
    faces = np.asarray(mesh["faces"])
    out = np.zeros((len(poses), len(faces)), np.int64)
    for view in range(len(poses)):
        R, t = TR.pose_parts(poses[view])
        key, _, projected = RR.rasterise([dict(vertices=mesh["vertices"], faces=faces)], K, R, t, H, W, near)
        depth = np.where(key == RR.EMPTY, np.float32(0), (key >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
        X, Y, z, keep, _ = projected[0]
        for f, tri in enumerate(faces):
            if not all(0 <= v < len(keep) and keep[v] for v in tri):
                continue
            Xs, Ys = [int(X[v]) for v in tri], [int(Y[v]) for v in tri]
            ok = True
            for k, v in enumerate(tri):
                i, j = (Ys[k] + 128) >> 8, (Xs[k] + 128) >> 8
                ok = 0 <= i < H and 0 <= j < W and (masks is None or masks[view][i, j] == 0) and \
                    bool(depth[i, j] == 0 or np.float64(z[v]) <= np.float64(depth[i, j]) + np.float64(depth_tolerance))
                if not ok:
                    break
            if ok:
                out[view, f] = (Xs[1] - Xs[0]) * (Ys[2] - Ys[0]) - (Xs[2] - Xs[0]) * (Ys[1] - Ys[0])
    return out


def vote(signed, facing=0):
    """The table d_area of n calls of hive_texture_vote: |A| where the sign passes ``facing`` (0: either, 1: A < 0, -1: A > 0)."""
    signed = np.asarray(signed, np.int64)
    passes = signed != 0 if facing == 0 else (signed < 0 if facing > 0 else signed > 0)
    return np.where(passes, np.abs(signed), 0).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- neighbours
def valid_faces(faces, nv):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < nv)).all(axis=1)
    distinct = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return in_range & distinct


def face_neighbours(faces, nv):
    """-> offsets int64 (nf + 1,), neighbours int32 (total,): per face edge (a, b) the other valid faces of a that hold b, each face's entries ascending."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(faces, nv)
    of_vertex = collections.defaultdict(list)
    for f in np.flatnonzero(ok):
        for v in faces[f]:
            of_vertex[int(v)].append(int(f))
    offsets, entries = [0], []
    for f, tri in enumerate(faces):
        mine = []
        if ok[f]:
            for k in range(3):
                a, b = int(tri[k]), int(tri[(k + 1) % 3])
                mine += [g for g in of_vertex[a] if g != f and b in faces[g]]
        entries += sorted(mine)
        offsets.append(len(entries))
    return np.asarray(offsets, np.int64), np.asarray(entries, np.int32)


# ---------------------------------------------------------------------------------------------------------------- smooth
def start_labels(area):
    area = np.asarray(area, np.int64)
    return np.where(area.max(axis=0) > 0, area.argmax(axis=0), -1).astype(np.int32)  # (argmax: the first, i.e. the lower view on a tie)


def seam_entries(labels, offsets, neighbours):
    """Neighbour entries (f, g) with f < g whose labels are both >= 0 and differ."""
    n = 0
    for f in range(len(labels)):
        for g in neighbours[offsets[f]:offsets[f + 1]]:
            n += int(g > f and labels[f] >= 0 and labels[g] >= 0 and labels[f] != labels[g])
    return n


def energy(area, labels, offsets, neighbours, seam_cost):
    kept = sum(int(area[l, f]) for f, l in enumerate(labels) if l >= 0)
    return -kept + seam_cost * seam_entries(labels, offsets, neighbours)


def proposal(area, labels, offsets, neighbours, seam_cost, f):
    """(gain, label) of face f on these labels, or None."""
    cur = int(labels[f])
    if cur < 0:
        return None
    count = collections.Counter(int(labels[g]) for g in neighbours[offsets[f]:offsets[f + 1]])
    best = None
    for l in sorted(count):
        if l < 0 or l == cur or area[l, f] == 0:
            continue
        gain = (int(area[l, f]) - int(area[cur, f])) + seam_cost * (count[l] - count[cur])
        if gain > 0 and (best is None or gain > best[0]):  # (ascending l: the lower label keeps a tie)
            best = (gain, l)
    return best


def smooth(area, offsets, neighbours, seam_cost, on_round=None):
    """-> best uint64 (nf,), labels int32 (nf,), stats int64 (5,) = rounds, label changes, seam entries before, after, area given up.  ``on_round(labels)`` is
    called with the start labels and after every round."""
    area = np.asarray(area, np.int64)
    n, nf = area.shape
    degree = np.diff(offsets)
    if not (0 <= seam_cost < 2 ** 40) or (degree > MAX_DEGREE).any() or (area < 0).any() or (area >= 2 ** 47).any():
        raise ValueError("seam_cost, a degree or an area out of range")
    labels = start_labels(area)
    first = labels.copy()
    if on_round:
        on_round(labels.copy())
    rounds = changes = 0
    while True:
        proposals = {f: p for f in range(nf) for p in [proposal(area, labels, offsets, neighbours, seam_cost, f)] if p is not None}
        if not proposals:
            break
        if rounds == MAX_ROUNDS:
            raise RuntimeError(f"{MAX_ROUNDS} rounds and faces still propose")
        after = labels.copy()
        for f, (gain, l) in proposals.items():
            rivals = [(proposals[int(g)][0], int(g)) for g in neighbours[offsets[f]:offsets[f + 1]] if int(g) in proposals]
            if all(gain > other or (gain == other and mix32(f) < mix32(g)) for other, g in rivals):
                after[f] = l
                changes += 1
        labels = after
        rounds += 1
        if on_round:
            on_round(labels.copy())
    kept = lambda L: sum(int(area[l, f]) for f, l in enumerate(L) if l >= 0)
    best = np.array([0 if l < 0 else (int(area[l, f]) << 16) | (65535 - int(l)) for f, l in enumerate(labels)], np.uint64)
    stats = np.array([rounds, changes, seam_entries(first, offsets, neighbours), seam_entries(labels, offsets, neighbours), kept(first) - kept(labels)], np.int64)
    return best, labels, stats


def patches(labels, offsets, neighbours):
    """Connected sets of labelled faces with one label (joined through neighbour entries)."""
    seen, count = np.zeros(len(labels), bool), 0
    for s in range(len(labels)):
        if seen[s] or labels[s] < 0:
            continue
        count += 1
        stack, seen[s] = [s], True
        while stack:
            f = stack.pop()
            for g in neighbours[offsets[f]:offsets[f + 1]]:
                if not seen[g] and labels[g] == labels[f]:
                    seen[g] = True
                    stack.append(int(g))
    return count


def texture_mesh(mesh, frames, K, poses, masks=None, cell=8, depth_tolerance=0.05, near=0.05, smoothness=0.0, cull_back_faces=False):
    """-> dict(vertices, faces, uv, texture, views, stats): ``hive_amd.texturing.texture_mesh(..., return_views=True, return_stats=True)`` on its smoothing path
    (``stats``: the five integers, the area in the table's unit)."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    area = vote(signed_areas(mesh, K, poses, H, W, masks, depth_tolerance, near), 1 if cull_back_faces else 0)
    offsets, neighbours = face_neighbours(mesh["faces"], len(mesh["vertices"]))
    best, labels, stats = smooth(area, offsets, neighbours, seam_cost_of(smoothness))
    vertices, faces, uv = TR.unweld(mesh, cell)
    return dict(vertices=vertices, faces=faces, uv=uv, texture=TR.fill(mesh, best, frames, K, poses, cell, near), views=TR.views_of(best), stats=stats)
