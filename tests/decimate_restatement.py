"""Test helper: a numpy / Python restatement of the parallel quadric edge collapse of csrc/decimate.hip (hive_mesh_decimate), round by round -- the same
quadric arithmetic (float64, no fused multiply-add), the same keys, 2-ring independence rule and last-round prefix -- so that the kernel can be compared with
it bit for bit.  Also a small sequential heap decimater with the same legality rules, the yardstick of the parallel schedule's quality.  Not the product."""
import heapq

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
INF_KEY = (1 << 64) - 1
MAX_ROUNDS = 4096
# a vertex's key orders by the top 5 bits of its best cost's order-mapped float32 bits -- bands of 16 octaves -- then by mix32(v0): with the full cost,
# a smooth cost field has few local minima and a round applies ~2 collapses (measured: 426 rounds for a 2.5 k-face object), with bands ~7 (200 rounds)
KEY_BAND_SHIFT = 27
# no collapse leaves v1 with more than this many faces (faces(v0) + faces(v1) - faces removed): fans stay small, and the kernel holds a vertex's
# neighbourhood in registers (without the cap, flat regions grow fans of 50+ faces whose legality checks cost O(faces^3))
MAX_FACES = 24


class DecimationStateError(RuntimeError):
    """The round cap ran out while legal collapses remained (the library's HIVE_ERR_STATE)."""


def face_quadrics(vertices, faces):
    """(F, 10) plane quadrics [aa ab ac ad bb bc bd cc cd dd] * area, each face in float64 in the kernel's operation order."""
    p = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p0, p1, p2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    a, b = p1 - p0, p2 - p0
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = np.sqrt(nx * nx + ny * ny + nz * nz)
    big = area > FLT_MIN
    safe = np.where(big, area, 1.0)
    nx, ny, nz = np.where(big, nx / safe, nx), np.where(big, ny / safe, ny), np.where(big, nz / safe, nz)
    area = np.where(big, area * 0.5, area)
    d = -(p0[:, 0] * nx + p0[:, 1] * ny + p0[:, 2] * nz)
    terms = (nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d)
    return np.stack([t * area for t in terms], axis=1)


def vertex_quadrics(vertices, faces):
    """(V, 10): every vertex sums the quadrics of its faces in ascending face index."""
    nv = len(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fq = face_quadrics(vertices, f)
    corner_v = f.ravel()
    corner_f = np.repeat(np.arange(len(f)), 3)
    order = np.lexsort((corner_f, corner_v))
    corner_v, corner_f = corner_v[order], corner_f[order]
    start = np.searchsorted(corner_v, np.arange(nv))
    rank = np.arange(len(corner_v)) - start[corner_v]
    q = np.zeros((nv, 10))
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == k
        q[corner_v[sel]] += fq[corner_f[sel]]
    return q


def qeval(q, p):
    """OpenMesh QuadricT::evaluate, left to right."""
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    a, b, c, d, e, f, g, h, i, j = (float(t) for t in q)
    return (a * x * x + 2.0 * b * x * y + 2.0 * c * x * z + 2.0 * d * x + e * y * y + 2.0 * f * y * z + 2.0 * g * y + h * z * z + 2.0 * i * z + j)


def mix32(v):
    """The low word of a key: a bijective 32-bit mix of the vertex id, so that equal costs are not ordered by position in the mesh."""
    x = int(v) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def cost_bits(cost):
    """The high word of a key: float32(cost) mapped to an order-preserving unsigned integer."""
    with np.errstate(over="ignore"):  # a finite float64 cost past float32's range is +-inf, as the kernel's cast makes it
        bits = int(np.array(cost, np.float64).astype(np.float32).view(np.uint32))
    return (~bits) & 0xffffffff if bits & 0x80000000 else bits | 0x80000000


class _Mesh:
    """Incidence of the faces alive at the start of a round."""

    def __init__(self, faces, alive):
        self.faces = faces = faces.tolist()
        self.vf = {}
        for fi in np.nonzero(alive)[0].tolist():
            for v in faces[fi]:
                self.vf.setdefault(v, []).append(fi)
        self.ec = {}  # v -> {w: faces of v that contain w}
        for v, fl in self.vf.items():
            c = {}
            for fi in fl:
                for w in faces[fi]:
                    if w != v:
                        c[w] = c.get(w, 0) + 1
            self.ec[v] = c
        self.bnd = {v: any(k == 1 for k in c.values()) for v, c in self.ec.items()}

    def nbrs(self, v):
        return self.ec.get(v, {})

    def boundary(self, v):
        return self.bnd.get(v, False)


def locked_vertices(n_vertices, faces):
    """Vertices whose boundary edges number neither 0 nor 2, and the ends of edges with more than two faces."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    m = _Mesh(faces, np.ones(len(faces), bool))
    locked = np.zeros(n_vertices, bool)
    for v, c in m.ec.items():
        nb = sum(1 for k in c.values() if k == 1)
        if nb not in (0, 2) or any(k > 2 for k in c.values()):
            locked[v] = True
    return locked


def collapse_check(m, q, pos, locked, v0, v1, max_error):
    """(None, cost, faces removed) for a legal halfedge collapse v0 -> v1 on mesh m, else (the name of the first rule that rejects it, None, 0).
    `edge faces` is never the first rule: v1 is a neighbour of v0, so the edge has a face, and the ends of an edge with more than two faces are locked
    (and no collapse makes such an edge: the link condition forbids it).  `side edges` is the first only at a vertex like decimate_cases.flag's: on a
    manifold boundary the other faces of v0 give it further boundary edges, so it is locked or rejected as `boundary` before."""
    if locked[v0] or locked[v1]:
        return "locked", None, 0
    if len(m.vf.get(v0, ())) < 2:
        return "v0 faces < 2", None, 0
    n0, n1 = m.nbrs(v0), m.nbrs(v1)
    c = n0.get(v1, 0)
    if c not in (1, 2):
        return "edge faces", None, 0
    if len(m.vf[v0]) + len(m.vf.get(v1, ())) - c > MAX_FACES:
        return "fan cap", None, 0
    opp = []
    for fi in m.vf[v0]:
        a, b, c3 = (int(x) for x in m.faces[fi])
        if a == v1 or b == v1 or c3 == v1:
            opp.append(a + b + c3 - v0 - v1)
    if len(set(opp)) != c:
        return "vl == vr", None, 0
    b0, b1 = m.boundary(v0), m.boundary(v1)
    if b0 and not (c == 1 and b1):
        return "boundary", None, 0
    if c == 2 and b0 and b1:
        return "boundary", None, 0
    if set(n0) & set(n1) != set(opp):
        return "link", None, 0
    for o in opp:
        if n0.get(o, 0) == 1 and n1.get(o, 0) == 1:
            return "side edges", None, 0
    if c == 2:
        vl, vr = opp
        if vr in m.nbrs(vl) and len(m.nbrs(vl)) == 3 and len(m.nbrs(vr)) == 3:
            return "valence 3", None, 0
    cost = qeval(q[v0] + q[v1], pos[v1])
    if not cost < max_error:
        return "max_error", None, 0
    return None, cost, c


def collapse_cost(m, q, pos, locked, v0, v1, max_error):
    """Cost of the halfedge collapse v0 -> v1 on mesh m, or None when it is not legal; also the faces it removes."""
    rule, cost, c = collapse_check(m, q, pos, locked, v0, v1, max_error)
    return None if rule else (cost, c)


def decimate(vertices, faces, budget, max_error, max_rounds=MAX_ROUNDS, trace=None, census=None):
    """The parallel rounds.  Returns (faces renumbered, kept input vertex ids, stats = (rounds, collapses, locked)).  ``trace`` (a list) receives one
    (F at round start, [(v0, v1), ...] applied, the live faces at round start) per round; ``census`` (a dict) receives, for every halfedge of the mesh
    where the rounds ended, the first rule that rejects its collapse (rule name -> count)."""
    pos = np.asarray(vertices, np.float64)
    faces = np.array(faces, np.int64).reshape(-1, 3)
    nv, nf = len(pos), len(faces)
    assert budget >= 0
    if nf <= budget:
        return faces.copy(), np.arange(nv), (0, 0, 0)
    q = vertex_quadrics(pos, faces)
    locked = locked_vertices(nv, faces)
    alive = np.ones(nf, bool)
    removed = np.zeros(nv, bool)
    f_cur, rounds, collapses = nf, 0, 0
    while f_cur > budget:
        m = _Mesh(faces, alive)
        key = np.full(nv, INF_KEY, np.uint64)
        tgt = np.full(nv, -1, np.int64)
        rem = np.zeros(nv, np.int64)
        for v0 in m.vf:
            best = None
            for v1 in m.nbrs(v0):
                r = collapse_cost(m, q, pos, locked, v0, v1, max_error)
                if r is None:
                    continue
                cand = (cost_bits(r[0]), v1, r[1])
                if best is None or cand[:2] < best[:2]:
                    best = cand
            if best is not None:
                key[v0] = np.uint64(((best[0] >> KEY_BAND_SHIFT) << 32) | mix32(v0))
                tgt[v0], rem[v0] = best[1], best[2]
        m1 = key.copy()
        fk = np.full(nf, INF_KEY, np.uint64)
        live = np.nonzero(alive)[0]
        fk[live] = key[faces[live]].min(axis=1)
        for v, fl in m.vf.items():
            m1[v] = min(m1[v], fk[fl].min())
        m2 = m1.copy()
        fk[live] = m1[faces[live]].min(axis=1)
        for v, fl in m.vf.items():
            m2[v] = min(m2[v], fk[fl].min())
        sel = [v for v in range(nv) if key[v] != INF_KEY and key[v] == m2[v] and key[v] == m2[tgt[v]]]
        if not sel:
            if census is not None:
                for v0 in m.vf:
                    for v1 in m.nbrs(v0):
                        rule = collapse_check(m, q, pos, locked, v0, v1, max_error)[0]
                        census[rule] = census.get(rule, 0) + 1
            break
        if rounds == max_rounds:
            raise DecimationStateError(f"{max_rounds} rounds and legal collapses remain")
        sel.sort(key=lambda v: int(key[v]))
        need = f_cur - budget
        cum = np.cumsum([rem[v] for v in sel])
        if cum[-1] >= need:
            sel = sel[:int(np.searchsorted(cum, need)) + 1]
        applied = [(v, int(tgt[v])) for v in sel]
        if trace is not None:
            trace.append((f_cur, applied, faces[alive].copy()))
        target = np.arange(nv)
        for v0, v1 in applied:
            target[v0] = v1
            q[v1] = q[v1] + q[v0]
            removed[v0] = True
        idx = np.nonzero(alive)[0]
        faces[idx] = target[faces[idx]]
        f = faces[idx]
        dead = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
        alive[idx[dead]] = False
        f_cur -= int(dead.sum())
        rounds += 1
        collapses += len(applied)
    kept = np.nonzero(~removed)[0]
    vmap = np.full(nv, -1, np.int64)
    vmap[kept] = np.arange(len(kept))
    return vmap[faces[alive]], kept, (rounds, collapses, int(locked.sum()))


def decimate_sequential(vertices, faces, budget, max_error):
    """OpenMesh-style greedy decimation with the same rules: a heap of every vertex's best collapse by (float32 cost, v1), the cheapest applied first,
    the neighbourhood re-evaluated after each.  Returns (faces renumbered, kept input vertex ids)."""
    pos = np.asarray(vertices, np.float64)
    faces = np.array(faces, np.int64).reshape(-1, 3)
    nv, nf = len(pos), len(faces)
    if nf <= budget:
        return faces.copy(), np.arange(nv)
    q = vertex_quadrics(pos, faces)
    locked = locked_vertices(nv, faces)
    alive = np.ones(nf, bool)
    removed = np.zeros(nv, bool)
    f_cur = nf
    vf = {}
    for fi in range(nf):
        for v in faces[fi]:
            vf.setdefault(int(v), set()).add(fi)

    class _View:  # _Mesh over the live incidence, only around the vertices asked for
        def __init__(self):
            self.faces = faces
            self.vf = vf
            self.ec = {}

        def nbrs(self, v):
            c = {}
            for fi in vf.get(v, ()):
                for w in faces[fi]:
                    if w != v:
                        c[int(w)] = c.get(int(w), 0) + 1
            return c

        def boundary(self, v):
            return any(k == 1 for k in self.nbrs(v).values())

    view = _View()
    version = np.zeros(nv, np.int64)
    heap = []

    def push(v0):
        version[v0] += 1
        best = None
        for v1 in view.nbrs(v0):
            r = collapse_cost(view, q, pos, locked, v0, v1, max_error)
            if r is not None and (best is None or (cost_bits(r[0]), v1) < best[:2]):
                best = (cost_bits(r[0]), v1)
        if best is not None:
            heapq.heappush(heap, (best[0], v0, best[1], int(version[v0])))

    for v in list(vf):
        push(v)
    while f_cur > budget and heap:
        _, v0, v1, ver = heapq.heappop(heap)
        if ver != version[v0] or removed[v0]:
            continue
        if collapse_cost(view, q, pos, locked, v0, v1, max_error) is None:
            push(v0)
            continue
        ring = set(view.nbrs(v0)) | {v0}
        for fi in list(vf[v0]):
            f = faces[fi]
            f[f == v0] = v1
            if len(set(f.tolist())) < 3:
                alive[fi] = False
                f_cur -= 1
                for w in set(f.tolist()):
                    vf[int(w)].discard(fi)
            else:
                vf.setdefault(v1, set()).add(fi)
        vf.pop(v0, None)
        q[v1] = q[v1] + q[v0]
        removed[v0] = True
        version[v0] += 1
        for w in set(view.nbrs(v1)) | {v1} | ring:
            if not removed[w]:
                push(w)
                for x in view.nbrs(w):
                    if not removed[x]:
                        push(x)
    kept = np.nonzero(~removed)[0]
    vmap = np.full(nv, -1, np.int64)
    vmap[kept] = np.arange(len(kept))
    return vmap[faces[alive]], kept


def api_decimate(vertices, faces, is_object, num_faces_object, num_faces_background, max_error):
    """``Pipeline._decimate_mesh``'s budget choice, quirk included, then ``decimate``: (vertex rows kept, faces)."""
    if (is_object and num_faces_object == -1) or num_faces_background == -1:
        return np.arange(len(vertices)), np.asarray(faces)
    budget = num_faces_object if is_object else num_faces_background
    f, kept, _ = decimate(vertices, faces, budget, max_error)
    return kept, f


# ---- test meshes ----

def grid_mesh(h, w, z=None, spacing=0.01, offset=(0.0, 0.0)):
    """(h w, 3) vertices of a pixel lattice with heights z (h, w) and two faces per cell, wound like the frame path's."""
    v, u = np.mgrid[0:h, 0:w]
    zz = np.zeros((h, w)) if z is None else np.asarray(z, np.float64)
    verts = np.stack([u.ravel() * spacing + offset[0], v.ravel() * spacing + offset[1], zz.ravel()], 1)
    ids = np.arange(h * w).reshape(h, w)
    a, b, c, d = ids[:-1, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, :-1].ravel(), ids[1:, 1:].ravel()
    faces = np.stack([np.stack([a, c, b], 1), np.stack([b, c, d], 1)], 1).reshape(-1, 3)
    return verts, faces.astype(np.int32)


def test_meshes(n=12, seed=0):
    """name -> (vertices, faces): a plane, a two-plane roof, a noisy sphere cap, an annulus (hole, isolated vertices), two components, two bowties."""
    rng = np.random.default_rng(seed)
    out = {"plane": grid_mesh(n, n)}
    v, u = np.mgrid[0:n, 0:n]
    r = n | 1  # odd: a column of vertices on the ridge
    vr, ur = np.mgrid[0:r, 0:r]
    out["roof"] = grid_mesh(r, r, 0.004 * np.abs(ur - (r - 1) // 2))
    x, y = (u - (n - 1) / 2.0) * 0.01, (v - (n - 1) / 2.0) * 0.01
    out["sphere_cap"] = grid_mesh(n, n, np.sqrt(0.09 - x * x - y * y) + rng.normal(0.0, 2e-4, (n, n)))
    verts, faces = grid_mesh(n, n, rng.normal(0.0, 1e-4, (n, n)))
    centre = verts[faces].mean(axis=1)[:, :2] - (n - 1) * 0.005
    out["annulus"] = verts, faces[(centre ** 2).sum(1) > (0.22 * n * 0.01) ** 2]
    va, fa = grid_mesh(n, n // 2 + 2, rng.normal(0.0, 1e-4, (n, n // 2 + 2)))
    vb, fb = grid_mesh(n // 2 + 2, n, rng.normal(0.0, 1e-4, (n // 2 + 2, n)), offset=(0.3, 0.0))
    out["two_components"] = np.vstack([va, vb]), np.vstack([fa, fb + len(va)]).astype(np.int32)
    # bowties: three lattices, the second shares the first's last corner, the third the second's
    m = n // 2 + 1
    parts, faces, base = [], [], 0
    for k in range(3):
        vk, fk = grid_mesh(m, m, rng.normal(0.0, 1e-4, (m, m)), offset=(k * (m - 1) * 0.01, k * (m - 1) * 0.01))
        if k:
            keep = np.arange(1, m * m)  # drop this lattice's first corner: it is the previous one's last
            remap = np.full(m * m, -1)
            remap[keep] = base + np.arange(len(keep))
            remap[0] = last
            parts.append(vk[keep])
            faces.append(remap[fk])
            base += len(keep)
        else:
            parts.append(vk)
            faces.append(fk)
            base += len(vk)
        last = base - 1
    out["bowties"] = np.vstack(parts), np.vstack(faces).astype(np.int32)
    return out


def euler_and_loops(n_vertices, faces):
    """(V - E + F over the referenced vertices, number of boundary loops, max faces on an edge)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return 0, 0, 0
    e = np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    keys, counts = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    uniq = np.stack([keys >> 32, keys & 0xffffffff], axis=1)
    chi = len(np.unique(faces)) - len(uniq) + len(faces)
    bnd = uniq[counts == 1]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in bnd.tolist():
        parent[find(a)] = find(b)
    loops = len({find(x) for x in np.unique(bnd).tolist()}) if len(bnd) else 0
    return chi, loops, int(counts.max())


def point_surface_distance(points, vertices, faces):
    """Distance of every point to the nearest triangle of (vertices, faces)."""
    tri = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    out = np.empty(len(points))
    for i, p in enumerate(np.asarray(points, np.float64)):
        ab, ac, ap = b - a, c - a, p - a
        d00, d01, d11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
        d20, d21 = (ap * ab).sum(1), (ap * ac).sum(1)
        den = np.where(np.abs(d00 * d11 - d01 * d01) > 0, d00 * d11 - d01 * d01, 1.0)
        v = (d11 * d20 - d01 * d21) / den
        w = (d00 * d21 - d01 * d20) / den
        inside = (v >= 0) & (w >= 0) & (v + w <= 1)
        proj = a + v[:, None] * ab + w[:, None] * ac
        best = np.where(inside, np.linalg.norm(p - proj, axis=1), np.inf)
        for s, t in ((a, b), (b, c), (c, a)):
            st = t - s
            u = np.clip(((p - s) * st).sum(1) / np.maximum((st * st).sum(1), 1e-300), 0.0, 1.0)
            best = np.minimum(best, np.linalg.norm(p - (s + u[:, None] * st), axis=1))
        out[i] = best.min()
    return out
