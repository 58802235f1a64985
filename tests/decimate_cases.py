"""Cases for csrc/decimate.hip (hive_mesh_decimate) beyond open lattice patches: closed surfaces, non-manifold input, fans at the face cap, extreme
scales, rounds wider than thresh's workgroup (tests/test_decimate_cases_cpu.py proves with the restatement alone that every case is what its name
says; tests/test_decimate_edges_gpu.py runs them on the GPU).  Every builder is deterministic and returns (float64 vertices (V, 3), int32 faces (F, 3)).
The yardstick stays tests/decimate_restatement.py; this module only builds meshes, counts rejections and shares cached runs of the restatement."""
import ctypes
import functools

import numpy as np

import decimate_restatement as D

RULES = ("locked", "v0 faces < 2", "edge faces", "fan cap", "vl == vr", "boundary", "link", "side edges", "valence 3", "max_error")
THRESH_THREADS = 1024  # dec_thresh_kernel: one workgroup, the selected list is read in strides of this


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------------
def _mesh(vertices, faces):
    return np.ascontiguousarray(vertices, np.float64).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([[0.0, 0.0, 0.0], [0.1, 0.0, 0.01], [0.0, 0.1, 0.02], [0.03, 0.02, 0.1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])


def pillow():
    """Two faces on one vertex triple, back to back, and one isolated vertex."""
    return _mesh([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.01], [0.5, 0.5, 0.5]], [[0, 1, 2], [0, 2, 1]])


def torus(n, m, seed=5):
    """A torus of n x m vertices (n around the axis), two faces per cell, 1 % noise on the tube radius."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:n, 0:m]
    u, v = 2.0 * np.pi * i / n, 2.0 * np.pi * j / m
    r = 0.03 * (1.0 + 0.01 * rng.standard_normal((n, m)))
    verts = np.stack([(0.1 + r * np.cos(v)) * np.cos(u), (0.1 + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    a, b, c, d = i * m + j, (i + 1) % n * m + j, i * m + (j + 1) % m, (i + 1) % n * m + (j + 1) % m
    faces = np.stack([np.stack([a, b, c], -1), np.stack([b, d, c], -1)], 2).reshape(-1, 3)
    return _mesh(verts, faces)


def torus_3x3():
    return torus(3, 3)


def icosphere(subdivisions, noise=0.01, seed=7):
    """A unit icosahedron subdivided, every vertex pushed to radius 0.1 (1 + noise * normal)."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(v, np.float64) for v in verts]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                mid[k] = len(verts)
                verts.append((verts[a] + verts[b]) * 0.5)
            return mid[k]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    v = np.array(verts)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    return _mesh(v * (0.1 * (1.0 + noise * rng.standard_normal(len(v))))[:, None], faces)


def spindle(k, height=0.1):
    """A closed double cone: a wavy ring of k vertices (ids 0 .. k - 1) and the apexes k (above) and k + 1 (below), k faces on each.  At the default
    height a collapse at an apex costs bands more than one along the ring, so the ring shrinks first; at 0.001 (`flat_spindle`) all costs share a
    band, the apexes compete from the first round and the result depends on the cap being exactly 24 (test_decimate_cases_cpu.py)."""
    th = 2.0 * np.pi * np.arange(k) / k
    ring = np.stack([0.1 * np.cos(th), 0.1 * np.sin(th), 0.004 * np.sin(3.0 * th) + 0.002 * np.cos(7.0 * th + 0.3)], 1)
    verts = np.vstack([ring, [[0.0, 0.0, height], [0.0, 0.0, -height]]])
    i = np.arange(k)
    n = (i + 1) % k
    faces = np.vstack([np.stack([np.full(k, k), i, n], 1), np.stack([np.full(k, k + 1), n, i], 1)])
    return _mesh(verts, faces)


def fan(k):
    """An open fan of k faces: the apex is vertex 0, the rim vertices 1 .. k + 1 lie on three quarters of a wavy circle."""
    th = 1.5 * np.pi * np.arange(k + 1) / k
    rim = np.stack([0.1 * np.cos(th), 0.1 * np.sin(th), 0.003 * np.sin(5.0 * th)], 1)
    i = np.arange(1, k + 1)
    return _mesh(np.vstack([[[0.0, 0.0, 0.01]], rim]), np.stack([np.zeros(k, np.int64), i, i + 1], 1))


BOOK_PAGE = 4


def book(pages, n=BOOK_PAGE, seed=11):
    """`pages` lattices of n x n vertices that share their first column (the spine: vertices 0 .. n - 1), spread around it; every other vertex has
    a little noise.  With three pages every spine edge has three faces."""
    rng = np.random.default_rng(seed)
    verts = [np.stack([np.zeros(n), np.arange(n) * 0.01, np.zeros(n)], 1)]
    faces, base = [], n
    for p in range(pages):
        ang = 2.0 * np.pi * p / pages + 0.2
        ids = np.empty((n, n), np.int64)  # [row along the spine][column away from it]
        ids[:, 0] = np.arange(n)
        ids[:, 1:] = base + np.arange(n * (n - 1)).reshape(n, n - 1)
        r, c = np.mgrid[0:n, 1:n]
        page = np.stack([c * 0.01 * np.cos(ang), r * 0.01, c * 0.01 * np.sin(ang)], -1) + rng.normal(0.0, 1e-4, (n, n - 1, 3))
        verts.append(page.reshape(-1, 3))
        base += n * (n - 1)
        a, b, c2, d = ids[:-1, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, :-1].ravel(), ids[1:, 1:].ravel()
        faces.append(np.stack([np.stack([a, c2, b], 1), np.stack([b, c2, d], 1)], 1).reshape(-1, 3))
    return _mesh(np.vstack(verts), np.vstack(faces))


def flag():
    """A closed fan of six faces around vertex 0 (rim 1 .. 6) and the triangle (0, 7, 8) that touches it only there.  Vertex 0 has two boundary edges,
    so it is not locked, and 0 -> 7 and 0 -> 8 run along a boundary edge whose opposite vertex is joined to both ends by boundary edges: the one
    input found on which the `side edges` rule is the first to reject."""
    th = 2.0 * np.pi * np.arange(6) / 6
    rim = np.stack([0.1 * np.cos(th), 0.1 * np.sin(th), 0.004 * np.sin(2.0 * th + 0.5)], 1)
    verts = np.vstack([[[0.0, 0.0, 0.01]], rim, [[0.02, 0.01, 0.1], [-0.03, 0.02, 0.11]]])
    i = np.arange(6)
    faces = np.vstack([np.stack([np.zeros(6, np.int64), 1 + i, 1 + (i + 1) % 6], 1), [[0, 7, 8]]])
    return _mesh(verts, faces)


def noisy_lattice(n, seed=3):
    return D.grid_mesh(n, n, np.random.default_rng(seed).normal(0.0, 1e-4, (n, n)))


def tilted_plane(n):
    """z = 0.5 + 0.3 x + 0.2 y over the lattice: exactly planar up to rounding, so the costs are rounding noise of either sign around zero."""
    verts, faces = D.grid_mesh(n, n)
    verts[:, 2] = 0.5 + 0.3 * verts[:, 0] + 0.2 * verts[:, 1]
    return _mesh(verts, faces)


def degenerate(n):
    """The noisy lattice with vertex (5, 6) moved onto its neighbour (5, 5) -- the faces on that edge have area exactly 0 -- and a NaN vertex at (2, 8)."""
    verts, faces = noisy_lattice(n)
    verts = verts.copy()
    verts[5 * n + 6] = verts[5 * n + 5]
    verts[degenerate_nan_vertex(n)] = np.nan
    return _mesh(verts, faces)


def degenerate_nan_vertex(n):
    return 2 * n + 8


def scaled(n, factor):
    verts, faces = noisy_lattice(n)
    return _mesh(verts * factor, faces)


def wide_lattice(n):
    """n x n vertices with normal(0, 1e-4) heights, seed 1: at n = 200 the first round selects more collapses than dec_thresh_kernel has threads."""
    return D.grid_mesh(n, n, np.random.default_rng(1).normal(0.0, 1e-4, (n, n)))


def one_face():
    return _mesh([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0]], [[0, 1, 2]])


def two_faces():
    return _mesh([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.1, 0.1, 0.03]], [[0, 1, 2], [1, 3, 2]])


def islands():
    """fan(12) among isolated vertices: 40 before it, 7 behind it."""
    verts, faces = fan(12)
    rng = np.random.default_rng(13)
    return _mesh(np.vstack([rng.normal(0.0, 1.0, (40, 3)), verts, rng.normal(0.0, 1.0, (7, 3))]), faces + 40)


def sphere_field(dim, centre, radius):
    """float32 [dim][dim][dim]: the distance to a sphere in voxel units over a truncation of 2.5 voxels, clipped to [-1, 1]."""
    x, y, z = np.meshgrid(*[np.arange(dim, dtype=np.float64)] * 3, indexing="ij")
    sd = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(sd / 2.5, -1.0, 1.0).astype(np.float32)


MC_DIM, MC_VOXEL = 24, 0.125
MC_SPHERES = {"closed": ((11.63, 11.29, 12.37), 6.3), "open": ((3.3, 11.29, 12.37), 6.3)}  # the second pokes through the wall x = 0


CASES = {
    "tetrahedron": tetrahedron, "pillow": pillow, "torus_3x3": torus_3x3, "icosphere_2": lambda: icosphere(2), "icosphere_3": lambda: icosphere(3),
    "torus_16x8": lambda: torus(16, 8), "spindle_22": lambda: spindle(22), "spindle_23": lambda: spindle(23), "spindle_24": lambda: spindle(24), "spindle_25": lambda: spindle(25),
    "spindle_40": lambda: spindle(40), "flat_spindle_23": lambda: spindle(23, 0.001), "fan_25": lambda: fan(25), "fan_12": lambda: fan(12), "book_3": lambda: book(3), "book_2": lambda: book(2),
    "flag": flag,
    "tilted_plane": lambda: tilted_plane(12), "degenerate": lambda: degenerate(12), "scaled_1e-20": lambda: scaled(12, 1e-20),
    "scaled_1e25": lambda: scaled(12, 1e25), "wide_lattice": lambda: wide_lattice(200),
}


@functools.lru_cache(maxsize=None)
def case(name):
    verts, faces = CASES[name]()
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


# ---- the restatement, cached and shared ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(name, budget, max_error, max_rounds=D.MAX_ROUNDS):
    """(faces, kept, stats, trace) of the restatement on a named case; a run that hits ``max_rounds`` returns (None, None, None, the trace so far)."""
    verts, faces = case(name)
    trace = []
    try:
        f, kept, stats = D.decimate(verts, faces, budget, max_error, max_rounds=max_rounds, trace=trace)
    except D.DecimationStateError:
        return None, None, None, trace
    return f, kept, stats, trace


def removes(live_faces, applied):
    """Faces each applied collapse (v0, v1) removes: the live faces that contain both."""
    f = np.asarray(live_faces)
    return np.array([int(((f == v0).any(1) & (f == v1).any(1)).sum()) for v0, v1 in applied], np.int64)


def rule_census(vertices, faces, budget, max_error):
    """{rule name: halfedges it rejects first}, summed over every round of ``decimate`` -- the round in which nothing is selected included -- with the
    legal halfedges under ``None``.  Each round is judged on its own mesh and quadrics, as ``decimate`` judges it."""
    pos = np.asarray(vertices, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    trace = []
    out, kept, _ = D.decimate(pos, faces, budget, max_error, trace=trace)
    census = {}
    if len(faces) <= budget:
        return census
    q = D.vertex_quadrics(pos, faces)
    locked = D.locked_vertices(len(pos), faces)

    def count(live):
        m = D._Mesh(live, np.ones(len(live), bool))
        for v0 in m.vf:
            for v1 in m.nbrs(v0):
                rule = D.collapse_check(m, q, pos, locked, v0, v1, max_error)[0]
                census[rule] = census.get(rule, 0) + 1
    for _, applied, live in trace:
        count(live)
        for v0, v1 in applied:
            q[v1] = q[v1] + q[v0]
    if len(out) > budget:  # the rounds ended because a round selected nothing: that round looked at the final mesh
        count(np.asarray(kept)[out])
    return census


def face_counts(live_faces, n_vertices):
    return np.bincount(np.asarray(live_faces).ravel(), minlength=n_vertices)


# ---- budgets that the cases bring along -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_rounds():
    """The first two rounds of wide_lattice(200), neither cut short: [(F at round start, applied in key order, cumulative faces removed)]."""
    trace = restated("wide_lattice", 0, 1e9, 2)[3]
    assert len(trace) == 2
    return [(f_cur, applied, np.cumsum(removes(live, applied))) for f_cur, applied, live in trace]


@functools.lru_cache(maxsize=None)
def wide_budgets():
    """{name: (budget, rounds, collapses applied in the last round)}: (a) round one cut after more than 1024 keys, (b) cut before the 1024th key,
    (c) all of round one, then round two cut in its middle.  Read from the uncut rounds, the cut being the first key whose prefix removes enough."""
    (f1, applied1, cum1), (f2, applied2, cum2) = wide_rounds()
    ia = (THRESH_THREADS + len(applied1)) // 2  # index of the last key applied
    ib = THRESH_THREADS // 2 - 1
    ic = len(applied2) // 2
    return {"a": (int(f1 - cum1[ia]), 1, ia + 1), "b": (int(f1 - cum1[ib]), 1, ib + 1), "c": (int(f2 - cum2[ic]), 2, ic + 1)}


# budgets for which the restatement runs exactly 16, 17 and 32 rounds (DEC_BATCH = 16 rounds are issued between two polls), found by scanning every
# budget of the mesh with the restatement; tests/test_decimate_cases_cpu.py asserts the counts
BATCH_CASE = "icosphere_2"
BATCH_BUDGETS = {15: 224, 16: 218, 17: 212, 32: 136, 33: 134}  # rounds -> budget


def spindle_high_budget(k):
    """The ring loses two vertices and no more: both apexes keep k - 2 faces."""
    return 2 * k - 4


def own_budgets(name):
    """The budgets a case adds to 1, F // 2, F - 1."""
    if name == "wide_lattice":
        return [b for b, _, _ in wide_budgets().values()]
    if name == BATCH_CASE:
        return sorted(BATCH_BUDGETS.values())
    if name in ("spindle_25", "spindle_40"):
        return [spindle_high_budget(int(name[8:]))]
    return []


def max_errors(name):
    """1e9 and 1e-6; inf too where costs are infinite in float32 (scaled_1e25) or NaN (degenerate: NaN is not below inf either)."""
    return (1e9, 1e-6, float("inf")) if name in ("scaled_1e25", "degenerate") else (1e9, 1e-6)


def runs():
    """[(case, budget, max_error)] that the restatement and the kernel are compared on: budgets 1, F // 2, F - 1 and the case's own.  The wide lattice
    names its own budgets ("a", "b", "c": finding them takes rounds of the restatement, which a test does and the collection of tests does not);
    ``budget_of`` turns a name into the number.  Restating the wide lattice to F // 2 takes about 70 s and to budget 1 about 150 s per max_error."""
    out = []
    for name in CASES:
        n_faces = len(case(name)[1])
        budgets = sorted({1, n_faces // 2, n_faces - 1} | (set() if name == "wide_lattice" else set(own_budgets(name))))
        budgets += list("abc") if name == "wide_lattice" else []
        out += [(name, budget, max_error) for budget in budgets for max_error in max_errors(name)]
    return out


def budget_of(name, budget):
    return wide_budgets()[budget][0] if isinstance(budget, str) else budget


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------------------
def gpu_decimate(ctx, verts, faces, budget, max_error, on_device):
    """hive_mesh_decimate directly: (faces, kept vertex ids, stats)."""
    from hive_amd._lib import MEM_DEVICE, MEM_HOST, ptr
    v = np.ascontiguousarray(verts, np.float64)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nf, nv = ctypes.c_int64(0), ctypes.c_int64(0)
    stats = np.zeros(3, np.int64)
    if on_device:
        import torch
        dv, df = torch.from_numpy(np.array(v)).cuda(), torch.from_numpy(np.array(f)).cuda()  # (copies: a cached case is read-only)
        of, ovi = torch.empty((len(f), 3), dtype=torch.int32, device="cuda"), torch.empty(len(v), dtype=torch.int32, device="cuda")
        ctx.follow_torch_stream()
        ctx.check(ctx.lib.hive_mesh_decimate(ctx.handle, ptr(dv), len(v), ptr(df), len(f), budget, max_error, MEM_DEVICE, ptr(of), ptr(ovi), ctypes.byref(nf),
                                             ctypes.byref(nv), ptr(stats)))
        return of[:nf.value].cpu().numpy(), ovi[:nv.value].cpu().numpy(), tuple(stats.tolist())
    of, ovi = np.empty((len(f), 3), np.int32), np.empty(len(v), np.int32)
    ctx.check(ctx.lib.hive_mesh_decimate(ctx.handle, ptr(v), len(v), ptr(f), len(f), budget, max_error, MEM_HOST, ptr(of), ptr(ovi), ctypes.byref(nf),
                                         ctypes.byref(nv), ptr(stats)))
    return of[:nf.value], ovi[:nv.value], tuple(stats.tolist())


def assert_same(got, want):
    assert got[2] == want[2], (got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
