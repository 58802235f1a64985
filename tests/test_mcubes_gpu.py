"""Marching cubes on the GPU (`hive_tsdf_extract_mesh`, csrc/mcubes.hip) against the C oracle, at the tails, sizes and edges where
its bit-sliced passes can go wrong: every ragged last sign word (Z = 1, 31, 33, 63, 65, 97), axes of length 1 and 2, both sign kernels
(the 16-byte vector path and the per-word path that ragged rows and unaligned storage take), the block scan with several counts per
thread, exact zeros / negative zeros / denormals, .5 ties in the colour lookup, the benchmark's 512^3 room and config 4's 1024^3 volume.

Every volume has the bounds [0, d * 0.125] per axis at 0.125 voxels, so its dims are d exactly, and colours are random 24-bit integers,
so that a wrong colour index shows.  Faces, vertices (world and voxel coordinates), colours and normals must equal the oracle's bit for
bit.  The oracle is serial; at 1024^3 a vectorised numpy restatement of it (`restate_mesh`, proven equal to it on the sweep below)
stands in.  Topology (closed manifold, Euler characteristic, winding, components) is checked on the GPU mesh itself.
"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = 0.125
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_BLOCK = 256  # lanes (= sign words) per block of the count / verts / faces passes
EMPTY = "Surface level must be within volume data range."


def _table(hdr, name):
    body = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", hdr, re.S).group(1)
    return np.array([int(v) for v in re.findall(r"\d+", body)], np.int64)


_HDR = open(os.path.join(ROOT, "include", "hive_mc_tables.h")).read()
NUM_TRIS = _table(_HDR, "HIVE_MC_NUM_TRIS")
TRI_TABLE = _table(_HDR, "HIVE_MC_TRI_TABLE").reshape(256, 15)
EDGE_OWNER = _table(_HDR, "HIVE_MC_EDGE_OWNER").reshape(12, 4)
CORNER_OFFSET = _table(_HDR, "HIVE_MC_CORNER_OFFSET").reshape(8, 3)
assert NUM_TRIS.shape == (256,)


# ---- scalar fields (float32 [X][Y][Z], voxel units) ------------------------------------------------------------------------

def _coords(dims):
    return np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")


def _clip(sd, trunc=2.5):
    return np.clip(sd / trunc, -1.0, 1.0).astype(np.float32)


def sphere(dims, centre=None, radius=None):
    """Clipped signed distance of a sphere, centre off-grid (test_oracle_cpu._sphere_volume's field)."""
    d = np.array(dims, np.float64)
    c = d * 0.47 + np.array([0.13, -0.21, 0.37]) if centre is None else np.asarray(centre, np.float64)
    r = max(0.3 * d.max(), 1.3) if radius is None else radius
    X, Y, Z = _coords(dims)
    return _clip(np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r)


def cut_sphere_params(dims):
    """A sphere centred in the volume whose radius lies between the largest half-extent and the half-diagonal: it crosses all six faces."""
    h = (np.array(dims, np.float64) - 1) / 2
    return h + np.array([0.11, -0.07, 0.05]), h.max() + 0.5 * (np.linalg.norm(h) - h.max())


def cut_sphere(dims):
    c, r = cut_sphere_params(dims)
    return sphere(dims, c, r)


def torus(dims, major=None, minor=None):
    d = np.array(dims, np.float64)
    c = d / 2 + np.array([0.21, -0.17, 0.09])
    R = 0.25 * d[:2].min() if major is None else major
    r = 0.4 * R if minor is None else minor
    X, Y, Z = _coords(dims)
    q = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - R
    return _clip(np.sqrt(q ** 2 + (Z - c[2]) ** 2) - r)


def two_spheres(dims):
    d = np.array(dims, np.float64)
    r = 0.15 * d.min()
    a = sphere(dims, d * np.array([0.28, 0.5, 0.5]) + 0.13, r)
    b = sphere(dims, d * np.array([0.72, 0.5, 0.5]) - 0.21, r)
    return np.minimum(a, b)


def random_signs(dims, seed=0):
    """I.i.d. signs of density 0.5, magnitudes in [0.05, 1]."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.05, 1.0, dims)
    return np.where(rng.random(dims) < 0.5, -mag, mag).astype(np.float32)


def checkerboard(dims):
    """+1 / -1 by the parity of x + y + z: every edge crosses at t = 0.5, so every colour lookup is a rounding tie."""
    X, Y, Z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    return np.where((X + Y + Z) % 2 == 0, 1.0, -1.0).astype(np.float32)


def zeros_and_denormals(dims, seed=0):
    """Random signs with ~10 % +0.0, ~5 % -0.0 and a few +-1e-40 (float32 denormals): the sign test is tsdf < 0."""
    t = random_signs(dims, seed)
    rng = np.random.default_rng(seed + 100)
    u = rng.random(dims)
    t[u < 0.10] = 0.0
    t[(u >= 0.10) & (u < 0.15)] = -0.0
    flat = t.reshape(-1)
    k = max(2, flat.size // 200)
    idx = rng.choice(flat.size, size=min(2 * k, flat.size), replace=False)
    flat[idx[:len(idx) // 2]] = np.float32(1e-40)
    flat[idx[len(idx) // 2:]] = np.float32(-1e-40)
    return t


FIELDS = {"sphere": sphere, "cut_sphere": cut_sphere, "random": random_signs, "checker": checkerboard, "zeros": zeros_and_denormals}
SWEEP_DIMS = [(1, 5, 7), (5, 1, 33), (3, 4, 1), (2, 2, 2), (7, 9, 31), (7, 9, 32), (7, 9, 33), (5, 6, 63), (5, 6, 64), (5, 6, 65),
              (4, 3, 97), (17, 13, 96), (64, 64, 64)]


def colours(dims, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 24, dims).astype(np.float32)


# ---- volumes -------------------------------------------------------------------------------------------------------------

def bounds(dims):
    return np.array([[0.0, d * VS] for d in dims])


def gpu_volume(ctx, dims, tsdf, color, storage=None):
    from hive_amd import fusion
    vol = fusion.TSDFVolume(bounds(dims), VS, ctx=ctx, storage=storage)
    assert tuple(int(d) for d in vol.vol_dim) == tuple(dims)
    vol.set_volume(tsdf, color, np.ones(dims, np.float32))
    return vol


def oracle_volume(oracle_lib, dims, tsdf, color):
    ora = oracle_lib.TSDFVolume(bounds(dims), VS)
    assert tuple(int(d) for d in ora._vol_dim) == tuple(dims)
    ora._tsdf = np.ascontiguousarray(tsdf, np.float32)
    ora._color = np.ascontiguousarray(color, np.float32)
    return ora


def mesh_or_empty(obj):
    """get_mesh(return_voxel_coords=True), or None when it raises the empty-volume ValueError."""
    try:
        return obj.get_mesh(return_voxel_coords=True)
    except ValueError as e:
        assert str(e) == EMPTY
        return None


def copy_mesh(vol, nv, nf):
    """The copy half of fusion.TSDFVolume.get_mesh (no extraction): what the last hive_tsdf_extract_mesh of `vol` left."""
    from hive_amd._lib import ptr
    verts, faces = np.empty((nv, 3), np.float32), np.empty((nf, 3), np.int32)
    norms, cols, vvox = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.uint8), np.empty((nv, 3), np.float32)
    vol._ctx.check(vol._ctx.lib.hive_tsdf_copy_mesh(vol._handle, ptr(verts), ptr(faces), ptr(norms), ptr(cols)))
    vol._ctx.check(vol._ctx.lib.hive_tsdf_copy_mesh_voxel_coords(vol._handle, ptr(vvox)))
    return verts, faces, norms, cols, vvox


def assert_mesh_equal(got, want, what=""):
    """faces, world vertices, colours, voxel-coordinate vertices and normals: all bit-exact."""
    if want is None:
        assert got is None, f"{what}: the oracle finds no surface, the GPU does"
        return
    assert got is not None, f"{what}: the GPU finds no surface, the oracle does"
    v, f, n, c, vv = got
    ov, of, on, oc, ovv = want
    assert v.shape == ov.shape and f.shape == of.shape, f"{what}: {len(v)} / {len(f)} vertices / faces vs oracle {len(ov)} / {len(of)}"
    assert np.array_equal(f, of), f"{what}: faces differ"
    assert np.array_equal(vv, ovv), f"{what}: voxel-coordinate vertices differ"
    assert np.array_equal(v, ov), f"{what}: world vertices differ"
    assert np.array_equal(c, oc), f"{what}: colours differ at {np.flatnonzero((c != oc).any(axis=1))[:8]}"
    assert np.array_equal(n, on), f"{what}: normals differ (max {np.abs(n - on).max():.3g})"


def has_sign_change(t):
    s = t < 0
    return bool(s.any() and not s.all())


def has_crossing_edge(t):
    s = t < 0
    return any(bool((np.diff(s, axis=a)).any()) for a in range(3) if s.shape[a] > 1)


# ---- numpy restatement of oracle_marching_cubes ----------------------------------------------------------------------------

def _grad_axis(flat, dims, p, r):
    """grad_axis of hive_oracle.c for points p = (x, y, z) int64 arrays: central difference, one-sided at the borders."""
    lo, hi = list(p), list(p)
    lo[r] = p[r] - (p[r] > 0)
    hi[r] = p[r] + (p[r] < dims[r] - 1)
    _, Y, Z = dims
    a = flat[(hi[0] * Y + hi[1]) * Z + hi[2]]
    b = flat[(lo[0] * Y + lo[1]) * Z + lo[2]]
    span = (hi[r] - lo[r]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(span > 0, (a - b) / span, np.float32(0)).astype(np.float32)


def restate_mesh(tsdf, color, origin, voxel_size, slab=32):
    """oracle_marching_cubes restated with numpy, one x-slab at a time.  Vertices: the sign-changing grid edges in (voxel index, axis)
    order; faces: the active cells in index order, each expanded by NUM_TRIS[case], their TRI_TABLE edges mapped through EDGE_OWNER to
    (owner voxel, axis) keys and found among the vertex keys with searchsorted.  float32 throughout, in the oracle's operation order."""
    dims = tuple(int(d) for d in tsdf.shape)
    X, Y, Z = dims
    flat = tsdf.reshape(-1)
    vkeys, fkeys = [], []
    for x0 in range(0, X, slab):
        x1 = min(x0 + slab, X)
        t = tsdf[x0:min(x1 + 1, X)]
        s = t < 0
        if not s.any() or s.all():
            continue
        n_own = x1 - x0
        e = np.zeros((n_own, Y, Z, 3), bool)
        m = s.shape[0] - 1 if x1 == X else n_own
        e[:m, :, :, 0] = s[:m] != s[1:m + 1]
        e[:, :-1, :, 1] = s[:n_own, :-1] != s[:n_own, 1:]
        e[:, :, :-1, 2] = s[:n_own, :, :-1] != s[:n_own, :, 1:]
        vkeys.append(np.flatnonzero(e.reshape(-1)) + 3 * x0 * Y * Z)
        del e
        nc = min(x1, X - 1) - x0
        if nc <= 0 or Y < 2 or Z < 2:
            continue
        cs = np.zeros((nc, Y - 1, Z - 1), np.uint8)
        for c, (dx, dy, dz) in enumerate(CORNER_OFFSET):
            cs |= s[dx:dx + nc, dy:dy + Y - 1, dz:dz + Z - 1].astype(np.uint8) << np.uint8(c)
        ix, iy, iz = np.nonzero(NUM_TRIS[cs] > 0)
        case = cs[ix, iy, iz].astype(np.int64)
        idx = ((ix + x0) * Y + iy) * Z + iz
        nt = NUM_TRIS[case]
        first = np.repeat(np.cumsum(nt) - nt, nt)
        k = np.arange(int(nt.sum())) - first
        case, idx = np.repeat(case, nt), np.repeat(idx, nt)
        keys = np.empty((len(k), 3), np.int64)
        for j in range(3):
            ed = TRI_TABLE[case, 3 * k + j]
            ow = EDGE_OWNER[ed]
            keys[:, j] = 3 * (idx + (ow[:, 0] * Y + ow[:, 1]) * Z + ow[:, 2]) + ow[:, 3]
        fkeys.append(keys)
    if not vkeys or sum(len(k) for k in vkeys) == 0:
        raise ValueError(EMPTY)
    keys = np.concatenate(vkeys)
    fk = np.concatenate(fkeys) if fkeys else np.zeros((0, 3), np.int64)
    faces = np.searchsorted(keys, fk).astype(np.int64)
    assert (faces < len(keys)).all() and np.array_equal(keys[np.minimum(faces, len(keys) - 1)], fk), "a face edge owns no vertex"
    faces = faces.astype(np.int32)
    idx, a = keys // 3, keys % 3
    p = [idx // (Y * Z), (idx // Z) % Y, idx % Z]
    stride = np.array([Y * Z, Z, 1], np.int64)
    v0 = flat[idx]
    v1 = flat[idx + stride[a]]
    t = v0 / (v0 - v1)
    pos = np.stack(p, axis=1).astype(np.float32)
    rows = np.arange(len(keys))
    pos[rows, a] = pos[rows, a] + t
    verts = pos * np.float32(voxel_size) + np.asarray(origin, np.float32)
    q = [c.copy() for c in p]
    for r in range(3):
        q[r] = q[r] + (a == r)
    g = []
    for r in range(3):
        g0 = _grad_axis(flat, dims, p, r)
        g1 = _grad_axis(flat, dims, q, r)
        g.append(g0 + t * (g1 - g0))
    ln = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        norms = np.stack([np.where(ln > 0, gr / ln, np.float32(0)) for gr in g], axis=1).astype(np.float32)
    ci = np.minimum(np.rint(pos).astype(np.int64), np.array(dims, np.int64) - 1)
    c = color.reshape(-1)[(ci[:, 0] * Y + ci[:, 1]) * Z + ci[:, 2]]
    cb = np.floor(c / np.float32(65536))
    cg = np.floor((c - cb * np.float32(65536)) / np.float32(256))
    cr = c - cb * np.float32(65536) - cg * np.float32(256)
    cols = np.stack([cr, cg, cb], axis=1).astype(np.uint8)
    return verts, faces, norms, cols, pos


# ---- topology of a mesh --------------------------------------------------------------------------------------------------

def edge_counts(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def euler(verts, faces):
    uniq, _ = edge_counts(faces)
    return len(verts) - len(uniq) + len(faces)


def components(n_verts, faces):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]]])
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n_verts, n_verts))
    return connected_components(g, directed=False)[0]


def outward(vvox, faces, centre):
    tri = vvox[faces].astype(np.float64)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return (fn * (tri.mean(axis=1) - centre)).sum(axis=1)


# ---- tests ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("dims", SWEEP_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_dims_sweep_bit_exact(gpu_ctx, oracle_lib, dims, field):
    """Every ragged last word, thin volumes (axes of 1 and 2), both sign kernels' shapes: the GPU mesh is the oracle's, bit for bit."""
    tsdf, color = FIELDS[field](dims), colours(dims)
    if field == "cut_sphere" and min(dims) >= 4:  # premise: the surface crosses all six faces of the volume
        for a in range(3):
            for end in (0, -1):
                assert has_sign_change(np.take(tsdf, end, axis=a)), (a, end)
    if field == "random" and np.prod(np.array(dims) - 1) >= 10000:
        cs = np.zeros(tuple(d - 1 for d in dims), np.int64)
        for c, (dx, dy, dz) in enumerate(CORNER_OFFSET):
            cs |= (tsdf[dx:dx + dims[0] - 1, dy:dy + dims[1] - 1, dz:dz + dims[2] - 1] < 0).astype(np.int64) << c
        assert len(np.unique(cs)) == 256, "all 256 cube cases occur"
    vol = gpu_volume(gpu_ctx, dims, tsdf, color)
    want = mesh_or_empty(oracle_volume(oracle_lib, dims, tsdf, color))
    got = mesh_or_empty(vol)
    assert (want is None) == (not has_crossing_edge(tsdf)), "an empty mesh iff no grid edge changes sign"
    assert_mesh_equal(got, want, f"{field} {dims}")
    if want is not None:
        if min(dims) == 1:
            assert got[1].shape == (0, 3), "a volume with an axis of 1 has edges but no cells"
        if field == "checker":
            X, Y, Z = dims
            assert NUM_TRIS[0b01011010] == NUM_TRIS[0b10100101]
            assert len(got[0]) == (X - 1) * Y * Z + X * (Y - 1) * Z + X * Y * (Z - 1)
            assert len(got[1]) == (X - 1) * (Y - 1) * (Z - 1) * NUM_TRIS[0b01011010]
            assert (got[4] % 1 == 0.5).sum(axis=1).tolist() == [1] * len(got[4]), "every vertex is an edge midpoint (a tie)"
    vol.close()


@pytest.mark.parametrize("dims", [(1, 5, 7), (7, 9, 33), (64, 64, 64)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("value", [1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40])
def test_no_sign_change_raises(gpu_ctx, oracle_lib, dims, value):
    """A constant volume has no surface: the oracle and the GPU raise scikit-image's ValueError (-0.0 is not negative; -1e-40 is)."""
    tsdf = np.full(dims, value, np.float32)
    for obj in (gpu_volume(gpu_ctx, dims, tsdf, colours(dims)), oracle_volume(oracle_lib, dims, tsdf, colours(dims))):
        with pytest.raises(ValueError, match=EMPTY):
            obj.get_mesh()


@pytest.mark.parametrize("field", ["random", "zeros", "checker", "cut_sphere"])
@pytest.mark.parametrize("dims", [d for d in SWEEP_DIMS if d[2] % 32 == 0], ids=lambda d: "x".join(map(str, d)))
def test_both_sign_kernels(gpu_ctx, oracle_lib, dims, field):
    """Z % 32 == 0: library-owned (16-byte aligned) storage takes mc_signs_vec_kernel; caller-owned storage at element offset 1 of a
    larger tensor is not 16-byte aligned and takes mc_signs_row_kernel.  Both are the oracle's mesh."""
    import torch
    tsdf, color = FIELDS[field](dims), colours(dims)
    n = int(np.prod(dims))
    want = mesh_or_empty(oracle_volume(oracle_lib, dims, tsdf, color))
    own = gpu_volume(gpu_ctx, dims, tsdf, color)
    assert own.device_ptrs()[0] % 16 == 0
    big = [torch.zeros(n + 5, dtype=torch.float32, device="cuda") for _ in range(3)]
    views = tuple(b[1:1 + n] for b in big)
    caller = gpu_volume(gpu_ctx, dims, tsdf, color, storage=views)
    assert caller.device_ptrs()[0] == views[0].data_ptr() and views[0].data_ptr() % 16 == 4
    a, b = mesh_or_empty(own), mesh_or_empty(caller)
    assert_mesh_equal(a, want, f"aligned {field} {dims}")
    assert_mesh_equal(b, want, f"unaligned {field} {dims}")
    assert torch.equal(big[0][0], torch.zeros((), device="cuda")) and torch.equal(big[0][n + 1:], torch.zeros(4, device="cuda"))
    own.close()
    caller.close()


@pytest.mark.parametrize("dims,field", [((300, 301, 70), "random"), ((257, 257, 257), "torus")], ids=["300x301x70", "257cubed"])
def test_multi_chunk_block_scan(gpu_ctx, oracle_lib, dims, field):
    """scan_counts_kernel gives each of its 1024 threads ceil(nb / 1024) block counts; here nb > 1024 and the last chunk is ragged."""
    X, Y, Z = dims
    nb = (X * Y * ((Z + 31) // 32) + MC_BLOCK - 1) // MC_BLOCK
    assert nb > 1024 and nb % 1024 != 0 and nb == {"random": 1059, "torus": 2323}[field]
    tsdf = random_signs(dims, seed=3) if field == "random" else torus(dims)
    color = colours(dims)
    vol = gpu_volume(gpu_ctx, dims, tsdf, color)
    got = mesh_or_empty(vol)
    want = mesh_or_empty(oracle_volume(oracle_lib, dims, tsdf, color))
    assert want is not None
    assert_mesh_equal(got, want, f"{field} {dims}")
    vol.close()


@pytest.mark.parametrize("dims", SWEEP_DIMS + [(300, 301, 70)], ids=lambda d: "x".join(map(str, d)))
def test_restatement_matches_oracle(oracle_lib, dims):
    """The numpy restatement used at 1024^3 is the C oracle, bit for bit, over the sweep (every field) and a multi-slab volume."""
    color = colours(dims)
    for name, make in FIELDS.items():
        tsdf = make(dims)
        ora = oracle_volume(oracle_lib, dims, tsdf, color)
        want = mesh_or_empty(ora)
        try:
            got = restate_mesh(tsdf, color, ora._vol_origin, VS, slab=7)
        except ValueError as e:
            assert str(e) == EMPTY
            got = None
        assert_mesh_equal(got, want, f"restatement {name} {dims}")


def test_benchmark_room_512(gpu_ctx, oracle_lib):
    """bench.py's mesh line: the synthetic room integrated into 512^3 at 1 cm voxels.  The GPU mesh of the GPU volume is the oracle's."""
    from hive_amd import fusion, synthetic
    seq = synthetic.make_sequence(num_frames=3, yaw_step_deg=40.0)
    vol = fusion.TSDFVolume(synthetic.room_bounds(), 0.01, ctx=gpu_ctx)
    assert tuple(vol.vol_dim) == (512, 512, 512)
    vol.integrate_batch(seq["color"], seq["depth"], seq["K"], seq["poses"])
    got = vol.get_mesh(return_voxel_coords=True)
    tsdf, color = vol.get_volume()
    ora = oracle_lib.TSDFVolume(synthetic.room_bounds(), 0.01)
    ora._tsdf, ora._color = tsdf, color
    want = ora.get_mesh(return_voxel_coords=True)
    assert len(want[0]) > 100000
    assert_mesh_equal(got, want, "room 512^3")
    vol.close()


def test_config4_volume_1024(gpu_ctx):
    """1024^3 (BASELINE config 4's volume): 2^30 voxels, so the tsdf and vbase arrays are 2^32 bytes and surface voxels sit at byte
    offsets past 2^31; the block scan runs 131072 counts.  Compared with the numpy restatement of the oracle."""
    import torch
    from hive_amd import fusion
    dims = (1024, 1024, 1024)
    n = int(np.prod(dims))
    nb = (n // 32 + MC_BLOCK - 1) // MC_BLOCK
    assert n == 1 << 30 and nb == 131072
    centre, radius = (640.3, 511.6, 500.9), 330.0
    assert 4 * (int(centre[0] + radius) * 1024 * 1024) > 1 << 31
    dev = "cuda"
    ar = torch.arange(1024, device=dev, dtype=torch.float32)
    d2 = ((ar - centre[0]) ** 2).view(-1, 1, 1) + ((ar - centre[1]) ** 2).view(1, -1, 1) + ((ar - centre[2]) ** 2).view(1, 1, -1)
    t_dev = ((d2.sqrt_() - radius) / 2.5).clamp_(-1.0, 1.0).reshape(-1)
    del d2
    gen = torch.Generator(device=dev).manual_seed(4)
    c_dev = torch.randint(0, 1 << 24, (n,), device=dev, dtype=torch.int32, generator=gen).to(torch.float32)
    vol = fusion.TSDFVolume(bounds(dims), VS, ctx=gpu_ctx)
    assert tuple(int(d) for d in vol.vol_dim) == dims
    vol.set_volume_device(t_dev, c_dev, None)
    got = vol.get_mesh(return_voxel_coords=True)
    origin = vol._vol_origin.copy()
    vol.close()
    tsdf = t_dev.cpu().numpy().reshape(dims)
    color = c_dev.cpu().numpy().reshape(dims)
    del t_dev, c_dev, vol
    torch.cuda.empty_cache()
    want = restate_mesh(tsdf, color, origin, VS)
    assert len(want[0]) > 1_000_000 and want[4][:, 0].max() > 512
    assert_mesh_equal(got, want, "sphere 1024^3")
    del tsdf, color, got, want


def test_topology_sphere(gpu_ctx):
    dims = (48, 50, 47)
    d = np.array(dims, np.float64)
    centre, radius = d * 0.47 + np.array([0.13, -0.21, 0.37]), 15.3
    vol = gpu_volume(gpu_ctx, dims, sphere(dims, centre, radius), colours(dims))
    verts, faces, norms, _, vvox = vol.get_mesh(return_voxel_coords=True)
    _, counts = edge_counts(faces)
    assert (counts == 2).all(), "every edge of a closed surface is in exactly two faces"
    assert euler(verts, faces) == 2
    assert (outward(vvox, faces, centre) > 0).all(), "faces are wound outward"
    assert ((norms * (vvox - centre)).sum(axis=1) > 0).all()
    vol.close()


def test_topology_torus(gpu_ctx):
    dims = (56, 52, 33)
    vol = gpu_volume(gpu_ctx, dims, torus(dims, 13.0, 5.2), colours(dims))
    verts, faces, _, _, _ = vol.get_mesh(return_voxel_coords=True)
    _, counts = edge_counts(faces)
    assert (counts == 2).all()
    assert euler(verts, faces) == 0
    assert components(len(verts), faces) == 1
    vol.close()


def test_topology_two_spheres(gpu_ctx):
    dims = (70, 40, 38)
    vol = gpu_volume(gpu_ctx, dims, two_spheres(dims), colours(dims))
    verts, faces, _, _, _ = vol.get_mesh(return_voxel_coords=True)
    _, counts = edge_counts(faces)
    assert (counts == 2).all()
    assert euler(verts, faces) == 4
    assert components(len(verts), faces) == 2
    vol.close()


def test_topology_boundary_cut_sphere(gpu_ctx):
    """The surface is open where the volume cuts it: every edge in one face only lies on one of the six outer faces, and each outer face
    holds such edges; no edge is in more than two faces."""
    dims = (40, 44, 49)
    vol = gpu_volume(gpu_ctx, dims, cut_sphere(dims), colours(dims))
    verts, faces, _, _, vvox = vol.get_mesh(return_voxel_coords=True)
    uniq, counts = edge_counts(faces)
    assert counts.max() == 2
    border = uniq[counts == 1]
    a, b = vvox[border[:, 0]], vvox[border[:, 1]]
    on_face = np.zeros((len(border), 6), bool)
    for ax in range(3):
        on_face[:, 2 * ax] = (a[:, ax] == 0) & (b[:, ax] == 0)
        on_face[:, 2 * ax + 1] = (a[:, ax] == dims[ax] - 1) & (b[:, ax] == dims[ax] - 1)
    assert on_face.any(axis=1).all(), "an open edge inside the volume"
    assert on_face.any(axis=0).all(), "the surface crosses all six faces"
    vol.close()


def test_repeated_extraction_one_volume(gpu_ctx, oracle_lib):
    """Small, large (buffers grow), small (reused), empty (ValueError, and again: no stale mesh), larger again; twice in a row is
    bit-identical."""
    from hive_amd import _lib
    from hive_amd._lib import ptr
    dims = (64, 64, 64)
    color = colours(dims)
    vol = gpu_volume(gpu_ctx, dims, sphere(dims, radius=5.2), color)
    steps = [("small", sphere(dims, radius=5.2)), ("large", random_signs(dims, 5)), ("small again", sphere(dims, radius=7.9)),
             ("empty", np.ones(dims, np.float32)), ("larger", checkerboard(dims))]
    sizes = []
    for name, tsdf in steps:
        vol.set_volume(tsdf, color)
        want = mesh_or_empty(oracle_volume(oracle_lib, dims, tsdf, color))
        if want is None:
            for _ in range(2):
                with pytest.raises(ValueError, match=EMPTY):
                    vol.get_mesh()
            rc = vol._ctx.lib.hive_tsdf_copy_mesh(vol._handle, ptr(np.empty((1, 3), np.float32)), None, None, None)
            assert rc == _lib.ERR_STATE, "no mesh to copy after an empty extraction"
            continue
        got = vol.get_mesh(return_voxel_coords=True)
        assert_mesh_equal(got, want, name)
        assert_mesh_equal(vol.get_mesh(return_voxel_coords=True), got, f"{name}, second extraction")
        sizes.append(len(want[0]))
    assert sizes[0] < sizes[1] > sizes[2] and sizes[3] > sizes[1]
    vol.close()


def test_two_volumes_share_one_context(oracle_lib):
    """A is extracted, then a larger B on the same context grows the shared sign scratch; A's mesh, copied afterwards, is still A's."""
    from hive_amd import _lib
    ctx = _lib.Context(0)
    da, db = (17, 13, 96), (96, 97, 98)
    ta, tb = random_signs(da, 7), torus(db)
    ca, cb = colours(da, 2), colours(db, 3)
    a = b = None
    try:  # the volumes go before their context, also when an assertion fails
        a, b = gpu_volume(ctx, da, ta, ca), gpu_volume(ctx, db, tb, cb)
        nv, nf = a._extract()
        b_mesh = b.get_mesh(return_voxel_coords=True)
        got_a = copy_mesh(a, nv, nf)
        assert_mesh_equal(got_a, oracle_volume(oracle_lib, da, ta, ca).get_mesh(return_voxel_coords=True), "A after B")
        assert_mesh_equal(b_mesh, oracle_volume(oracle_lib, db, tb, cb).get_mesh(return_voxel_coords=True), "B")
    finally:
        for v in (a, b):
            if v is not None:
                v.close()
        ctx.close()


def test_stream_order(gpu_ctx, oracle_lib):
    """A field written with set_volume_device on a side stream, behind other work on that stream, and extracted under the same stream:
    the mesh is the new field's."""
    import torch
    dims = (64, 64, 64)
    color = colours(dims)
    vol = gpu_volume(gpu_ctx, dims, sphere(dims), color)
    new = random_signs(dims, 9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            m = torch.randn(2048, 2048, device="cuda")
            for _ in range(8):
                m = (m @ m).clamp_(-1, 1)
            t = torch.from_numpy(new.reshape(-1)).to("cuda") + m[0, 0] * 0
            c = torch.from_numpy(color.reshape(-1)).to("cuda")
            vol.set_volume_device(t, c, None)
            got = vol.get_mesh(return_voxel_coords=True)
    finally:
        torch.cuda.synchronize()
        gpu_ctx.follow_torch_stream()  # back on the default stream for the tests after this one
    assert_mesh_equal(got, oracle_volume(oracle_lib, dims, new, color).get_mesh(return_voxel_coords=True), "side stream")
    vol.close()
