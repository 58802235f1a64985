"""hive_mesh_decimate (csrc/decimate.hip) against the restatement of its rounds (tests/decimate_restatement.py), bit for bit, on the meshes of
tests/decimate_cases.py -- closed surfaces of genus 0 and 1, two faces on one vertex triple, edges with three faces, fans on either side of the face cap,
costs of either sign, of float32 infinity and NaN, areas below FLT_MIN, rounds that select more collapses than dec_thresh_kernel has threads, round
counts around a batch of 16 -- on marching-cubes surfaces made on the device, and at the edges of the entry point.  What each case reaches is proven on
the CPU in tests/test_decimate_cases_cpu.py."""
import numpy as np
import pytest

import decimate_cases as C
import decimate_restatement as D
from decimate_cases import assert_same, gpu_decimate

pytestmark = pytest.mark.gpu


def identical(a, b):
    return a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype


@pytest.mark.parametrize("name,budget,max_error", C.runs())
@pytest.mark.parametrize("on_device", [False, True])
def test_case_equals_restatement(gpu_ctx, name, budget, max_error, on_device):
    verts, faces = C.case(name)
    budget = C.budget_of(name, budget)
    want = C.restated(name, budget, max_error)[:3]
    got = gpu_decimate(gpu_ctx, verts, faces, budget, max_error, on_device)
    assert_same(got, want)
    assert identical(got, gpu_decimate(gpu_ctx, verts, faces, budget, max_error, on_device))


# ---- marching-cubes surfaces, made on the device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc_meshes(gpu_ctx):
    """kind -> (float64 vertices, int32 faces) of a sphere in a 24^3 volume: wholly inside it, and poking through the wall x = 0."""
    from hive_amd import fusion
    out = {}
    vol = fusion.TSDFVolume(np.array([[0.0, C.MC_DIM * C.MC_VOXEL]] * 3), C.MC_VOXEL, ctx=gpu_ctx)
    assert tuple(int(d) for d in vol.vol_dim) == (C.MC_DIM,) * 3
    for kind, (centre, radius) in C.MC_SPHERES.items():
        vol.set_volume(C.sphere_field(C.MC_DIM, centre, radius), np.zeros((C.MC_DIM,) * 3, np.float32), np.ones((C.MC_DIM,) * 3, np.float32))
        verts, faces, _, _ = vol.get_mesh()
        out[kind] = np.ascontiguousarray(verts, np.float64), np.ascontiguousarray(faces, np.int32)
    return out


_mc_restated = {}


def mc_restated(mc_meshes, kind, budget, max_error):
    key = (kind, budget, max_error)
    if key not in _mc_restated:
        _mc_restated[key] = D.decimate(*mc_meshes[kind], budget, max_error)
    return _mc_restated[key]


def test_marching_cubes_surfaces_are_closed_and_open(mc_meshes):
    verts, faces = mc_meshes["closed"]
    assert len(faces) > 500 and D.euler_and_loops(len(verts), faces) == (2, 0, 2)
    verts, faces = mc_meshes["open"]
    chi, loops, most = D.euler_and_loops(len(verts), faces)
    assert len(faces) > 300 and loops >= 1 and most == 2
    print("marching-cubes meshes:", {k: (len(v), len(f)) for k, (v, f) in mc_meshes.items()}, "open: chi, loops =", (chi, loops))


@pytest.mark.parametrize("kind", ["closed", "open"])
@pytest.mark.parametrize("budget", ["half", 64])
@pytest.mark.parametrize("max_error", [1e9, 1e-3])
def test_marching_cubes_surface_equals_restatement(gpu_ctx, mc_meshes, kind, budget, max_error):
    verts, faces = mc_meshes[kind]
    budget = len(faces) // 2 if budget == "half" else budget
    want = mc_restated(mc_meshes, kind, budget, max_error)
    print(f"{kind} sphere, {len(faces)} faces, budget {budget}, max_error {max_error}: {len(want[0])} faces left, stats {want[2]}")
    assert D.euler_and_loops(len(want[1]), want[0])[:2] == D.euler_and_loops(len(verts), faces)[:2]
    for on_device in (False, True):
        got = gpu_decimate(gpu_ctx, verts, faces, budget, max_error, on_device)
        assert_same(got, want)
        assert identical(got, gpu_decimate(gpu_ctx, verts, faces, budget, max_error, on_device))


@pytest.mark.parametrize("kind", ["closed", "open"])
@pytest.mark.parametrize("on_device", [False, True])
def test_marching_cubes_surface_as_background(gpu_ctx, mc_meshes, kind, on_device):
    """foreground.decimate_mesh with the background's budget (is_object = False), the default max_error."""
    import torch
    from hive_amd import foreground
    from hive_amd.options import MeshDecimationOptions
    verts, faces = mc_meshes[kind]
    opts = MeshDecimationOptions(num_faces_background=len(faces) // 2)
    v, f = (torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()) if on_device else (verts, faces)
    rv, rf = foreground.decimate_mesh(v, f, False, opts, ctx=gpu_ctx)
    rv, rf = (rv.cpu().numpy(), rf.cpu().numpy()) if on_device else (rv, rf)
    kept, want = D.api_decimate(verts, faces, False, opts.num_faces_object, opts.num_faces_background, opts.max_error)
    assert np.array_equal(want, mc_restated(mc_meshes, kind, len(faces) // 2, opts.max_error)[0])
    assert np.array_equal(rf, want) and rf.dtype == faces.dtype
    assert rv.dtype == np.float64 and rv.tobytes() == verts[kept].tobytes()  # rows of the input, bit for bit
    rows = {r.tobytes() for r in verts}
    assert all(r.tobytes() in rows for r in rv)


# ---- the edges of the entry point ------------------------------------------------------------------------------------------------------------------------
def _still_works(gpu_ctx, on_device):
    assert_same(gpu_decimate(gpu_ctx, *C.case("fan_12"), 6, 1e9, on_device), C.restated("fan_12", 6, 1e9)[:3])


@pytest.mark.parametrize("on_device", [False, True])
def test_no_faces(gpu_ctx, on_device):
    verts = C.case("fan_12")[0]
    none = np.zeros((0, 3), np.int32)
    for budget in (0, 1, 10):
        out, kept, stats = gpu_decimate(gpu_ctx, verts, none, budget, 1e9, on_device)
        assert out.shape == (0, 3) and np.array_equal(kept, np.arange(len(verts))) and stats == (0, 0, 0)
    _still_works(gpu_ctx, on_device)
    out, kept, stats = gpu_decimate(gpu_ctx, np.zeros((0, 3)), none, 0, 1e9, on_device)  # no vertices either
    assert out.shape == (0, 3) and kept.shape == (0,) and stats == (0, 0, 0)
    _still_works(gpu_ctx, on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_budget_zero(gpu_ctx, on_device):
    for name in ("fan_12", "tetrahedron"):
        verts, faces = C.case(name)
        want = D.decimate(verts, faces, 0, 1e9)
        assert len(want[0]) > 0  # the rounds end because nothing is legal, not at the budget
        assert_same(gpu_decimate(gpu_ctx, verts, faces, 0, 1e9, on_device), want)
        _still_works(gpu_ctx, on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_one_and_two_faces(gpu_ctx, on_device):
    """One face: nothing is legal (`v0 faces < 2`).  Two faces on an edge: an end of the shared edge may slide along the boundary (the restatement
    applies one collapse at budgets 0 and 1); every other halfedge falls to `boundary` or `v0 faces < 2`."""
    verts, faces = C.one_face()
    for budget in (0, 1):
        got = gpu_decimate(gpu_ctx, verts, faces, budget, 1e9, on_device)
        assert_same(got, D.decimate(verts, faces, budget, 1e9))
        assert np.array_equal(got[0], faces) and got[2] == (0, 0, 0)
    verts, faces = C.two_faces()
    for budget in (0, 1, 2):
        for max_error in (1e9, 0.0):
            assert_same(gpu_decimate(gpu_ctx, verts, faces, budget, max_error, on_device), D.decimate(verts, faces, budget, max_error))
    _still_works(gpu_ctx, on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_isolated_vertices_around_one_component(gpu_ctx, on_device):
    verts, faces = C.islands()
    for budget in (0, 1, 6, 11):
        want = D.decimate(verts, faces, budget, 1e9)
        got = gpu_decimate(gpu_ctx, verts, faces, budget, 1e9, on_device)
        assert_same(got, want)
        assert set(range(40)) | set(range(len(verts) - 7, len(verts))) <= set(got[1].tolist())  # isolated vertices are kept
    _still_works(gpu_ctx, on_device)
