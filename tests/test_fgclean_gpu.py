"""Connected-component clean-up of the foreground meshes (csrc/fgmesh.hip hive_mesh_cleanup_cc / hive_fg_frame_mesh_cc) against a numpy + scipy
restatement of /root/reference/hive/pipeline.py:741-779 (trimesh 3.9's face_adjacency + graph.connected_components), the frame path and
process_frame against the reference's loop restated with it, and Pipeline.run's foreground output end to end."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def reference_cleanup(n_vertices, faces, is_object=True, min_len=5):
    """What ``_cleanup_with_connected_components`` leaves, as (kept input vertex ids in order, faces indexing them): trimesh.graph.face_adjacency (edges
    that exactly two faces use, self-pairs dropped), connected_components over the faces that have a neighbour (scipy labels, grouping.group with
    min_len), argmax of the sizes, update_faces; Trimesh(process=True) has already dropped the vertices no input face references."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(faces)
    if nf == 0:
        return np.arange(n_vertices), faces
    referenced = np.zeros(n_vertices, bool)
    referenced[faces.ravel()] = True
    kept_v = np.nonzero(referenced)[0]
    edges = np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    edge_face = np.repeat(np.arange(nf), 3)
    _, inverse, counts = np.unique(edges[:, 0] << 32 | edges[:, 1], return_inverse=True, return_counts=True)
    two = counts[inverse] == 2
    order = np.argsort(inverse[two], kind="stable")
    pairs = edge_face[two][order].reshape(-1, 2)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    components = []
    if len(pairs):
        nodes = np.unique(pairs)
        n = int(nodes.max()) + 1
        graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
        _, labels = connected_components(graph, directed=False)
        labels = labels[nodes]
        for label in np.unique(labels):
            members = nodes[labels == label]
            if len(members) >= min_len:
                components.append(members)
    mask = np.zeros(nf, bool)
    if components:
        if is_object:
            mask[components[int(np.argmax([len(c) for c in components]))]] = True
        else:
            mask[np.concatenate(components)] = True
    vmap = np.full(n_vertices, -1, np.int64)
    vmap[kept_v] = np.arange(len(kept_v))
    return kept_v, vmap[faces[mask]]


def lattice_faces(valid):
    """Two triangles per 2 x 2 block of `valid` pixels, indices = pixel ids (row-major); unreferenced pixels stay as unreferenced vertices."""
    h, w = valid.shape
    ids = np.arange(h * w).reshape(h, w)
    a, b, c, d = ids[:-1, :-1], ids[:-1, 1:], ids[1:, :-1], ids[1:, 1:]
    full = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
    t1 = np.stack([a[full], c[full], b[full]], axis=1)
    t2 = np.stack([b[full], c[full], d[full]], axis=1)
    return np.stack([t1, t2], axis=1).reshape(-1, 3).astype(np.int32)


def _cases():
    rng = np.random.default_rng(11)
    cases = {}
    # a ragged body with planted floaters: random holes, separate patches of 1 .. 6 blocks, faces in shuffled order
    valid = rng.random((40, 50)) > 0.12
    valid[:, 24:26] = False
    valid[5:7, 30:32] = True
    cases["floaters"] = (40 * 50, rng.permutation(lattice_faces(valid)))
    # two equal largest components (same shape), the second one first in face order: the tie goes to the smaller face index
    strip = lattice_faces(np.ones((4, 6), bool))
    cases["tie"] = (48, np.concatenate([strip + 24, strip]))
    # an edge used by three faces joins none of them (faces 0 .. 2 share (0, 1); face 0 still reaches face 3 through (1, 2)); a face using an edge
    # twice (degenerate) pairs with nothing through it
    fan = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [2, 1, 5], [5, 1, 6], [6, 1, 7], [3, 8, 8]], np.int32)
    cases["shared_by_three"] = (10, fan)
    # isolated faces only, and unreferenced vertices around a strip
    cases["isolated"] = (30, np.arange(24, dtype=np.int32).reshape(8, 3))
    cases["unreferenced"] = (200, lattice_faces(np.ones((5, 5), bool)) * 7 + 3)
    cases["no_faces"] = (17, np.zeros((0, 3), np.int32))
    # every component below min_len (pairs of faces)
    pairs = np.concatenate([np.array([[0, 1, 2], [2, 1, 3]], np.int32) + 4 * k for k in range(6)])
    cases["all_small"] = (24, pairs)
    return cases


CASES = _cases()


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("min_components", [1, 2.5, 5])
@pytest.mark.parametrize("is_object", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_cleanup_equals_reference_restatement(gpu_ctx, case, is_object, min_components, on_device):
    import torch
    from hive_amd import foreground
    n_vertices, faces = CASES[case]
    vertices = np.random.default_rng(3).random((n_vertices, 3))
    want_vi, want_f = reference_cleanup(n_vertices, faces, is_object, min_components)
    if on_device:
        got_v, got_f = foreground.cleanup_with_connected_components(torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda(), is_object,
                                                                    min_components, ctx=gpu_ctx)
        assert got_v.is_cuda and got_f.is_cuda
        got_v, got_f = got_v.cpu().numpy(), got_f.cpu().numpy()
    else:
        got_v, got_f = foreground.cleanup_with_connected_components(vertices, faces, is_object, min_components, ctx=gpu_ctx)
    assert got_f.shape == want_f.shape and np.array_equal(got_f, want_f), case
    assert got_v.shape == (len(want_vi), 3) and np.array_equal(got_v, vertices[want_vi]), case


def test_cleanup_known_answers(gpu_ctx):
    """The restatement itself on cases small enough to state by hand."""
    from hive_amd import foreground
    n, faces = CASES["tie"]
    _, f = foreground.cleanup_with_connected_components(np.zeros((n, 3)), faces, True, 5, ctx=gpu_ctx)
    assert len(f) == len(faces) // 2 and f.min() >= 24, "the tie keeps the component with the smallest face index (the copy on vertices 24 ..)"
    n, faces = CASES["shared_by_three"]
    _, f = foreground.cleanup_with_connected_components(np.zeros((n, 3)), faces, False, 1, ctx=gpu_ctx)
    assert np.array_equal(f, faces[[0, 3, 4, 5]]), "faces 0, 3, 4, 5 are one chain; faces 1, 2 only share the three-way edge; the degenerate face is alone"
    v, f = foreground.cleanup_with_connected_components(np.arange(30.0).reshape(10, 3), CASES["isolated"][1][:3], False, 1, ctx=gpu_ctx)
    assert len(f) == 0 and len(v) == 9, "isolated faces go; the vertices the input faces referenced stay"
    v, f = foreground.cleanup_with_connected_components(np.ones((17, 3)), np.zeros((0, 3), np.int32), True, 5, ctx=gpu_ctx)
    assert len(v) == 17 and len(f) == 0


def test_cleanup_rejects_out_of_range_vertex_ids(gpu_ctx):
    from hive_amd import _lib, foreground
    with pytest.raises(_lib.HiveError):
        foreground.cleanup_with_connected_components(np.zeros((4, 3)), np.array([[0, 1, 2], [2, 1, 4]], np.int32), ctx=gpu_ctx)


def _spiral_valid(h, w, pitch=6):
    """A lattice covered by one corridor winding inwards: a square spiral wall of 1-pixel lines, `pitch` apart."""
    valid = np.ones((h, w), bool)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    while bottom - top > 2 * pitch and right - left > 2 * pitch:
        valid[top + pitch, left:right - pitch + 1] = False
        valid[top + pitch:bottom - pitch + 1, right - pitch] = False
        valid[bottom - pitch, left + pitch:right - pitch + 1] = False
        valid[top + 2 * pitch:bottom - pitch + 1, left + pitch] = False
        top, left, bottom, right = top + 2 * pitch, left + pitch, bottom - pitch, right - pitch
    return valid


def test_spiral_at_1080p_equals_scipy_and_is_deterministic(gpu_ctx):
    """About 3.5 M faces of a 1080 x 1920 lattice in one spiral component (union chains as long as the corridor) plus small floaters: the survivors equal
    the restatement's for both modes, and two runs are bit-identical."""
    import torch
    from hive_amd import foreground
    h, w = 1080, 1920
    valid = _spiral_valid(h, w)
    valid[538:550, 958:970] = False  # an 8 x 8 floater ringed by two invalid pixels
    valid[540:548, 960:968] = True
    faces = lattice_faces(valid)
    assert len(faces) > 3_000_000
    verts = torch.zeros((h * w, 3), dtype=torch.float64, device="cuda")
    f_dev = torch.from_numpy(faces).cuda()
    for is_object in (True, False):
        want_vi, want_f = reference_cleanup(h * w, faces, is_object, 5)
        runs = [foreground.cleanup_with_connected_components(verts, f_dev, is_object, 5, ctx=gpu_ctx)[1].cpu().numpy() for _ in range(2)]
        assert np.array_equal(runs[0], runs[1])
        assert np.array_equal(runs[0], want_f)
    assert len(want_f) > 0.8 * len(faces)


def _frame_with_islands(H=480, W=640):
    from hive_amd import synthetic
    seq = synthetic.make_sequence(num_frames=1, height=H, width=W, yaw_step_deg=20.0)
    depth = seq["depth"][0].copy()
    mask = np.zeros((H, W), bool)
    mask[100:380, 150:500] = True
    depth[150:154, 200:204] += 0.5        # a 4 x 4 island: 18 faces, a component above min_len that is not the largest
    depth[200:202, 300:302] += 0.5        # a 2 x 2 island: 2 faces, below min_len
    depth[250:262, 400:412] = 0.0         # a patch ringed by zero depth
    depth[254:258, 404:408] = seq["depth"][0][254:258, 404:408]
    w2c = np.linalg.inv(seq["poses"][0])
    return seq, depth, mask, w2c[:3, :3], w2c[:3, 3:4]


@pytest.mark.parametrize("is_object", [True, False])
def test_frame_mesh_with_cleanup_equals_separate_steps(gpu_ctx, is_object):
    """frame_mesh(enable_cc_analysis=True) == point_cloud_from_depth + grid_faces + the restated clean-up + get_mesh_texture_and_uv over the vertices that are
    left, bit for bit; with the clean-up off it is still hive_fg_frame_mesh's result."""
    import torch
    from hive_amd import foreground, geometric
    from hive_amd.options import MeshFilteringOptions
    seq, depth, mask, R, t = _frame_with_islands()
    K, rgb = seq["K"], seq["color"][0]
    opts = MeshFilteringOptions()
    buffers = foreground.FrameMeshBuffers(*depth.shape)
    d, m, img = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(rgb).cuda()
    pc = geometric.point_cloud_from_depth(depth, mask, K, R, t)
    f = foreground.grid_faces(depth, mask, opts, ctx=gpu_ctx)
    kept_v, want_f = reference_cleanup(len(pc), f, is_object, opts.min_num_components)
    assert len(want_f) < len(f), "the planted islands are floaters"
    want_v = pc[kept_v]
    want_tex, want_uv = foreground.get_mesh_texture_and_uv(want_v, rgb, K, R, t, ctx=gpu_ctx)
    got = foreground.frame_mesh(d, m, img, K, R, t, opts, ctx=gpu_ctx, buffers=buffers, enable_cc_analysis=True, is_object=is_object,
                                min_components=opts.min_num_components)
    assert got["before"] == (len(pc), len(f))
    assert np.array_equal(got["vertices"].cpu().numpy(), want_v)
    assert np.array_equal(got["faces"].cpu().numpy(), want_f)
    assert np.array_equal(got["uv"].cpu().numpy(), want_uv)
    assert np.array_equal(got["texture"].cpu().numpy(), want_tex)
    # off: hive_fg_frame_mesh, bit for bit (fresh buffers: the cleaned result above must not leak into it)
    plain = foreground.frame_mesh(d, m, img, K, R, t, opts, ctx=gpu_ctx)
    off = foreground.frame_mesh(d, m, img, K, R, t, opts, ctx=gpu_ctx, buffers=buffers, enable_cc_analysis=False)
    assert "before" not in off
    for key in ("vertices", "faces", "uv", "texture"):
        assert np.array_equal(off[key].cpu().numpy(), plain[key].cpu().numpy()), key
    assert off["bbox"] == plain["bbox"] and np.array_equal(plain["vertices"].cpu().numpy(), pc)


def test_process_frame_with_cleanup_equals_reference_loop(gpu_ctx):
    """process_frame(enable_cc_analysis=True) == the reference's object loop (pipeline.py:357-468) restated with the clean-up between the face filter and the
    texture; object 3 is a checkerboard of 2 x 2 depth steps whose faces all go in the clean-up: it is stacked with its vertices and texture and no face."""
    import torch
    from hive_amd import foreground, geometric, synthetic
    from hive_amd.image_processing import dilate_mask
    from hive_amd.options import MaskDilationOptions, MeshFilteringOptions
    from test_fgmesh_gpu import _reference_pack_textures
    H, W = 240, 320
    seq = synthetic.make_sequence(num_frames=1, height=H, width=W)
    ids = synthetic.ellipse_masks(1, H, W, num_objects=2, seed=3)[0].copy()
    depth, rgb = seq["depth"][0].copy(), seq["color"][0]
    ids[180:220, 250:290] = 3
    yy, xx = np.mgrid[180:220, 250:290]
    depth[180:220, 250:290] += 0.5 * (((yy // 2) + (xx // 2)) % 2)
    ids[depth == 0] = 0
    pose = np.linalg.inv(seq["poses"][0])
    R, t = pose[:3, :3], pose[:3, 3:4]
    dil, flt = MaskDilationOptions(num_iterations=0), MeshFilteringOptions()
    K = seq["K"]
    verts, faces, texs, uvs, count, kept = [], [], [], [], 0, []
    for oid in range(1, int(ids.max()) + 1):
        mask = dilate_mask(ids == oid, dil)
        if mask.mean() < 0.01:
            continue
        v = geometric.point_cloud_from_depth(depth, mask, K, R, t)
        if len(v) < 9:
            continue
        f = foreground.grid_faces(depth, mask, flt, ctx=gpu_ctx)
        if len(f) < 1:
            continue
        kept_v, f = reference_cleanup(len(v), f, True, flt.min_num_components)
        v = v[kept_v]
        tex, uv = foreground.get_mesh_texture_and_uv(v, rgb, K, R, t, ctx=gpu_ctx)
        verts.append(v), faces.append(f + count), texs.append(tex), uvs.append(uv), kept.append(oid)
        count += len(v)
        if oid == 3:
            assert len(f) == 0 and len(v) > 1000
    want_atlas, want_uv = _reference_pack_textures(texs, uvs)
    got = foreground.process_frame(torch.from_numpy(rgb).cuda(), torch.from_numpy(depth).cuda(), torch.from_numpy(ids).cuda(), K, pose, dil, flt, ctx=gpu_ctx,
                                   enable_cc_analysis=True)
    assert got["objects"] == kept == [1, 2, 3]
    assert np.array_equal(got["vertices"].cpu().numpy(), np.vstack(verts)) and np.array_equal(got["faces"].cpu().numpy(), np.vstack(faces))
    assert np.array_equal(got["texture"].cpu().numpy(), want_atlas) and np.array_equal(got["uv"].cpu().numpy(), want_uv)
    plain = foreground.process_frame(rgb, depth, ids, K, pose, dil, flt, ctx=gpu_ctx)
    assert plain["faces"].shape[0] > got["faces"].shape[0], "without the clean-up the floaters (and object 3's faces) stay"


def read_ply(path):
    """(header lines, vertex record array, faces) of a binary little-endian PLY as write_ply writes it."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    types = {"float": "<f4", "uchar": "u1"}
    fields, nv, nf = [], 0, 0
    for line in header:
        parts = line.split()
        if parts[:2] == ["element", "vertex"]:
            nv = int(parts[2])
        elif parts[:2] == ["element", "face"]:
            nf = int(parts[2])
        elif parts[0] == "property" and parts[1] != "list":
            fields.append((parts[2], types[parts[1]]))
    v = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + v.nbytes)
    return header, v, f["i"]


def test_pipeline_run_writes_foreground_meshes(gpu_ctx, tmp_path):
    """Pipeline.run on a converted TUM-layout folder whose masks hold three ellipses: mesh/fg/%06d.ply + .png per frame, equal to process_frame with the
    clean-up (float32 in the PLY); bg.ply byte-identical to a background-only run, which writes no foreground file."""
    from PIL import Image
    from hive_amd import foreground, synthetic
    from hive_amd.dataset_adaptors import get_dataset
    from hive_amd.io import HiveDataset
    from hive_amd.options import BackgroundMeshOptions, PipelineOptions
    from hive_amd.pipeline import Pipeline
    from tum_fixture import write_tum_sequence
    tum, hive = str(tmp_path / "tum"), str(tmp_path / "hive")
    n = 3
    write_tum_sequence(tum, num_frames=n, yaw_step_deg=10.0)
    ds = get_dataset(tum, hive)
    masks = synthetic.ellipse_masks(n, ds.frame_height, ds.frame_width, num_objects=3, seed=5)
    names = sorted(os.listdir(os.path.join(hive, "mask")))
    assert len(names) == n
    for name, m in zip(names, masks):
        Image.fromarray(m).save(os.path.join(hive, "mask", name))
    bg_options = BackgroundMeshOptions(sdf_voxel_size=0.04, sdf_max_voxels=1_000_000, key_frame_threshold=0.9, key_frame_step=2)

    pipe = Pipeline(options=PipelineOptions(num_frames=n), background_mesh_options=bg_options)
    pipe.run(hive, str(tmp_path / "run"))
    with open(os.path.join(hive, "profiling.json")) as f:
        profiling = __import__("json").load(f)
    assert profiling["timing"]["foreground_reconstruction"]["total"] > 0
    assert "decimation" in profiling["foreground_reconstruction"]["not_applied"]
    fg = tmp_path / "run" / "mesh" / "fg"
    assert sorted(os.listdir(fg)) == sorted([f"{i:06d}.{ext}" for i in range(n) for ext in ("ply", "png")])

    data = HiveDataset(hive)
    want = foreground.process_frame(data.rgb_dataset[0], data.depth_dataset[0], data.mask_dataset[0], data.camera_matrix,
                                    data.camera_trajectory.to_homogenous_transforms()[0], pipe.dilation_options, pipe.filtering_options, ctx=gpu_ctx,
                                    enable_cc_analysis=True)
    header, v, f = read_ply(str(fg / "000000.ply"))
    assert "comment TextureFile 000000.png" in header
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), want["vertices"].cpu().numpy().astype(np.float32))
    assert np.array_equal(np.stack([v["texture_u"], v["texture_v"]], 1), want["uv"].cpu().numpy().astype(np.float32))
    assert np.array_equal(f, want["faces"].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(fg / "000000.png")), want["texture"].cpu().numpy())

    only = Pipeline(options=PipelineOptions(num_frames=n, background_only=True), background_mesh_options=bg_options)
    only.run(hive, str(tmp_path / "run_bg"))
    assert not (tmp_path / "run_bg" / "mesh" / "fg").exists()
    with open(tmp_path / "run" / "mesh" / "bg.ply", "rb") as a, open(tmp_path / "run_bg" / "mesh" / "bg.ply", "rb") as b:
        assert a.read() == b.read()
