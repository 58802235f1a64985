"""Foreground per-frame meshing inner loops of ``Pipeline._create_scene`` (/root/reference/hive/pipeline.py:340-483) on the
MI355X: the steps behind ``point_cloud_from_depth`` that are dense per-pixel work -- triangulation of the valid pixels, the
face filter, the quadric decimation (opt-in), the connected-component clean-up that removes floaters, the texture window and UV coordinates.

  ``grid_faces``                 fused ``_triangulate_faces`` + ``_filter_faces`` for one object mask of one frame
  ``triangulate_faces``          ``Pipeline._triangulate_faces(points)`` (:651-667) for lattice points
  ``filter_faces``               ``Pipeline._filter_faces(points2d, depth, faces, options)`` (:670-694), any face list
  ``get_mesh_texture_and_uv``    ``Pipeline._get_mesh_texture_and_uv(...)`` (:782-808)
  ``cleanup_with_connected_components``  ``Pipeline._cleanup_with_connected_components(...)`` (:741-779)
  ``decimate_mesh``              ``Pipeline._decimate_mesh(...)`` (:697-738), quadric edge collapse on the GPU
  ``billboard``                  the ``--billboard`` block of ``process_frame`` (:439-447): an object flattened to its median depth

The triangulation is the implicit one of the pixel grid (csrc/fgmesh.hip): unit squares and triangles of the valid pixels plus the
(sqrt 2, sqrt 2, 2) triangles with which a lattice Delaunay bridges one-pixel holes -- after the reference's filter (sides <= 2 pixels by
default) the face set equals the one the reference gets from Qhull, up to which diagonal splits four co-circular points (Qhull's
arbitrary choice); tests/test_fgmesh_gpu.py checks that against scipy.
"""
import ctypes

import numpy as np

from hive_amd import _lib
from hive_amd._lib import MEM_DEVICE, MEM_HOST, ptr
from hive_amd._pictures import is_torch as _is_torch
from hive_amd.options import MeshDecimationOptions, MeshFilteringOptions
from hive_amd.utils import validate_camera_parameter_shapes, validate_shape


def grid_faces(depth, mask, options: MeshFilteringOptions = None, ctx=None, return_vertex_count=False):
    """Faces of the valid pixels (``mask & (depth > 0)``) of one depth map, already filtered: int32 (F, 3) indices into the
    rows of ``point_cloud_from_depth(depth, mask, ...)``.  ``depth`` float32 (H, W) (numpy or device tensor), ``mask`` bool /
    uint8 (H, W) or None."""
    options = options or MeshFilteringOptions()
    ctx = ctx or _lib.default_context()
    if _is_torch(depth):
        import torch
        d = depth.contiguous()
        assert d.dtype == torch.float32
        m = None if mask is None else mask.to(torch.uint8).contiguous()
        mem = MEM_DEVICE
    else:
        d = np.ascontiguousarray(depth, dtype=np.float32)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        mem = MEM_HOST
    assert d.ndim == 2 and (m is None or tuple(m.shape) == tuple(d.shape)), "depth (H, W) and mask (H, W)"
    h, w = (int(v) for v in d.shape)
    nf, nv = ctypes.c_int64(0), ctypes.c_int64(0)
    args = (ctx.handle, ptr(d), ptr(m), h, w, float(options.max_pixel_distance), float(options.max_depth_distance), mem)
    ctx.check(ctx.lib.hive_grid_mesh(*args, None, 0, ctypes.byref(nf), ctypes.byref(nv)))  # size the output
    if mem == MEM_DEVICE:
        import torch
        faces = torch.empty((nf.value, 3), dtype=torch.int32, device=d.device)
    else:
        faces = np.empty((nf.value, 3), np.int32)
    if nf.value:
        ctx.check(ctx.lib.hive_grid_mesh(*args, ptr(faces), nf.value, ctypes.byref(nf), ctypes.byref(nv)))
    return (faces, nv.value) if return_vertex_count else faces


def triangulate_faces(points, ctx=None):
    """``Pipeline._triangulate_faces``: faces of a set of 2D lattice points (N, 2) = (u, v) integer pixel coordinates in
    row-major order (what ``np.vstack((u, v)).T`` of ``valid.nonzero()`` gives, pipeline.py:392-395) -- no filtering."""
    validate_shape(points, 'points', expected_shape=(None, 2))
    pts = np.asarray(points)
    assert np.issubdtype(pts.dtype, np.integer) and len(pts) > 0, "lattice (integer pixel) points expected"
    u0, v0 = pts[:, 0].min(), pts[:, 1].min()
    w, h = int(pts[:, 0].max() - u0 + 1), int(pts[:, 1].max() - v0 + 1)
    grid = np.zeros((h, w), np.float32)
    grid[pts[:, 1] - v0, pts[:, 0] - u0] = 1.0
    order = np.lexsort((pts[:, 0], pts[:, 1]))
    assert np.array_equal(order, np.arange(len(pts))), "points must be in row-major (v, then u) order"
    return grid_faces(grid, None, MeshFilteringOptions(max_pixel_distance=np.inf, max_depth_distance=np.inf), ctx=ctx)


def filter_faces(points2d, depth, faces, options: MeshFilteringOptions, ctx=None):
    """``Pipeline._filter_faces``: the faces whose three edges are at most ``max_pixel_distance`` long in image space and span
    at most ``max_depth_distance`` of depth; order preserved.  Works on any triangulation of the points."""
    validate_shape(points2d, 'points2d', expected_shape=(None, 2))
    validate_shape(depth, 'depth', expected_shape=(points2d.shape[0],))
    validate_shape(faces, 'faces', expected_shape=(None, 3))
    ctx = ctx or _lib.default_context()
    p = np.ascontiguousarray(points2d, dtype=np.int32)
    d = np.ascontiguousarray(depth, dtype=np.float32)
    f = np.ascontiguousarray(faces, dtype=np.int32)
    out = np.empty_like(f)
    n = ctypes.c_int64(0)
    ctx.check(ctx.lib.hive_filter_faces(ctx.handle, ptr(p), ptr(d), len(p), ptr(f), len(f), float(options.max_pixel_distance),
                                        float(options.max_depth_distance), MEM_HOST, ptr(out), ctypes.byref(n)))
    return out[:n.value].astype(np.asarray(faces).dtype, copy=False)


def get_mesh_texture_and_uv(vertices, image, camera_matrix, rotation=np.eye(3), translation=np.zeros((3, 1)), scale_factor=1.0, ctx=None, return_bbox=False):
    """``Pipeline._get_mesh_texture_and_uv``: (cropped texture, UV coordinates relative to the crop's corner); with ``return_bbox`` also the crop box
    (min_u, min_v, max_u, max_v) the texture is ``image[min_v:max_v, min_u:max_u]`` of."""
    validate_shape(vertices, 'vertices', expected_shape=(None, 3))
    validate_shape(image, 'image', expected_shape=(None, None, 3))
    validate_camera_parameter_shapes(camera_matrix, rotation, translation)
    ctx = ctx or _lib.default_context()
    pts = np.ascontiguousarray(vertices, dtype=np.float64)
    K = np.ascontiguousarray(camera_matrix, dtype=np.float64).reshape(3, 3)
    R = np.ascontiguousarray(rotation, dtype=np.float64).reshape(3, 3)
    t = np.ascontiguousarray(translation, dtype=np.float64).reshape(3)
    uv = np.empty((len(pts), 2), np.int32)  # world2image's default dtype: rounded pixel coordinates
    box = np.zeros(4, np.int32)
    ctx.check(ctx.lib.hive_texture_window(ctx.handle, ptr(pts), len(pts), ptr(K), ptr(R), ptr(t), float(scale_factor), MEM_HOST, ptr(uv), ptr(box)))
    min_u, min_v, max_u, max_v = (int(b) for b in box)
    texture = image[min_v:max_v, min_u:max_u, :].copy()
    return (texture, uv, (min_u, min_v, max_u, max_v)) if return_bbox else (texture, uv)


def _compact_mesh(vertices, faces, ctx, call):
    """The marshalling of the calls that keep a subset of a mesh (``hive_mesh_cleanup_cc``, ``hive_mesh_decimate``): device form when either input is a tensor,
    host form otherwise.  Prepares the int32 faces ``f`` and the outputs ``out_f`` (F, 3) and ``out_vi`` (V), runs
    ``call(ctx, as_input, f, nf, nv, mem, out_f, out_vi, n_faces, n_verts)`` (``as_input(a, "float64")``: ``a`` contiguous in that dtype where ``f`` lives; the
    last two are ``byref`` counts) and returns ``(vertices[kept], faces[:n])`` in the inputs' kind and dtype."""
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    n_faces, n_verts = ctypes.c_int64(0), ctypes.c_int64(0)
    on_device = _is_torch(faces) or _is_torch(vertices)
    if on_device:
        import torch
        dev = faces.device if _is_torch(faces) else vertices.device
        ctx = ctx or _lib.default_context(dev.index or 0)
        ctx.follow_torch_stream()
        as_input = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.asarray(a))).to(device=dev, dtype=getattr(torch, dt)).contiguous()
        out_f = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        out_vi = torch.empty(nv, dtype=torch.int32, device=dev)
    else:
        ctx = ctx or _lib.default_context()
        as_input = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        out_f = np.empty((nf, 3), np.int32)
        out_vi = np.empty(nv, np.int32)
    f = as_input(faces, "int32")
    ctx.check(call(ctx, as_input, f, nf, nv, MEM_DEVICE if on_device else MEM_HOST, out_f, out_vi, ctypes.byref(n_faces), ctypes.byref(n_verts)))
    if on_device:
        keep = out_vi[:n_verts.value].long()
        v = vertices if _is_torch(vertices) else torch.from_numpy(np.asarray(vertices)).to(dev)
        out_dtype = faces.dtype if _is_torch(faces) else torch.int32
        return v.index_select(0, keep.to(v.device)), out_f[:n_faces.value].to(out_dtype)
    return np.asarray(vertices)[out_vi[:n_verts.value]], out_f[:n_faces.value].astype(np.asarray(faces).dtype, copy=False)


def cleanup_with_connected_components(vertices, faces, is_object=True, min_components=5, ctx=None):
    """``Pipeline._cleanup_with_connected_components`` (/root/reference/hive/pipeline.py:741-779) in one library call (``hive_mesh_cleanup_cc``): the
    components of trimesh's face adjacency (faces sharing an edge that exactly two faces use; a face without such a neighbour is in no component and
    goes) with at least ``min_components`` faces survive -- only the largest of them (on a tie the one with the smallest face index) when ``is_object``.
    Returns (vertices, faces) of the same kind as the inputs (numpy arrays or device tensors): the vertices some input face references, in input order
    (``Trimesh(process=True)`` drops the others before ``update_faces``; it may also reorder and merge coincident vertices, which this does not -- equal up
    to vertex order), and the surviving faces in order, indexing them.  Without faces every vertex is kept."""
    validate_shape(vertices, 'vertices', expected_shape=(None, 3))
    validate_shape(faces, 'faces', expected_shape=(None, 3))
    def call(ctx, as_input, f, nf, nv, mem, out_f, out_vi, n_faces, n_verts):
        return ctx.lib.hive_mesh_cleanup_cc(ctx.handle, ptr(f), nf, nv, int(bool(is_object)), float(min_components), mem, ptr(out_f), ptr(out_vi), n_faces, n_verts)
    return _compact_mesh(vertices, faces, ctx, call)


def billboard(vertices, rotation, translation, ctx=None, return_median=False):
    """The ``--billboard`` block of ``process_frame`` (hive/pipeline.py:439-447) in one library call (``hive_fg_billboard``): the object flattened to
    the median camera-space depth of its vertices --

        camera_space_points = rotation @ (vertices.T + translation)
        camera_space_points[2, :] = np.median(camera_space_points[2, :])
        vertices = (rotation.T @ (camera_space_points - translation)).T

    restated literally, quirk included: the map is ``R (p + t)`` and back ``R^T (c - t)``, not the ``R p + t`` of ``world2image``, so for ``t != 0`` the two are
    not inverses of each other (an object does not land on the plane z = median of the camera that ``world2image`` describes).  The operation order is the one in
    include/hive_mi355x.h; the median is numpy's, bit for bit (an exact radix select on the GPU; -0 sorts before +0).  Finite coordinates only.

    ``vertices`` (V, 3): a float64 device tensor is flattened IN PLACE and returned; a numpy array (or a tensor of another dtype) is copied, and the result is of the
    input's kind.  V = 0 is a no-op.  With ``return_median`` also the median depth (one extra synchronisation)."""
    import torch
    validate_shape(vertices, 'vertices', expected_shape=(None, 3))
    validate_camera_parameter_shapes(np.eye(3), rotation, translation)
    R = np.ascontiguousarray(rotation, dtype=np.float64).reshape(3, 3)
    t = np.ascontiguousarray(translation, dtype=np.float64).reshape(3)
    if _is_torch(vertices):
        dev = vertices.device
        v = vertices if vertices.dtype == torch.float64 and vertices.is_contiguous() else vertices.to(torch.float64).contiguous()
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        v = torch.from_numpy(np.array(vertices, dtype=np.float64, order="C")).to(dev)
    ctx = ctx or _lib.default_context(dev.index or 0)
    ctx.follow_torch_stream()
    median = ctypes.c_double(0.0)
    ctx.check(ctx.lib.hive_fg_billboard(ctx.handle, ptr(v), int(v.shape[0]), ptr(R), ptr(t), ctypes.byref(median) if return_median else None))
    out = v if _is_torch(vertices) else v.cpu().numpy()
    return (out, median.value) if return_median else out


def _decimation_budget(is_object, options):
    """``Pipeline._decimate_mesh``'s choice, quirk included (pipeline.py:711-712, 724): None = no decimation, else the face budget."""
    if (is_object and options.num_faces_object == -1) or options.num_faces_background == -1:
        return None
    return int(options.num_faces_object if is_object else options.num_faces_background)


def decimate_mesh(vertices, faces, is_object, options: MeshDecimationOptions, ctx=None, return_stats=False):
    """``Pipeline._decimate_mesh`` (/root/reference/hive/pipeline.py:697-738) in one library call (``hive_mesh_decimate``: quadric edge collapse on the GPU,
    the rules in include/hive_mi355x.h).  No decimation when ``(is_object and options.num_faces_object == -1) or options.num_faces_background == -1``, as in
    the reference; otherwise the budget is ``num_faces_object`` for an object and ``num_faces_background`` else, with ``options.max_error``.  (``options.enabled``
    is Pipeline.run's switch and is not read here.)  Returns (vertices, faces) of the same kind as the inputs (numpy arrays or device tensors): the vertices
    that survive, isolated ones included, in input order (rows of the input, bit for bit), and the surviving faces in order, indexing them; with
    ``return_stats`` also (rounds, collapses, locked vertices)."""
    validate_shape(vertices, 'vertices', expected_shape=(None, 3))
    validate_shape(faces, 'faces', expected_shape=(None, 3))
    budget = _decimation_budget(is_object, options)
    if budget is None:
        return (vertices, faces, (0, 0, 0)) if return_stats else (vertices, faces)
    stats = np.zeros(3, np.int64)

    def call(ctx, as_input, f, nf, nv, mem, out_f, out_vi, n_faces, n_verts):
        v = as_input(vertices, "float64")
        return ctx.lib.hive_mesh_decimate(ctx.handle, ptr(v), nv, ptr(f), nf, budget, float(options.max_error), mem, ptr(out_f), ptr(out_vi), n_faces, n_verts, ptr(stats))
    out = _compact_mesh(vertices, faces, ctx, call)
    return (*out, tuple(int(x) for x in stats)) if return_stats else out


class FrameMeshBuffers:
    """Device buffers of worst-case size for ``frame_mesh`` (H W vertices, 4 H W faces), reused from frame to frame."""

    def __init__(self, height, width, device="cuda"):
        import torch
        n = int(height) * int(width)
        self.shape = (int(height), int(width))
        self.vertices = torch.empty((n, 3), dtype=torch.float64, device=device)
        self.faces = torch.empty((4 * n, 3), dtype=torch.int32, device=device)
        self.uv = torch.empty((n, 2), dtype=torch.int32, device=device)


def frame_mesh(depth, mask, image, camera_matrix, rotation=np.eye(3), translation=np.zeros((3, 1)), options: MeshFilteringOptions = None, ctx=None,
               buffers: FrameMeshBuffers = None, enable_cc_analysis=False, is_object=True, min_components=5, decimation_options: MeshDecimationOptions = None,
               billboard=False):
    """One object of one frame, device-resident, in ONE library call (``hive_fg_frame_mesh``): what the loop body of ``process_frame``
    (/root/reference/hive/pipeline.py:383-461) computes between the binary mask and the texture atlas --

        vertices = point_cloud_from_depth(depth, mask, K, R, t)             (:386)
        faces    = _filter_faces(points2d, depth[valid], _triangulate_faces(points2d), options)   (:402-408)
        vertices, faces = _cleanup_with_connected_components(vertices, faces, is_object, min_components)   (:431-437; only with enable_cc_analysis)
        texture, uv = _get_mesh_texture_and_uv(vertices, rgb, K, R, t)      (:453)

    With ``enable_cc_analysis`` the call is ``hive_fg_frame_mesh_cc``: the floaters go as in ``cleanup_with_connected_components``, the vertices are the ones
    the filtered faces reference (renumbered) and the texture window covers them; the dict also carries ``before`` = (point-cloud vertices, filtered faces),
    the counts the reference tests before the clean-up.  Off (the default), the result is ``hive_fg_frame_mesh``'s.

    With ``decimation_options`` (None by default: no decimation) the call is ``hive_fg_frame_mesh_dec``: the faces after the filter go through
    ``decimate_mesh(vertices, faces, is_object, decimation_options)`` before the clean-up (when enabled) and the texture window, the reference's order
    (:402-453); the dict also carries ``before`` and ``decimated`` = (vertices, faces) after the decimation, and ``decimation_stats``.  When the reference's
    -1 rule skips the decimation the result is the one without ``decimation_options`` (plus those keys).

    With ``billboard`` (off by default) the vertices are then flattened to their median depth (``billboard()``, :439-447: after the clean-up, and after the decimation
    when that is on) and ``uv``, ``bbox`` and ``texture`` are taken again from the flattened vertices (``hive_texture_window``, :449-453); the faces stay.  Flattened
    vertices may project outside the frame (the reference's TODO at this spot): the crop is clamped to the image as below.

    ``depth`` float32 (H, W), ``mask`` bool / uint8 (H, W) or None, ``image`` uint8 (H, W, 3): device tensors (numpy arrays are uploaded).  Returns a dict of
    device tensors -- ``vertices`` float64 (V, 3), ``faces`` int32 (F, 3), ``uv`` int32 (V, 2), ``texture`` uint8 crop -- and ``bbox`` (min_u, min_v, max_u, max_v);
    views into ``buffers`` (valid until its next use) when one is given.  Bit-identical to the three separate functions; seven launches and one read-back instead
    of sixteen launches, four read-backs and the host round trip of the vertices.  An object with no valid pixel gives V = F = 0 and ``texture`` None."""
    import torch
    options = options or MeshFilteringOptions()
    validate_camera_parameter_shapes(camera_matrix, rotation, translation)
    dev = depth.device if _is_torch(depth) else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or _lib.default_context(dev.index or 0)
    ctx.follow_torch_stream()
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    d = as_dev(depth, torch.float32)
    m = None if mask is None else as_dev(mask, torch.uint8)
    img = None if image is None else as_dev(image, torch.uint8)
    assert d.dim() == 2 and (m is None or tuple(m.shape) == tuple(d.shape)), "depth (H, W) and mask (H, W)"
    h, w = (int(v) for v in d.shape)
    buffers = buffers or FrameMeshBuffers(h, w, dev)
    assert buffers.shape == (h, w), "buffers were sized for another frame size"
    from hive_amd.geometric import _kinv
    K = np.ascontiguousarray(camera_matrix, dtype=np.float64).reshape(3, 3)
    Kinv = _kinv(np.asarray(camera_matrix).reshape(3, 3))  # as point_cloud_from_depth computes it: inverted in K's own dtype (geometric.py:203)
    R = np.ascontiguousarray(rotation, dtype=np.float64).reshape(3, 3)
    t = np.ascontiguousarray(translation, dtype=np.float64).reshape(3)
    nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    box = np.zeros(4, np.int32)
    before = None
    budget = None if decimation_options is None else _decimation_budget(is_object, decimation_options)
    decimated, stats = None, np.zeros(3, np.int64)
    # what the three entry points share: the inputs through max_depth_distance in front, the buffers and results behind the stages' own arguments
    inputs = (ctx.handle, ptr(d), ptr(m), h, w, ptr(Kinv), ptr(K), ptr(R), ptr(t), float(options.max_pixel_distance), float(options.max_depth_distance))
    outputs = (ptr(buffers.vertices), buffers.vertices.shape[0], ptr(buffers.faces), buffers.faces.shape[0], ptr(buffers.uv), ctypes.byref(nv), ctypes.byref(nf), ptr(box))
    cleanup = (int(bool(is_object)), float(min_components))
    counts, after = np.zeros(2, np.int64), np.zeros(2, np.int64)
    if budget is not None:
        ctx.check(ctx.lib.hive_fg_frame_mesh_dec(*inputs, budget, float(decimation_options.max_error), int(bool(enable_cc_analysis)), *cleanup, *outputs, ptr(counts),
                                                 ptr(after), ptr(stats)))
        before, decimated = (int(counts[0]), int(counts[1])), (int(after[0]), int(after[1]))
    elif enable_cc_analysis:
        ctx.check(ctx.lib.hive_fg_frame_mesh_cc(*inputs, *cleanup, *outputs, ptr(counts)))
        before = (int(counts[0]), int(counts[1]))
    else:
        ctx.check(ctx.lib.hive_fg_frame_mesh(*inputs, *outputs))
    if billboard and nv.value:
        ctx.check(ctx.lib.hive_fg_billboard(ctx.handle, ptr(buffers.vertices), nv.value, ptr(R), ptr(t), None))
        ctx.check(ctx.lib.hive_texture_window(ctx.handle, ptr(buffers.vertices), nv.value, ptr(K), ptr(R), ptr(t), 1.0, MEM_DEVICE, ptr(buffers.uv), ptr(box)))
    min_u, min_v, max_u, max_v = (int(b) for b in box)
    texture = None
    if nv.value and img is not None:
        texture = img[max(min_v, 0):max_v, max(min_u, 0):max_u, :].clone()  # `image[min_v:max_v, min_u:max_u, :].copy()` (pipeline.py:805)
    out = {"vertices": buffers.vertices[:nv.value], "faces": buffers.faces[:nf.value], "uv": buffers.uv[:nv.value], "texture": texture,
           "bbox": (min_u, min_v, max_u, max_v)}
    if before is not None:
        out["before"] = before
    if decimation_options is not None:
        if decimated is None:  # skipped by the -1 rule: the counts after the filter
            before = out.get("before", (nv.value, nf.value))
            out["before"] = before
            decimated = before
        out["decimated"] = decimated
        out["decimation_stats"] = tuple(int(x) for x in stats)
    return out


def pack_textures_row(textures, uvs):
    """``Pipeline._pack_textures(textures_atlas, uvs_atlas, n_rows=1)`` (/root/reference/hive/pipeline.py:811-866) for the one form the reference calls: the objects' texture
    crops side by side in ONE row (top-aligned, zero below the shorter ones), every object's u shifted by the widths in front of it, then u / atlas width and
    v -> 1 - v / atlas height.  ``textures``: uint8 (h_i, w_i, 3) device tensors, ``uvs``: (V_i, 2) integer tensors relative to their crop.  Returns (atlas uint8
    (max h, sum w, 3), uv float64 (sum V, 2)) on the device."""
    import torch
    assert len(textures) == len(uvs) and len(textures) > 0
    height, width = max(int(t.shape[0]) for t in textures), sum(int(t.shape[1]) for t in textures)
    atlas = torch.zeros((height, width, 3), dtype=torch.uint8, device=textures[0].device)
    shifted, x = [], 0
    for tex, uv in zip(textures, uvs):
        h, w = int(tex.shape[0]), int(tex.shape[1])
        atlas[:h, x:x + w] = tex
        moved = uv.to(torch.float64)
        moved[:, 0] += x
        shifted.append(moved)
        x += w
    out = torch.cat(shifted)
    # (tensor / tensor: torch turns a division by a Python scalar into a multiplication by its reciprocal on the GPU -- one ulp off numpy's `/=` in places)
    size = torch.tensor([float(width), float(height)], dtype=torch.float64, device=out.device)
    out = out / size
    out[:, 1] = 1.0 - out[:, 1]
    return atlas, out


def process_frame(rgb, depth, mask_encoded, camera_matrix, pose, dilation_options=None, filtering_options: MeshFilteringOptions = None,
                  disable_coverage_constraint=False, ctx=None, buffers: FrameMeshBuffers = None, enable_cc_analysis=False,
                  decimation_options: MeshDecimationOptions = None, billboard=False):
    """The body of ``process_frame`` in ``Pipeline._create_scene`` (/root/reference/hive/pipeline.py:340-483) for the dynamic objects of ONE frame, device-resident:
    for every object id 1 .. mask_encoded.max(): the binary mask, dilated (``dilate_mask``, :369-370); skipped when it covers less than 1 % of the frame (:374-379); its
    mesh in one library call (``frame_mesh``: point cloud, triangulation + face filter, texture window); skipped with fewer than 9 vertices or no face (:388-391, 410-413);
    the objects' vertices stacked, their faces offset by the vertices in front, their textures packed in one atlas row (:463-468, 811-866).  With ``enable_cc_analysis``
    (the reference's ``Pipeline.process_frame`` keyword; off by default here) every object goes through the connected-component clean-up (:431-437) with
    ``filtering_options.min_num_components`` between the face filter and the texture window; an object whose faces all go is still stacked (its vertices and texture,
    no face), as in the reference.  With ``decimation_options`` (None by default: no decimation) every object is decimated after the face filter and before
    the clean-up (:415-429, ``decimate_mesh`` with is_object=True) and the result also carries ``decimation`` = {object id: (vertices, faces) before,
    (vertices, faces) after}, the reference's ``mesh_decimation`` profiling counts.  With ``billboard`` (the reference's ``--billboard``; off by default) every
    object is flattened to its median depth after those stages and textured from the flattened vertices (:439-453, ``frame_mesh(billboard=True)``).

    ``rgb`` uint8 (H, W, 3+), ``depth`` float32 (H, W), ``mask_encoded`` uint8 (H, W) instance ids (0 = background), ``pose`` the frame's 4 x 4 world-to-camera transform
    (``dataset.camera_trajectory.to_homogenous_transforms()[index]``).  Numpy arrays or device tensors.  Returns None for a frame without a surviving object (the reference
    returns an empty ``trimesh.Trimesh()``), else a dict of device tensors: ``vertices`` float64 (V, 3), ``faces`` int64 (F, 3), ``uv`` float64 (V, 2) in atlas
    coordinates, ``texture`` uint8 atlas, and ``objects`` = the ids that survived."""
    import torch
    from hive_amd.options import MaskDilationOptions
    dilation_options = dilation_options or MaskDilationOptions()
    filtering_options = filtering_options or MeshFilteringOptions()
    dev = depth.device if _is_torch(depth) else torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or _lib.default_context(dev.index or 0)
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    rgb_d = as_dev(rgb, torch.uint8)[:, :, :3].contiguous()  # (`rgb[:, :, :3]`, :355)
    depth_d = as_dev(depth, torch.float32)
    ids = as_dev(mask_encoded, torch.uint8)
    h, w = (int(v) for v in depth_d.shape)
    buffers = buffers or FrameMeshBuffers(h, w, dev)
    pose = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    rotation, translation = pose[:3, :3], pose[:3, 3:4]  # get_pose_components
    se = dilation_options.structuring_element()
    n_objects = int(ids.max().item())
    vertices, faces, uvs, textures, kept = [], [], [], [], []
    decimation = {}
    vertex_count = 0
    for object_id in range(1, n_objects + 1):
        mask = (ids == object_id).to(torch.uint8)
        if dilation_options.num_iterations > 0:
            ctx.follow_torch_stream()
            grown = torch.empty_like(mask)
            ctx.check(ctx.lib.hive_dilate_mask_se(ctx.handle, ptr(mask), h, w, ptr(se), se.shape[0], se.shape[1], int(dilation_options.num_iterations), MEM_DEVICE, ptr(grown)))
            mask = grown
        if float(mask.float().mean().item()) < 0.01 and not disable_coverage_constraint:
            continue
        mesh = frame_mesh(depth_d, mask, rgb_d, camera_matrix, rotation, translation, filtering_options, ctx=ctx, buffers=buffers,
                          enable_cc_analysis=enable_cc_analysis, is_object=True, min_components=filtering_options.min_num_components,
                          decimation_options=decimation_options, billboard=billboard)
        n_points, n_filtered = mesh.get("before", (mesh["vertices"].shape[0], mesh["faces"].shape[0]))
        if n_points < 9 or n_filtered < 1:
            continue
        if decimation_options is not None:
            decimation[object_id] = ((n_points, n_filtered), mesh["decimated"])
        vertices.append(mesh["vertices"].clone())
        faces.append(mesh["faces"].to(torch.int64) + vertex_count)
        uvs.append(mesh["uv"].clone())
        textures.append(mesh["texture"])
        vertex_count += int(mesh["vertices"].shape[0])
        kept.append(object_id)
    if not kept:
        return None
    atlas, uv = pack_textures_row(textures, uvs)
    out = {"vertices": torch.cat(vertices), "faces": torch.cat(faces), "uv": uv, "texture": atlas, "objects": kept}
    if decimation_options is not None:
        out["decimation"] = decimation
    return out
