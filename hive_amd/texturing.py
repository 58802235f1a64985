"""Texture a mesh from posed frames on the MI355X (csrc/texture.hip): per face the one view that sees it best, an atlas with two faces per block, one gather
per texel.  The reference has no counterpart: its background mesh keeps the TSDF volume's vertex colours (/root/reference/hive/pipeline.py:258-286), one colour
per voxel corner however sharp the frames are.

The rules -- the candidate test on the rasteriser's own snapped vertices and depth plane, the 64-bit area | view key, the atlas layout, the barycentric map of a
texel, the bilinear sample -- are stated in include/hive_mi355x.h above ``hive_texture_select`` and restated in numpy in tests/texturing_restatement.py; the
kernels match that restatement bit for bit.  Not done here: seam levelling or label smoothing between neighbouring faces that chose different views, exposure
compensation, blending of several views, a back-face test."""
import ctypes

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr
from hive_amd._pictures import is_torch as _is_torch
from hive_amd.geometric import CameraMatrix, pose_vec2mat
from hive_amd.render import RenderBuffers, _host

MIN_CELL, MAX_CELL, MAX_ATLAS, MAX_VIEWS = 6, 64, 16384, 65535


def atlas_layout(num_faces, cell=8):
    """(Wt, Ht, per_row) of ``hive_texture_layout``: faces 2k and 2k + 1 share block k of ``cell`` x ``cell`` texels, ``per_row = ceil(sqrt(blocks))`` blocks in a
    row.  Host arithmetic (no GPU).  ValueError: no face, ``cell`` outside [6, 64], a side above 16384."""
    num_faces, cell = int(num_faces), int(cell)
    if num_faces < 1:
        raise ValueError("an empty mesh has no atlas")
    if not MIN_CELL <= cell <= MAX_CELL:
        raise ValueError(f"cell {cell} outside [{MIN_CELL}, {MAX_CELL}]")
    wt, ht, per_row = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if _lib.load().hive_texture_layout(num_faces, cell, ctypes.byref(wt), ctypes.byref(ht), ctypes.byref(per_row)) != _lib.OK:
        blocks = (num_faces + 1) // 2
        raise ValueError(f"{num_faces} faces at cell {cell} need an atlas of about {int(np.ceil(np.sqrt(blocks))) * cell} texels a side, over {MAX_ATLAS}")
    return wt.value, ht.value, per_row.value


def _mesh_parts(mesh):
    if isinstance(mesh, dict):
        return mesh.get("vertices"), mesh.get("faces"), mesh.get("vertex_colors")
    return getattr(mesh, "vertices", None), getattr(mesh, "faces", None), getattr(getattr(mesh, "visual", None), "vertex_colors", None)


def _poses(camera_poses):
    poses = _host(camera_poses).astype(np.float64)
    if poses.ndim == 2 and poses.shape[1] == 7:
        poses = np.stack([pose_vec2mat(p) for p in poses]) if len(poses) else poses.reshape(0, 4, 4)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"camera_poses: (n, 7) rows or (n, 4, 4) world-to-camera matrices, got shape {poses.shape}")
    return poses


def _frames(frames):
    """One (n, H, W, 3) uint8 array or tensor, or a sequence of (H, W, 3) pictures of one size."""
    if isinstance(frames, (list, tuple)):
        if len(frames) == 0:
            raise ValueError("no frame to texture from")
        shapes = {tuple(f.shape) for f in frames}
        if len(shapes) != 1:
            raise ValueError(f"frames of mixed size: {sorted(shapes)}")
        import torch
        frames = torch.stack(list(frames)) if _is_torch(frames[0]) else np.stack([np.asarray(f) for f in frames])
    if getattr(frames, "ndim", 0) != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames: uint8 (n, H, W, 3), got shape {tuple(getattr(frames, 'shape', ()))}")
    return frames


def texture_mesh(mesh, frames, camera_matrix, camera_poses, masks=None, cell=8, depth_tolerance=0.05, near=0.05, ctx=None, buffers: RenderBuffers = None,
                 return_views=False):
    """The mesh with a texture atlas filled from the frames: a dict with ``vertices`` (3F, 3) float64, ``faces`` (F, 3) int32, ``uv`` (3F, 2) float64 and ``texture``
    (Ht, Wt, 3) uint8 as device tensors -- the keys of a ``foreground.process_frame`` mesh, so ``render_mesh``, ``gltf.Scene.add_geometry`` and ``write_glb`` take it
    as it is.  With ``return_views`` also ``views`` int32 (F,): the frame each face was textured from, -1 for none.

    ``mesh``: a ``mesh.Mesh`` / trimesh, or a dict with ``vertices``, ``faces`` and ``vertex_colors`` (faces no view sees are filled from the vertex colours, so the
    whole mesh stays one textured primitive).  ``frames``: uint8 (n, H, W, 3), numpy or device (or a sequence of pictures of one size).  ``camera_matrix``: a
    ``CameraMatrix`` or a 3 x 3 array.  ``camera_poses``: (n, 7) rows (``pose_vec2mat``) or (n, 4, 4) world-to-camera matrices, as ``render_mesh`` takes one.
    ``masks``: (n, H, W), non-zero = do not use that pixel.  ``cell``: the side of an atlas block (two faces) in texels.  ``depth_tolerance``: how far behind the
    rendered surface a vertex may lie and still count as seen (a parameter default: 5 cm for a scene in metres); ``near``: ``render_mesh``'s.  Each face takes the
    view in which its exact snapped area is largest; on equal area the lower index.  There is no back-face test and no blending.

    ValueError: an empty mesh, no frame or more than 65535, frames of mixed size, ``cell`` outside [6, 64], an atlas side above 16384, a mesh without vertex
    colours, face ids outside [0, V)."""
    import torch
    vertices, faces, colors = _mesh_parts(mesh)
    if vertices is None or faces is None or len(vertices) == 0 or len(faces) == 0:
        raise ValueError("an empty mesh cannot be textured")
    if colors is None:
        raise ValueError("a mesh needs vertex colours: faces that no view sees are filled from them")
    frames = _frames(frames)
    n, h, w = (int(v) for v in frames.shape[:3])
    if n == 0 or n > MAX_VIEWS:
        raise ValueError(f"{n} frames: between 1 and {MAX_VIEWS}")
    if not near > 0:
        raise ValueError(f"near must be > 0, got {near}")
    if not depth_tolerance >= 0:
        raise ValueError(f"depth_tolerance must be >= 0, got {depth_tolerance}")
    K = np.ascontiguousarray(camera_matrix.matrix if isinstance(camera_matrix, CameraMatrix) else _host(camera_matrix), dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera_matrix: a CameraMatrix or a 3 x 3 array, got shape {K.shape}")
    poses = _poses(camera_poses)
    if len(poses) != n:
        raise ValueError(f"{n} frames and {len(poses)} poses")
    if masks is not None and tuple(masks.shape) != (n, h, w):
        raise ValueError(f"masks: (n, H, W) = {(n, h, w)}, got {tuple(masks.shape)}")
    nf, nv = len(faces), len(vertices)
    wt, ht, _ = atlas_layout(nf, cell)
    if 3 * nf >= 2 ** 31:
        raise ValueError(f"{nf} faces need {3 * nf} vertices: the indices are int32")

    dev = buffers.device if buffers is not None else next((a.device for a in (vertices, frames) if _is_torch(a) and a.is_cuda), None) or \
        torch.device("cuda", torch.cuda.current_device())
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    v, f = as_dev(vertices, torch.float64), as_dev(faces, torch.int32)
    c = as_dev(colors, torch.uint8)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"a mesh needs vertices (V, 3) and faces (F, 3), got {tuple(v.shape)} and {tuple(f.shape)}")
    if c.dim() != 2 or c.shape[0] != nv or c.shape[1] not in (3, 4):
        raise ValueError(f"vertex colours (V, 3) or (V, 4), got {tuple(c.shape)}")
    c = c[:, :3].contiguous()
    lo, hi = torch.aminmax(f)
    if int(lo) < 0 or int(hi) >= nv:
        raise ValueError(f"face ids {int(lo)} .. {int(hi)} outside [0, {nv})")
    d_frames = as_dev(frames, torch.uint8)
    d_masks = None if masks is None else ((masks if _is_torch(masks) else torch.from_numpy(np.ascontiguousarray(masks))).to(dev) != 0).to(torch.uint8).contiguous()
    d_poses = torch.from_numpy(np.ascontiguousarray(np.concatenate([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3]], axis=1))).to(dev)

    ctx = ctx or _lib.default_context(dev.index or 0)
    ctx.follow_torch_stream()
    buffers = buffers or RenderBuffers(h, w, dev)
    if buffers.shape != (h, w):
        raise ValueError(f"buffers were sized for {buffers.shape}, not {(h, w)}")
    lib, handle = ctx.lib, ctx.handle
    buffers._used = 0
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    best = torch.zeros(nf, dtype=torch.int64, device=dev)  # (the bits of a uint64)
    for k in range(n):
        R, t = np.ascontiguousarray(poses[k, :3, :3]), np.ascontiguousarray(poses[k, :3, 3])
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
        ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), h, w, float(near), ptr(xy), ptr(z), ptr(large), ptr(counts),
                                       ptr(buffers.key)))
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, None, None, ptr(depth), None))
        ctx.check(lib.hive_texture_select(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), ptr(None if d_masks is None else d_masks[k]), h, w, k,
                                          float(depth_tolerance), ptr(best)))
    out = dict(vertices=torch.empty((3 * nf, 3), dtype=torch.float64, device=dev), faces=torch.empty((nf, 3), dtype=torch.int32, device=dev),
               uv=torch.empty((3 * nf, 2), dtype=torch.float64, device=dev), texture=torch.empty((ht, wt, 3), dtype=torch.uint8, device=dev))
    views = torch.empty(nf, dtype=torch.int32, device=dev) if return_views else None
    ctx.check(lib.hive_texture_unweld(handle, ptr(v), nv, ptr(f), nf, int(cell), ptr(best), ptr(out["vertices"]), ptr(out["faces"]), ptr(out["uv"]), ptr(views)))
    ctx.check(lib.hive_texture_fill(handle, ptr(v), nv, ptr(c), ptr(f), nf, ptr(best), ptr(d_frames), n, h, w, ptr(K), ptr(d_poses), float(near), int(cell),
                                    ptr(out["texture"])))
    if return_views:
        out["views"] = views
    return out
