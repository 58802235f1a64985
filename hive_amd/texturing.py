"""Texture a mesh from posed frames on the MI355X (csrc/texture.hip): per face the one view that sees it best, an atlas with two faces per block, one gather
per texel.  The reference has no counterpart: its background mesh keeps the TSDF volume's vertex colours (/root/reference/hive/pipeline.py:258-286), one colour
per voxel corner however sharp the frames are.

The rules -- the candidate test on the rasteriser's own snapped vertices and depth plane, the 64-bit area | view key, the atlas layout, the barycentric map of a
texel, the bilinear sample -- are stated in include/hive_mi355x.h above ``hive_texture_select`` and restated in numpy in tests/texturing_restatement.py; the
kernels match that restatement bit for bit.

With ``smoothness`` or ``cull_back_faces`` the labels come from csrc/texture_smooth.hip instead (rules above ``hive_texture_vote``, restated in
tests/texture_smoothing_restatement.py): every view's areas are kept in a table, the faces' edge adjacency is built, and labels move while that lowers
-(area kept) + seam cost x (seam edges) -- iterated conditional modes, a local optimum, not a graph cut.  Not done here: a chart atlas (the layout stays three
vertices per face and ``cell``^2 texels per face pair), blending of several views.

With ``exposure`` or ``levelling`` csrc/texture_level.hip corrects what stays visible at the label changes that remain (rules above ``hive_texture_samples``,
restated in tests/texture_levelling_restatement.py): one Q16 gain per key frame and channel from the faces two views share, and additive offsets that close the
step at the seam vertices and are harmonic inside each patch.  A border between a textured and an untextured face is not levelled."""
import ctypes
import math

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


AREA_UNITS_PER_PX2 = 131072  # the snapped area A is twice the area in 1/256-pixel units: 2 * 256 * 256 per square pixel
STATS = ("rounds", "label_changes", "seam_entries_before", "seam_entries_after", "area_given_up_px2")


def _context(ctx, dev):
    ctx = ctx or _lib.default_context(dev.index or 0)
    return ctx.follow_torch_stream()


def face_neighbours(faces, num_vertices, ctx=None):
    """The edge adjacency of a triangle list (``hive_mesh_face_neighbours``): ``(offsets int64 (F + 1,), neighbours int32 (total,))`` on the device; face f's
    neighbour entries are ``neighbours[offsets[f]:offsets[f + 1]]``, ascending, one entry per edge shared.  A face with an id outside [0, num_vertices) or a
    repeated id has none.  ``faces``: int (F, 3), numpy or device."""
    import torch
    dev = faces.device if _is_torch(faces) and faces.is_cuda else torch.device("cuda", torch.cuda.current_device())
    f = (faces if _is_torch(faces) else torch.from_numpy(np.ascontiguousarray(faces))).to(device=dev, dtype=torch.int32).contiguous()
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces (F, 3), got {tuple(f.shape)}")
    nf = f.shape[0]
    if 3 * nf >= 2 ** 31:
        raise ValueError(f"{nf} faces: 3 F must stay below 2^31")
    ctx = _context(ctx, dev)
    offsets = torch.empty(nf + 1, dtype=torch.int64, device=dev)
    capacity, total = 3 * nf, ctypes.c_int64(0)  # what a closed manifold has
    for attempt in range(2):
        neighbours = torch.empty(capacity, dtype=torch.int32, device=dev)
        rc = ctx.lib.hive_mesh_face_neighbours(ctx.handle, ptr(f), nf, int(num_vertices), ptr(offsets), ptr(neighbours), capacity, ctypes.byref(total))
        if rc == _lib.OK or attempt == 1 or total.value <= capacity:
            break
        capacity = total.value  # an edge with more than two faces: once more with what the call counted
    ctx.check(rc)
    return offsets, neighbours[:total.value]


def smooth_labels(area, offsets, neighbours, seam_cost, ctx=None, rounds_per_poll=0):
    """``hive_texture_smooth``: ``(best, stats)`` -- ``best`` int64 (F,) on the device holding the bits of the uint64 keys ``area << 16 | (65535 - view)`` (0 = no
    view), ``stats`` the five integers {rounds, label changes, seam entries before, seam entries after, area given up} in the table's unit.  ``area``: int64
    (n, F) (numpy or device), ``offsets`` / ``neighbours`` as ``face_neighbours`` returns them, ``seam_cost``: an integer in [0, 2^40) in the same unit;
    ``rounds_per_poll``: rounds issued between two read-backs (0: the default; the result does not depend on it)."""
    import torch
    dev = next((a.device for a in (area, offsets, neighbours) if _is_torch(a) and a.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    area, offsets, neighbours = as_dev(area, torch.int64), as_dev(offsets, torch.int64), as_dev(neighbours, torch.int32)
    if area.dim() != 2 or offsets.dim() != 1 or neighbours.dim() != 1 or offsets.shape[0] != area.shape[1] + 1:
        raise ValueError(f"area (n, F), offsets (F + 1,), neighbours (total,), got {tuple(area.shape)}, {tuple(offsets.shape)}, {tuple(neighbours.shape)}")
    n, nf = (int(v) for v in area.shape)
    if n * nf >= 2 ** 31:
        raise ValueError(f"{n} views x {nf} faces: the table must stay below 2^31 entries")
    ctx = _context(ctx, dev)
    best = torch.zeros(nf, dtype=torch.int64, device=dev)
    stats = np.zeros(5, np.int64)
    ctx.check(ctx.lib.hive_texture_smooth(ctx.handle, ptr(area), n, nf, ptr(offsets), ptr(neighbours), int(neighbours.shape[0]), int(seam_cost), int(rounds_per_poll),
                                          ptr(best), ptr(stats)))
    return best, stats


MAX_EXPOSURE_VIEWS, MAX_SWEEPS, UNIT_GAIN, MIN_GAIN, MAX_GAIN = 256, 4096, 65536, 16384, 262144


def exposure_sums(samples, ctx=None):
    """``hive_texture_exposure_sums``: ``(G, D, N)`` as numpy int64 of shapes (3, n, n), (3, n, n) and (n, n) from the table ``samples`` uint16 (n, F, 3) that n calls of
    ``hive_texture_samples`` wrote (numpy or device; (0, 0, 0) = invalid).  Over the faces valid in both views a != b: ``G[c, a, b]`` = sum s_a s_b, ``D[c, a, b]`` =
    sum s_a^2, ``N[a, b]`` = their number.  ValueError: more than 256 views, n F >= 2^31."""
    import torch
    dev = samples.device if _is_torch(samples) and samples.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if _is_torch(samples):
        s = samples.to(device=dev).contiguous()
        if s.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
            raise ValueError(f"samples: a tensor of uint16 words (or int16 holding their bits), got {s.dtype}")
    else:
        s = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.uint16).view(np.int16)).to(dev)  # (the bits: older torch copies no uint16 from numpy)
    if s.dim() != 3 or s.shape[2] != 3:
        raise ValueError(f"samples (n, F, 3), got {tuple(s.shape)}")
    n, nf = int(s.shape[0]), int(s.shape[1])
    if not 1 <= n <= MAX_EXPOSURE_VIEWS:
        raise ValueError(f"{n} views: the exposure sums take between 1 and {MAX_EXPOSURE_VIEWS}")
    if n * nf >= 2 ** 31:
        raise ValueError(f"{n} views x {nf} faces: the table must stay below 2^31 entries")
    ctx = _context(ctx, dev)
    G, D, N = np.zeros((3, n, n), np.int64), np.zeros((3, n, n), np.int64), np.zeros((n, n), np.int64)
    ctx.check(ctx.lib.hive_texture_exposure_sums(ctx.handle, ptr(s), n, nf, ptr(G), ptr(D), ptr(N)))
    return G, D, N


def solve_gains(G, D, prior=0.01):
    """The host's part of the exposure rule (include/hive_mi355x.h, ``solve``): ``(q, fallback_channels)`` -- ``q`` uint32 (n, 3), the Q16 gain of every view and
    channel, and the list of channels whose solve failed (they keep 65536).  Per channel, in float64: e_a = sum_b D[a, b] (an exact integer), M_aa = e_a + prior e_a,
    M_ab = -G[a, b], rhs_a = prior e_a, a view without overlap (e_a = 0) the identity row; g = numpy.linalg.solve(M, rhs), renormalised so that the energy-weighted
    mean gain of the views with overlap is 1; q = clip(floor(g 65536 + 0.5), 16384, 262144).  ``prior`` has no unit (0.01 is a parameter default, not a measured
    optimum)."""
    G, D = np.asarray(G), np.asarray(D)
    if G.ndim != 3 or G.shape[0] != 3 or G.shape[1] != G.shape[2] or D.shape != G.shape:
        raise ValueError(f"G and D (3, n, n), got {G.shape} and {D.shape}")
    if not (math.isfinite(prior) and prior >= 0):
        raise ValueError(f"the prior must be finite and >= 0, got {prior}")
    n, lam = G.shape[1], np.float64(prior)
    q, fallback = np.full((n, 3), UNIT_GAIN, np.uint32), []
    for ch in range(3):
        e = [sum(int(D[ch, a, b]) for b in range(n)) for a in range(n)]  # (Python integers: exact)
        M, rhs = np.zeros((n, n), np.float64), np.zeros(n, np.float64)
        for a in range(n):
            if e[a] == 0:
                M[a, a], rhs[a] = 1.0, 1.0
                continue
            ea = np.float64(e[a])
            M[a] = -G[ch, a].astype(np.float64)
            M[a, a] = ea + lam * ea
            rhs[a] = lam * ea
        seen = [a for a in range(n) if e[a] > 0]
        try:
            with np.errstate(all="ignore"):
                g = np.linalg.solve(M, rhs)
                if not (np.isfinite(g).all() and (g > 0).all()):  # (the solve's own gains: the renormalisation would turn two negative ones positive)
                    raise np.linalg.LinAlgError("a gain that is not finite or not positive")
                if seen:
                    total = weighted = np.float64(0.0)
                    for a in seen:
                        total = total + np.float64(e[a])
                        weighted = weighted + np.float64(e[a]) * g[a]
                    g = np.where(np.asarray(e) > 0, g * total / weighted, g)
            if not (np.isfinite(g).all() and (g > 0).all()):
                raise np.linalg.LinAlgError("a gain that is not finite or not positive")
        except np.linalg.LinAlgError:
            fallback.append(ch)
            continue
        q[:, ch] = np.clip(np.floor(g * 65536.0 + 0.5), MIN_GAIN, MAX_GAIN).astype(np.uint32)
    return q, fallback


def _gains_on(gains_q16, n, dev):
    import torch
    q = np.ascontiguousarray(_host(gains_q16)).astype(np.int64)
    if q.shape != (n, 3) or (q < 0).any() or (q >= 2 ** 32).any():
        raise ValueError(f"gains_q16: ({n}, 3) integers in [0, 2^32), got shape {q.shape}")
    return torch.from_numpy(q.astype(np.uint32).view(np.int32)).to(dev)  # (the bits of the uint32 words)


def level_offsets(mesh, labels, frames, camera_matrix, camera_poses, gains_q16=None, sweeps=64, ctx=None):
    """``hive_texture_level``: ``(offsets, stats)`` -- ``offsets`` float64 (F, 3, 3) on the device, per face corner and channel the additive offset of its node
    (vertex, label), and ``stats`` = dict(seam_vertices, sweeps, max_offset).  ``mesh`` as ``texture_mesh`` takes it (the vertex colours are not used), ``labels`` int
    (F,): the view each face is textured from, -1 for none (what ``return_views`` returns), ``gains_q16`` (n, 3) Q16 integers (None: all 65536)."""
    import torch
    vertices, faces, _ = _mesh_parts(mesh)
    frames = _frames(frames)
    n, h, w = (int(v) for v in frames.shape[:3])
    sweeps = int(sweeps)
    if not 0 <= sweeps <= MAX_SWEEPS:
        raise ValueError(f"{sweeps} sweeps outside [0, {MAX_SWEEPS}]")
    K = np.ascontiguousarray(camera_matrix.matrix if isinstance(camera_matrix, CameraMatrix) else _host(camera_matrix), dtype=np.float64)
    poses = _poses(camera_poses)
    if K.shape != (3, 3) or len(poses) != n or not 1 <= n <= MAX_VIEWS:
        raise ValueError(f"a 3 x 3 camera matrix and one pose per frame (1 .. {MAX_VIEWS} frames), got {K.shape}, {n} frames and {len(poses)} poses")
    dev = next((a.device for a in (vertices, frames, labels) if _is_torch(a) and a.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    v, f, lab = as_dev(vertices, torch.float64), as_dev(faces, torch.int32), as_dev(labels, torch.int64)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3 or lab.shape != (nf,) or nf == 0 or nv == 0 or 3 * nf >= 2 ** 31:
        raise ValueError(f"vertices (V, 3), faces (F, 3) with 0 < 3 F < 2^31 and labels (F,), got {tuple(v.shape)}, {tuple(f.shape)} and {tuple(lab.shape)}")
    best = torch.where((lab >= 0) & (lab < n), (1 << 16) | (65535 - lab), torch.zeros_like(lab)).contiguous()  # keys of area 1
    q = _gains_on(np.full((n, 3), UNIT_GAIN) if gains_q16 is None else gains_q16, n, dev)
    d_frames = as_dev(frames, torch.uint8)
    d_poses = torch.from_numpy(np.ascontiguousarray(np.concatenate([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3]], axis=1))).to(dev)
    ctx = _context(ctx, dev)
    offsets, stats = _level(ctx, v, nv, f, nf, best, d_frames, n, h, w, K, d_poses, q, sweeps)
    return offsets, stats


def _level(ctx, v, nv, f, nf, best, d_frames, n, h, w, K, d_poses, q, sweeps):
    import torch
    offsets = torch.empty((nf, 3, 3), dtype=torch.float64, device=v.device)
    seams, most = ctypes.c_int64(0), ctypes.c_double(0.0)
    ctx.check(ctx.lib.hive_texture_level(ctx.handle, ptr(v), nv, ptr(f), nf, ptr(best), ptr(d_frames), n, h, w, ptr(K), ptr(d_poses), ptr(q), int(sweeps), ptr(offsets),
                                         ctypes.byref(seams), ctypes.byref(most)))
    return offsets, dict(seam_vertices=int(seams.value), sweeps=int(sweeps), max_offset=float(most.value))


def texture_mesh(mesh, frames, camera_matrix, camera_poses, masks=None, cell=8, depth_tolerance=0.05, near=0.05, ctx=None, buffers: RenderBuffers = None,
                 return_views=False, smoothness=0.0, cull_back_faces=False, return_stats=False, exposure=False, exposure_prior=0.01, levelling=False,
                 levelling_sweeps=64):
    """The mesh with a texture atlas filled from the frames: a dict with ``vertices`` (3F, 3) float64, ``faces`` (F, 3) int32, ``uv`` (3F, 2) float64 and ``texture``
    (Ht, Wt, 3) uint8 as device tensors -- the keys of a ``foreground.process_frame`` mesh, so ``render_mesh``, ``gltf.Scene.add_geometry`` and ``write_glb`` take it
    as it is.  With ``return_views`` also ``views`` int32 (F,): the frame each face was textured from, -1 for none.

    ``mesh``: a ``mesh.Mesh`` / trimesh, or a dict with ``vertices``, ``faces`` and ``vertex_colors`` (faces no view sees are filled from the vertex colours, so the
    whole mesh stays one textured primitive).  ``frames``: uint8 (n, H, W, 3), numpy or device (or a sequence of pictures of one size).  ``camera_matrix``: a
    ``CameraMatrix`` or a 3 x 3 array.  ``camera_poses``: (n, 7) rows (``pose_vec2mat``) or (n, 4, 4) world-to-camera matrices, as ``render_mesh`` takes one.
    ``masks``: (n, H, W), non-zero = do not use that pixel.  ``cell``: the side of an atlas block (two faces) in texels.  ``depth_tolerance``: how far behind the
    rendered surface a vertex may lie and still count as seen (a parameter default: 5 cm for a scene in metres); ``near``: ``render_mesh``'s.  Each face takes the
    view in which its exact snapped area is largest; on equal area the lower index.  There is no blending.

    ``smoothness`` (px^2, default 0): the projected area a face may give up to remove one seam edge, i.e. an edge whose two faces are textured from different
    views; the labels are then smoothed across edges (``hive_texture_smooth``) with ``seam_cost = llround(smoothness * 131072)``.  ``cull_back_faces``: a view
    counts for a face only where it sees the face's front (snapped area A < 0, this project's marching-cubes winding).  With both at their defaults the
    per-face selection above runs as it always did.  ``return_stats`` adds ``stats``: a dict of ``rounds``, ``label_changes``, ``seam_entries_before``,
    ``seam_entries_after`` and ``area_given_up_px2`` (None on the default path).  The table of areas takes 8 n F bytes of device memory.

    ``exposure``: one gain per key frame and channel, solved from the faces two views both see (``exposure_sums``, ``solve_gains`` with ``exposure_prior``), so that
    frames of different exposure or white balance agree before they are sampled.  ``levelling``: additive offsets that make the two sides of every remaining label
    change meet at the mean colour at the seam vertices and fade out inside each patch over ``levelling_sweeps`` Jacobi sweeps (``level_offsets``).  Both are off by
    default; ``exposure_prior=0.01`` and ``levelling_sweeps=64`` are parameter defaults, not measured optima.  When either is on the labels come from the table path
    (with ``smoothness=0`` and no culling: the same keys) and ``stats`` gains ``exposure`` = dict(``gains`` (n, 3) floats q / 65536, ``pair_counts`` (n, n),
    ``fallback_channels``) and / or ``levelling`` = dict(``seam_vertices``, ``sweeps``, ``max_offset``).  The samples take 6 n F bytes, the offsets 72 F.

    ValueError: a negative or non-finite ``exposure_prior``, ``levelling_sweeps`` outside [0, 4096], more than 256 frames with ``exposure``; an empty mesh, no frame or more than 65535, frames of mixed size, ``cell`` outside [6, 64], an atlas side above 16384, a mesh without vertex
    colours, face ids outside [0, V), a negative or non-finite ``smoothness`` (or one of 2^23 px^2 and more), n F >= 2^31 on the smoothing path."""
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
    if not (math.isfinite(smoothness) and smoothness >= 0):
        raise ValueError(f"smoothness must be finite and >= 0, got {smoothness}")
    seam_cost = int(math.floor(float(smoothness) * AREA_UNITS_PER_PX2 + 0.5))  # llround of a non-negative number (the product by 2^17 is exact)
    if seam_cost >= 2 ** 40:
        raise ValueError(f"smoothness {smoothness} px^2 is 2^23 px^2 or more")
    exposure, levelling, levelling_sweeps = bool(exposure), bool(levelling), int(levelling_sweeps)
    if not (math.isfinite(exposure_prior) and exposure_prior >= 0):
        raise ValueError(f"exposure_prior must be finite and >= 0, got {exposure_prior}")
    if not 0 <= levelling_sweeps <= MAX_SWEEPS:
        raise ValueError(f"levelling_sweeps {levelling_sweeps} outside [0, {MAX_SWEEPS}]")
    if exposure and n > MAX_EXPOSURE_VIEWS:
        raise ValueError(f"{n} frames: exposure gains take at most {MAX_EXPOSURE_VIEWS}")
    adjusting = exposure or levelling
    smoothing = seam_cost > 0 or bool(cull_back_faces) or adjusting  # (the table path; with seam_cost 0 and no culling it leaves select's keys)
    if smoothing and n * nf >= 2 ** 31:
        raise ValueError(f"{n} frames x {nf} faces: the table of areas must stay below 2^31 entries")

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
    area = torch.empty((n, nf), dtype=torch.int64, device=dev) if smoothing else None
    samples = torch.empty((n, nf, 3), dtype=torch.int16, device=dev) if exposure else None  # (the bits of uint16 words)
    for k in range(n):
        R, t = np.ascontiguousarray(poses[k, :3, :3]), np.ascontiguousarray(poses[k, :3, 3])
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
        ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), h, w, float(near), ptr(xy), ptr(z), ptr(large), ptr(counts),
                                       ptr(buffers.key)))
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, None, None, ptr(depth), None))
        if smoothing:
            ctx.check(lib.hive_texture_vote(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), ptr(None if d_masks is None else d_masks[k]), h, w, k,
                                            float(depth_tolerance), 1 if cull_back_faces else 0, ptr(area)))
            if exposure:
                ctx.check(lib.hive_texture_samples(handle, ptr(f), nf, nv, ptr(xy), ptr(area), ptr(d_frames[k]), h, w, k, ptr(samples)))
            continue
        ctx.check(lib.hive_texture_select(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), ptr(None if d_masks is None else d_masks[k]), h, w, k,
                                          float(depth_tolerance), ptr(best)))
    stats = None
    if smoothing:
        offsets, neighbours = face_neighbours(f, nv, ctx=ctx)
        best, counts = smooth_labels(area, offsets, neighbours, seam_cost, ctx=ctx)
        stats = {name: int(value) for name, value in zip(STATS, counts)}
        stats["area_given_up_px2"] = stats["area_given_up_px2"] / AREA_UNITS_PER_PX2
    out = dict(vertices=torch.empty((3 * nf, 3), dtype=torch.float64, device=dev), faces=torch.empty((nf, 3), dtype=torch.int32, device=dev),
               uv=torch.empty((3 * nf, 2), dtype=torch.float64, device=dev), texture=torch.empty((ht, wt, 3), dtype=torch.uint8, device=dev))
    views = torch.empty(nf, dtype=torch.int32, device=dev) if return_views else None
    ctx.check(lib.hive_texture_unweld(handle, ptr(v), nv, ptr(f), nf, int(cell), ptr(best), ptr(out["vertices"]), ptr(out["faces"]), ptr(out["uv"]), ptr(views)))
    if adjusting:
        q, fallback = np.full((n, 3), UNIT_GAIN, np.uint32), []
        if exposure:
            G, D, N = exposure_sums(samples, ctx=ctx)
            q, fallback = solve_gains(G, D, float(exposure_prior))
            stats["exposure"] = dict(gains=q.astype(np.float64) / 65536.0, pair_counts=N, fallback_channels=fallback)
        d_q = _gains_on(q, n, dev)
        if levelling:
            offsets, stats["levelling"] = _level(ctx, v, nv, f, nf, best, d_frames, n, h, w, K, d_poses, d_q, levelling_sweeps)
        else:
            offsets = torch.zeros((nf, 3, 3), dtype=torch.float64, device=dev)
        ctx.check(lib.hive_texture_fill_adjusted(handle, ptr(v), nv, ptr(c), ptr(f), nf, ptr(best), ptr(d_frames), n, h, w, ptr(K), ptr(d_poses), float(near),
                                                 int(cell), ptr(d_q), ptr(offsets), ptr(out["texture"])))
    else:
        ctx.check(lib.hive_texture_fill(handle, ptr(v), nv, ptr(c), ptr(f), nf, ptr(best), ptr(d_frames), n, h, w, ptr(K), ptr(d_poses), float(near), int(cell),
                                        ptr(out["texture"])))
    if return_views:
        out["views"] = views
    if return_stats:
        out["stats"] = stats
    return out
