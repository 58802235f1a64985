"""Render meshes from a camera pose on the MI355X: the reference's ``render_mesh`` (/root/reference/scripts/experiments.py:861-883, pyrender with
``RenderFlags.FLAT``) as an exact z-buffer rasteriser (csrc/render.hip), and ``psnr`` to score a render against a frame (:835-852).

The rules -- camera frame, 8 sub-pixel bits, integer coverage with the top-left rule, the 64-bit depth | face key, perspective-correct unlit shading --
are stated in include/hive_mi355x.h above ``hive_render_clear`` and restated in numpy in tests/render_restatement.py; the kernels match that
restatement bit for bit."""
import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr
from hive_amd._pictures import is_torch as _is_torch
from hive_amd.geometric import CameraMatrix, pose_vec2mat


def _host(a):
    return a.detach().cpu().numpy() if _is_torch(a) else np.asarray(a)


class RenderBuffers:
    """Device scratch of ``render_mesh`` for one screen size, reused from call to call: the key plane (8 bytes a pixel) and, per mesh of the call, the
    projected vertices, the list of large faces and the two path counts (grown on demand, never shrunk)."""

    def __init__(self, height, width, device="cuda"):
        import torch
        self.shape = (int(height), int(width))
        self.device = torch.device(device)
        self.key = torch.empty(self.shape, dtype=torch.int64, device=self.device)  # (the bits of a uint64)
        self._slots = []
        self._used = 0

    def slot(self, k, nv, nf):
        """(xy int32 [nv][2], z float64 [nv], large int32 [nf], counts int32 [2]) of the call's k-th mesh."""
        import torch
        while len(self._slots) <= k:
            self._slots.append(None)
        s = self._slots[k]
        if s is None or s[0].shape[0] < nv or s[2].shape[0] < nf:
            room_v, room_f = max(nv, 0 if s is None else s[0].shape[0]), max(nf, 0 if s is None else s[2].shape[0])
            s = (torch.empty((room_v, 2), dtype=torch.int32, device=self.device), torch.empty(room_v, dtype=torch.float64, device=self.device),
                 torch.empty(room_f, dtype=torch.int32, device=self.device), torch.zeros(2, dtype=torch.int32, device=self.device))
            self._slots[k] = s
        self._used = max(self._used, k + 1)
        return s

    def path_counts(self):
        """(faces drawn by one thread each, faces drawn by one workgroup each) of the most recent ``render_mesh`` on these buffers, over all its meshes."""
        small = large = 0
        for s in self._slots[:self._used]:
            c = s[3].cpu().numpy()
            large, small = large + int(c[0]), small + int(c[1])
        return small, large


def _camera(camera_matrix, camera_pose, size):
    if isinstance(camera_matrix, CameraMatrix):
        K = camera_matrix.matrix
        if size is None:
            size = (camera_matrix.height, camera_matrix.width)
    else:
        K = _host(camera_matrix)
        if K.shape != (3, 3):
            raise ValueError(f"camera_matrix: a CameraMatrix or a 3 x 3 array, got shape {K.shape}")
        if size is None:
            raise ValueError("a 3 x 3 camera_matrix needs size=(height, width)")
    h, w = (int(v) for v in size)
    if h <= 0 or w <= 0:
        raise ValueError(f"empty size {h} x {w}")
    pose = _host(camera_pose).astype(np.float64)
    if pose.shape == (7,):
        pose = pose_vec2mat(pose)
    if pose.shape != (4, 4):
        raise ValueError(f"camera_pose: a 7-vector or a 4 x 4 world-to-camera matrix, got shape {pose.shape}")
    return (np.ascontiguousarray(K, dtype=np.float64), np.ascontiguousarray(pose[:3, :3], dtype=np.float64),
            np.ascontiguousarray(pose[:3, 3], dtype=np.float64).reshape(3), h, w)


def _device_of(meshes):
    """The device of the first mesh whose vertices are a device tensor, or None."""
    for mesh in meshes:
        v = mesh.get("vertices") if isinstance(mesh, dict) else getattr(mesh, "vertices", None)
        if _is_torch(v) and v.is_cuda:
            return v.device
    return None


def _mesh_arrays(mesh, dev):
    """None for a mesh the reference skips (:871), else device tensors (vertices f64, faces i32, colours u8 or None, uv f64 or None, texture u8 or None);
    copies only where the dtype, the device or the layout differ, and never writes to them."""
    import torch
    as_dev = lambda a, dt: (a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    if mesh is None:
        return None
    if isinstance(mesh, dict):
        vertices, faces = mesh.get("vertices"), mesh.get("faces")
        colors, uv, texture = mesh.get("vertex_colors"), mesh.get("uv"), mesh.get("texture")
    else:
        vertices, faces = mesh.vertices, mesh.faces
        colors, uv, texture = getattr(getattr(mesh, "visual", None), "vertex_colors", None), None, None
    if vertices is None or faces is None or len(vertices) == 0 or len(faces) == 0:
        return None
    v, f = as_dev(vertices, torch.float64), as_dev(faces, torch.int32)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"a mesh needs vertices (V, 3) and faces (F, 3), got {tuple(v.shape)} and {tuple(f.shape)}")
    if colors is not None:
        c = as_dev(colors, torch.uint8)
        if c.dim() != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4):
            raise ValueError(f"vertex colours (V, 3) or (V, 4), got {tuple(c.shape)}")
        return v, f, c[:, :3].contiguous(), None, None  # alpha dropped
    if uv is None or texture is None:
        raise ValueError("a mesh needs vertex colours, or uv and a texture")
    u, tex = as_dev(uv, torch.float64), as_dev(texture, torch.uint8)[:, :, :3].contiguous()
    if tuple(u.shape) != (v.shape[0], 2) or tex.dim() != 3 or tex.shape[0] == 0 or tex.shape[1] == 0:
        raise ValueError(f"uv (V, 2) and a texture (Ht, Wt, 3), got {tuple(u.shape)} and {tuple(tex.shape)}")
    return v, f, None, u, tex


def render_mesh(camera_matrix, camera_pose, *meshes, size=None, background=(255, 255, 255), near=0.05, return_depth=False, return_faces=False, ctx=None,
                buffers: RenderBuffers = None):
    """``render_mesh(camera_matrix, camera_pose, *meshes)`` of /root/reference/scripts/experiments.py:861-883: the meshes seen from a camera, unlit
    (``RenderFlags.FLAT``) on a white background, by the exact rasteriser of csrc/render.hip (rules: include/hive_mi355x.h, ``hive_render_clear``).

    ``camera_matrix``: a ``geometric.CameraMatrix`` (its width and height are the picture's size) or a 3 x 3 array with ``size=(H, W)``.  ``camera_pose``: the
    7-vector the reference passes (``pose_vec2mat``) or a 4 x 4 world-to-camera matrix.  The project's camera frame is used as it stands (x right, y down, z
    forward; the reference's flip to pyrender's OpenGL camera is not restated) and pixel (i, j) samples the screen point (j, i), ``world2image``'s convention.
    Each mesh: a ``mesh.Mesh`` / trimesh with ``visual.vertex_colors`` (alpha dropped), or a ``foreground.process_frame`` dict (``vertices``, ``faces``,
    ``uv`` in atlas coordinates, ``texture``; a dict with ``vertex_colors`` is taken as coloured).  ``None`` and empty meshes are skipped (:871).  Numpy arrays
    or device tensors; never modified.  Faces are numbered over all meshes in argument order; on equal float32 depth the smaller number wins.

    Returns the picture as a uint8 (H, W, 3) device tensor (the reference returns a PIL image); with ``return_depth`` / ``return_faces`` a tuple with the
    float32 depth (0 where nothing was hit) and / or the int32 global face index (-1 there) behind it.  ``near``: faces with a vertex nearer than this are
    dropped whole (no clipping).  ``buffers``: a ``RenderBuffers`` of the same size to reuse the scratch.  ValueError: ``near <= 0``, an empty size, face ids
    outside [0, V)."""
    import torch
    if not near > 0:
        raise ValueError(f"near must be > 0, got {near}")
    K, R, t, h, w = _camera(camera_matrix, camera_pose, size)
    bg = np.ascontiguousarray(background, dtype=np.uint8).reshape(3)
    dev = buffers.device if buffers is not None else _device_of(meshes) or torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or _lib.default_context(dev.index or 0)
    ctx.follow_torch_stream()
    buffers = buffers or RenderBuffers(h, w, dev)
    if buffers.shape != (h, w):
        raise ValueError(f"buffers were sized for {buffers.shape}, not {(h, w)}")
    drawn, base = [], 0
    for mesh in meshes:
        arrays = _mesh_arrays(mesh, dev)
        if arrays is None:
            continue
        lo, hi = torch.aminmax(arrays[1])
        if int(lo) < 0 or int(hi) >= arrays[0].shape[0]:
            raise ValueError(f"face ids {int(lo)} .. {int(hi)} outside [0, {arrays[0].shape[0]})")
        drawn.append((arrays, base))
        base += int(arrays[1].shape[0])
    if base >= 2 ** 31:
        raise ValueError(f"{base} faces: the face plane is int32")
    lib, handle = ctx.lib, ctx.handle
    buffers._used = 0
    color = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev) if return_depth else None
    face = torch.empty((h, w), dtype=torch.int32, device=dev) if return_faces else None
    ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
    slots = []
    for k, ((v, f, c, uv, tex), face_base) in enumerate(drawn):
        xy, z, large, counts = buffers.slot(k, v.shape[0], f.shape[0])
        slots.append((xy, z))
        ctx.check(lib.hive_render_draw(handle, ptr(v), v.shape[0], ptr(f), f.shape[0], face_base, ptr(K), ptr(R), ptr(t), h, w, float(near), ptr(xy), ptr(z),
                                       ptr(large), ptr(counts), ptr(buffers.key)))
    for ((v, f, c, uv, tex), face_base), (xy, z) in zip(drawn, slots):
        ht, wt = (0, 0) if tex is None else (int(tex.shape[0]), int(tex.shape[1]))
        ctx.check(lib.hive_render_shade(handle, v.shape[0], ptr(f), f.shape[0], face_base, ptr(xy), ptr(z), ptr(c), ptr(uv), ptr(tex), ht, wt, ptr(buffers.key),
                                        h, w, ptr(color)))
    ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, ptr(bg), ptr(color), ptr(depth), ptr(face)))
    extra = tuple(x for x in (depth, face) if x is not None)
    return (color, *extra) if extra else color


def psnr(a, b, mask=None):
    """Peak signal-to-noise ratio of two uint8 pictures, ``10 log10(255^2 / mse)`` in float64 (the score of experiments.py:835-852), over the pixels where
    ``mask`` is true when one is given.  A host helper on the colour values (device tensors are copied back); inf for identical pictures.  The reference's
    own scores -- SSIM and PSNR of the gray pictures, MS-SSIM, on the device -- are ``hive_amd.evaluation.image_similarity``."""
    x, y = _host(a).astype(np.float64), _host(b).astype(np.float64)
    if x.shape != y.shape:
        raise ValueError(f"shapes differ: {x.shape} and {y.shape}")
    if mask is not None:
        m = _host(mask).astype(bool)
        x, y = x[m], y[m]
    if x.size == 0:
        raise ValueError("no pixel to compare")
    mse = float(np.mean(np.square(x - y)))
    return float("inf") if mse == 0.0 else float(10.0 * np.log10(255.0 ** 2 / mse))
