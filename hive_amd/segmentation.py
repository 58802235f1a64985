"""Instance masks of what moved: every frame's depth against a ray cast of the fused static model, on the GPU (csrc/segment.hip; the rules `motion`,
`open` and `label` are in include/hive_mi355x.h).

The reference takes its masks from detectron2's Mask R-CNN (hive/io.py:163-230), which is absent here.  This is a rule of this project, not that network, and
it is not pinned against it: it finds what moved, not persons.  A pixel whose live surface lies well in front of what the static model shows along the same ray
belongs to something that moved; the set pixels are opened (small specks go) and the connected components that are large enough become the objects.  The format
is the reference's: uint8, 0 = background, 1 .. k = objects, ids per frame and not tracked over time (io.py:214-218)."""
import logging
import math
import os
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr

MAX_BATCH_FRAMES = 32768  # frames per library call (the frame index is a 16-bit grid dimension)


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _device_frames(a, dtype, ctx, what):
    """``a`` (numpy array or tensor; one picture or a batch) as a contiguous device tensor (n, H, W) of ``dtype``, whether it was one picture, the context."""
    import torch
    if _is_torch(a):
        t = a
    else:
        dev = torch.device("cuda", ctx.device if ctx is not None else torch.cuda.current_device())
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    if t.ndim not in (2, 3):
        raise ValueError(f"{what}: one picture (H, W) or a batch (n, H, W), got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.cuda()
    single = t.ndim == 2
    t = (t[None] if single else t).to(dtype).contiguous()
    if min(t.shape) < 1:
        raise ValueError(f"{what}: empty shape {tuple(t.shape)}")
    return t, single, _lib.context_for(ctx, t.device)


def _batches(n):
    return [(a, min(n, a + MAX_BATCH_FRAMES)) for a in range(0, n, MAX_BATCH_FRAMES)]


def motion_mask(live_depth, model_depth, min_difference=0.05, relative_difference=0.0, ctx=None):
    """Rule `motion` alone (``hive_motion_mask``): uint8 0 / 1 device tensor of the depths' shape."""
    import torch
    live, single, ctx = _device_frames(live_depth, torch.float32, ctx, "live_depth")
    model, _, _ = _device_frames(model_depth, torch.float32, ctx, "model_depth")
    if live.shape != model.shape:
        raise ValueError(f"live depth {tuple(live.shape)} and model depth {tuple(model.shape)} differ in shape")
    n, h, w = (int(v) for v in live.shape)
    out = torch.empty((n, h, w), dtype=torch.uint8, device=live.device)
    for a, b in _batches(n):
        ctx.check(ctx.lib.hive_motion_mask(ctx.handle, ptr(live[a:b]), ptr(model[a:b]), b - a, h, w, float(min_difference), float(relative_difference), ptr(out[a:b])))
    return out[0] if single else out


def open_mask(mask, iterations=1, ctx=None):
    """Rule `open` alone (``hive_mask_open``): ``iterations`` 3 x 3 erosions, then as many dilations; uint8 device tensor of the mask's shape."""
    import torch
    m, single, ctx = _device_frames(mask, torch.uint8, ctx, "mask")
    n, h, w = (int(v) for v in m.shape)
    out = torch.empty_like(m)
    for a, b in _batches(n):
        ctx.check(ctx.lib.hive_mask_open(ctx.handle, ptr(m[a:b]), b - a, h, w, int(iterations), ptr(out[a:b])))
    return out[0] if single else out


def label_components(mask, connectivity=8, min_area=0, dtype=None, return_areas=False, ctx=None):
    """Connected components of ``mask != 0`` (rule `label`, ``hive_label_components``), numbered 1 .. k in ascending order of their first pixel in raster order
    (``scipy.ndimage.label``'s order) after components of fewer than ``min_area`` pixels are removed.

    ``mask``: one picture (H, W) or a batch (n, H, W), numpy array or device tensor.  ``dtype``: ``torch.int32`` (the default; any number of components, nothing
    synchronises) or ``torch.uint8`` (more than 255 components in a frame raise ``HiveError`` with the frame and the count).  Returns device tensors
    ``(labels, counts)`` -- ``counts`` int32 (n,), or a 0-d tensor for one picture -- and with ``return_areas`` also ``areas`` int32 (n, capacity): the area of
    component j at j - 1, zeros behind the count; the capacity is ceil(H W / 2), which no mask exceeds, or ``return_areas`` itself when it is an int above 1."""
    import torch
    dtype = dtype or torch.int32
    if dtype not in (torch.int32, torch.uint8):
        raise ValueError(f"label_components: dtype {dtype} (torch.int32 or torch.uint8)")
    m, single, ctx = _device_frames(mask, torch.uint8, ctx, "mask")
    n, h, w = (int(v) for v in m.shape)
    labels = torch.empty((n, h, w), dtype=dtype, device=m.device)
    counts = torch.empty((n,), dtype=torch.int32, device=m.device)
    capacity = 0
    if return_areas:
        capacity = int(return_areas) if not isinstance(return_areas, bool) and int(return_areas) > 1 else (h * w + 1) // 2
    areas = torch.empty((n, capacity), dtype=torch.int32, device=m.device) if capacity else None
    for a, b in _batches(n):
        ctx.check(ctx.lib.hive_label_components(ctx.handle, ptr(m[a:b]), b - a, h, w, int(connectivity), int(min_area), 1 if dtype == torch.uint8 else 4,
                                                ptr(labels[a:b]), ptr(counts[a:b]), ptr(areas[a:b]) if capacity else None, capacity))
    out = (labels[0], counts[0]) if single else (labels, counts)
    if return_areas:
        out += (areas[0] if single else areas,)
    return out


@dataclass
class MotionSegmentationOptions:
    """The parameters of ``motion_masks``.  The defaults are parameter defaults, not measured quantities: 5 cm for depths in metres, and 1 % of the frame as
    in ``foreground.process_frame``'s coverage rule (a smaller object would be dropped there anyway).

    :param min_difference: metres the live surface must lie in front of the model's.
    :param relative_difference: the same as a share of the model's depth; the larger of the two thresholds counts (sensor noise grows with depth).
    :param opening_iterations: 3 x 3 erosions, then as many dilations, of the raw mask (0 .. 16).
    :param min_area_share: components below ``ceil(min_area_share * H * W)`` pixels are removed.
    :param connectivity: 8 or 4.
    """
    min_difference: float = 0.05
    relative_difference: float = 0.0
    opening_iterations: int = 1
    min_area_share: float = 0.01
    connectivity: int = 8

    def __post_init__(self):
        if not (math.isfinite(self.min_difference) and self.min_difference >= 0 and math.isfinite(self.relative_difference) and self.relative_difference >= 0):
            raise ValueError(f"min_difference = {self.min_difference}, relative_difference = {self.relative_difference}: finite and not negative")
        if not 0 <= int(self.opening_iterations) <= 16:
            raise ValueError(f"opening_iterations = {self.opening_iterations}: 0 .. 16")
        if not 0.0 <= self.min_area_share <= 1.0:
            raise ValueError(f"min_area_share = {self.min_area_share}: 0 .. 1")
        if self.connectivity not in (4, 8):
            raise ValueError(f"connectivity = {self.connectivity}: 4 or 8")

    def min_area(self, height, width):
        """``ceil(min_area_share * H * W)``: the one place this is computed."""
        return int(math.ceil(self.min_area_share * (int(height) * int(width))))


def motion_masks(live_depth, model_depth, options=None, ctx=None):
    """Instance ids of what moved (``hive_motion_segment``: `motion`, `open`, `label` in one call): ``live_depth`` and ``model_depth`` float32 (n, H, W) or (H, W) in
    metres, 0 = invalid, numpy or device.  Returns device tensors ``(ids uint8 (n, H, W), counts int32 (n,))``; a frame with more than 255 objects raises
    ``HiveError`` with the frame and the count."""
    import torch
    options = options or MotionSegmentationOptions()
    live, _, ctx = _device_frames(live_depth, torch.float32, ctx, "live_depth")
    model, _, _ = _device_frames(model_depth, torch.float32, ctx, "model_depth")
    if live.shape != model.shape:
        raise ValueError(f"live depth {tuple(live.shape)} and model depth {tuple(model.shape)} differ in shape")
    n, h, w = (int(v) for v in live.shape)
    min_area = options.min_area(h, w)
    ids = torch.empty((n, h, w), dtype=torch.uint8, device=live.device)
    counts = torch.empty((n,), dtype=torch.int32, device=live.device)
    for a, b in _batches(n):
        ctx.check(ctx.lib.hive_motion_segment(ctx.handle, ptr(live[a:b]), ptr(model[a:b]), b - a, h, w, float(options.min_difference),
                                              float(options.relative_difference), int(options.opening_iterations), int(options.connectivity), min_area, ptr(ids[a:b]),
                                              ptr(counts[a:b])))
    return ids, counts


SegmentationResult = namedtuple("SegmentationResult", ["masks", "counts", "volume"])


def segment_dataset(dataset, options=None, mesh_options=None, num_frames=-1, chunk_frames=None, write=True, png_encoder="host"):
    """Instance masks for a HIVE folder whose masks are empty: the frames are fused into one static model (``fusion.tsdf_fusion`` with nothing masked; an
    object that crosses the scene is seen as free space by most frames and does not survive the averaging), the model is ray cast from every frame's pose, and
    ``motion_masks`` compares the frame's depth with it, in chunks of ``chunk_frames`` frames that stay on the device.

    With ``write``, ``mask/%06d.png`` of the folder is replaced (8-bit gray; ``png_encoder`` "host" = Pillow, "gpu" = ``hive_amd.png``); open the folder again
    (``HiveDataset(path)``) to see the new masks.  Returns ``SegmentationResult(masks uint8 device tensor (n, H, W), counts int32 device tensor (n,), volume)``."""
    import torch
    from hive_amd import fusion, png
    png.check_encoder(png_encoder)
    options = options or MotionSegmentationOptions()
    n = dataset.num_frames if num_frames == -1 else min(int(num_frames), dataset.num_frames)
    frame_set = list(range(n))
    chunk_frames = int(chunk_frames or fusion.CHUNK_FRAMES)
    _, volume = fusion.tsdf_fusion(dataset, mesh_options, frame_set=frame_set, return_volume=True, chunk_frames=chunk_frames)
    masks, counts = [], []
    for a, frames in zip(range(0, n, chunk_frames), fusion.frame_chunks(dataset, frame_set, False, chunk_frames, with_color=False)):
        size = tuple(int(v) for v in frames.depth.shape[1:])
        model = torch.stack([volume.raycast(dataset.camera_matrix, pose, size) for pose in frames.poses])
        ids, k = motion_masks(frames.depth, model, options)
        masks.append(ids)
        counts.append(k)
        if write:
            names = [os.path.join(dataset.base_path, dataset.mask_folder, dataset.index_to_filename(a + j)) for j in range(len(frames))]
            if png_encoder == "gpu":
                for name, data in zip(names, png.encode([ids[j] for j in range(len(names))])):
                    png.write_file(name, data)
            else:
                from PIL import Image
                for name, picture in zip(names, ids.cpu().numpy()):
                    Image.fromarray(picture).save(name)
    masks, counts = torch.cat(masks), torch.cat(counts)
    logging.info("Motion segmentation: %d of %d frames hold an object.", int((counts > 0).sum()), n)
    return SegmentationResult(masks, counts, volume)
