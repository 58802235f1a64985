"""``dilate_mask`` of /root/reference/hive/image_processing.py:30-45 on the MI355X, and the Telea inpainting that stands in for
``cv2.inpaint`` (hive/dataset_adaptors.py:506-511)."""
import numpy as np

from hive_amd import _lib
from hive_amd._lib import MEM_DEVICE, MEM_HOST, ptr
from hive_amd.options import MaskDilationOptions
from hive_amd.utils import validate_shape


def dilate_mask(mask, dilation_options: MaskDilationOptions):
    """Dilate an instance segmentation mask so that it covers a larger area.

    The reference runs ``cv2.dilate(mask, dilation_options.filter, iterations=num_iterations)``.  With the default 3x3 rectangle
    that equals one (2n+1) x (2n+1) box maximum with out-of-image pixels ignored (two separable launches); any other structuring
    element (``MaskDilationOptions(dilation_filter=...)``, /root/reference/hive/options.py:245-268) is iterated literally on the
    device with cv2's definition: anchor at the element's centre, taps outside the image ignored.

    :return: The dilated mask (bool).
    """
    mask = np.asarray(mask)
    validate_shape(mask, 'mask', expected_shape=(None, None))
    se = dilation_options.structuring_element()
    mask_u8 = np.ascontiguousarray(mask.astype(np.float32) != 0, dtype=np.uint8)
    out = np.empty_like(mask_u8)
    ctx = _lib.default_context()
    ctx.check(ctx.lib.hive_dilate_mask_se(ctx.handle, ptr(mask_u8), mask_u8.shape[0], mask_u8.shape[1], ptr(se), se.shape[0], se.shape[1],
                                          int(dilation_options.num_iterations), MEM_HOST, ptr(out)))
    return out.astype(bool)


def inpaint_telea(image, mask, radius=30, ctx=None):
    """Fill ``image`` under ``mask`` (non-zero = hole) with Telea's method in the level order of ``hive_inpaint_telea``
    (include/hive_mi355x.h states it to the bit; it is not cv2's heap order).

    ``image``: uint8 [H][W] or [H][W][3], or uint16 [H][W]; ``mask``: uint8 / bool [H][W].  numpy arrays go through host memory and
    give a numpy array; torch tensors on the GPU stay there and give a tensor.  A frame without a hole comes back unchanged; a frame
    without a known pixel, or a radius outside 2 .. 64, raises ``HiveError`` (``ERR_INVALID``)."""
    on_device = not isinstance(image, np.ndarray) and hasattr(image, "data_ptr")
    if on_device:
        import torch
        image = image.contiguous()
        mask = (mask != 0).to(torch.uint8).contiguous()
        assert image.is_cuda and mask.is_cuda and image.dtype in (torch.uint8, torch.uint16), "inpaint_telea: uint8 / uint16 tensors on the GPU"
        out = torch.empty_like(image)
        sample_bytes = image.element_size()
        ctx = ctx or _lib.default_context(image.device.index or 0)
    else:
        image = np.ascontiguousarray(image)
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert image.dtype in (np.uint8, np.uint16), f"inpaint_telea: uint8 or uint16 images, got {image.dtype}"
        out = np.empty_like(image)
        sample_bytes = image.dtype.itemsize
        ctx = ctx or _lib.default_context()
    assert image.ndim in (2, 3) and tuple(mask.shape) == tuple(image.shape[:2]), f"inpaint_telea: image {tuple(image.shape)} and mask {tuple(mask.shape)}"
    channels = 1 if image.ndim == 2 else int(image.shape[2])
    ctx.check(ctx.lib.hive_inpaint_telea(ctx.handle, ptr(image), int(image.shape[0]), int(image.shape[1]), channels, sample_bytes, ptr(mask), int(radius),
                                         MEM_DEVICE if on_device else MEM_HOST, ptr(out)))
    return out


def inpaint_frames(rgb, depth, mask, dilation=(5, 5, 5), radius=30, ctx=None, return_levels=False):
    """A batch of frames on the GPU (``hive_inpaint_frames``): ``rgb`` uint8 [n][H][W][3] and ``depth`` uint16 [n][H][W] torch tensors (either
    may be None), ``mask`` uint8 [n][H][W].  ``mask != 0`` is dilated ``dilation = (kh, kw, iterations)`` first (the reference: 5 x 5, 5 times;
    0 iterations: not at all); colour and depth share the mask, the levels and the weights.  Returns (rgb, depth), with ``return_levels`` also the
    level count of every frame."""
    import torch
    n, h, w = (int(v) for v in mask.shape)
    mask = mask.contiguous()
    assert mask.is_cuda and mask.dtype == torch.uint8, "inpaint_frames: a uint8 mask tensor on the GPU"
    rgb_out = depth_out = None
    if rgb is not None:
        rgb = rgb.contiguous()
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (n, h, w, 3), f"inpaint_frames: rgb {tuple(rgb.shape)} {rgb.dtype}"
        rgb_out = torch.empty_like(rgb)
    if depth is not None:
        depth = depth.contiguous()
        assert depth.dtype == torch.uint16 and tuple(depth.shape) == (n, h, w), f"inpaint_frames: depth {tuple(depth.shape)} {depth.dtype}"
        depth_out = torch.empty_like(depth)
    levels = np.zeros(n, np.int32)
    ctx = ctx or _lib.default_context(mask.device.index or 0)
    kh, kw, iterations = (int(v) for v in dilation)
    ctx.check(ctx.lib.hive_inpaint_frames(ctx.handle, ptr(rgb), ptr(depth), ptr(mask), n, h, w, kh, kw, iterations, int(radius), ptr(rgb_out), ptr(depth_out),
                                          ptr(levels)))
    return (rgb_out, depth_out, levels) if return_levels else (rgb_out, depth_out)
