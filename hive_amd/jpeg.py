"""Baseline JPEG on the device: ``encode`` / ``encode_to_device`` over csrc/jpeg.hip (``hive_jpeg_layout`` / ``hive_jpeg_encode``: a batch of pictures of
different sizes in seven launches, the rules in include/hive_mi355x.h).  The bytes are the ones Pillow writes with ``quality=q, subsampling=s, optimize=False,
restart_marker_rows=1``; tests/jpeg_restatement.py restates them in numpy.  The reference has no such step: its glTF textures are PNG.
"""
import numpy as np

from hive_amd import _lib, _pictures

SUBSAMPLINGS = tuple(_lib.JPEG_SUBSAMPLING)


def check_settings(quality, subsampling):
    """ValueError unless ``quality`` is an integer of 1 .. 100 and ``subsampling`` one of "4:4:4", "4:2:0"."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality {quality!r}: an integer of 1 .. 100")
    if subsampling not in _lib.JPEG_SUBSAMPLING:
        raise ValueError(f"JPEG subsampling {subsampling!r} is not one of {SUBSAMPLINGS}")


def _check_picture(k, image):
    dtype = str(image.dtype).replace("torch.", "")
    if dtype != "uint8" or len(image.shape) != 3 or image.shape[2] != 3:
        raise ValueError(f"picture {k}: an (H, W, 3) uint8 array or tensor, got {dtype} {tuple(image.shape)}")
    if not (1 <= image.shape[0] <= 65535 and 1 <= image.shape[1] <= 65535):
        raise ValueError(f"picture {k}: {image.shape[0]} x {image.shape[1]} (sides of 1 .. 65535)")


def layout(shapes, subsampling="4:2:0"):
    """(offsets, total) of ``hive_jpeg_layout`` for pictures of these (H, W): the worst-case bound of every file.  Host only."""
    if subsampling not in _lib.JPEG_SUBSAMPLING:
        raise ValueError(f"JPEG subsampling {subsampling!r} is not one of {SUBSAMPLINGS}")
    table = (_lib.JpegImage * max(len(shapes), 1))()
    for row, (h, w) in zip(table, shapes):
        row.height, row.width, row.pitch = int(h), int(w), 3 * int(w)
    offsets, total = np.zeros(max(len(shapes), 1), np.int64), _lib.c_int64(0)
    _lib.check(_lib.load().hive_jpeg_layout(table, len(shapes), _lib.JPEG_SUBSAMPLING[subsampling], _lib.ptr(offsets), total))
    return offsets[:len(shapes)], int(total.value)


def encode_to_device(images, quality=90, subsampling="4:2:0", ctx=None):
    """(packed uint8 device tensor, offsets, sizes) of a list of (H, W, 3) uint8 pictures (device tensors, or host arrays, which are uploaded as they are): file
    ``k`` is ``packed[offsets[k]:offsets[k] + sizes[k]]``.  A device tensor may be a row-pitched view (a crop of a larger picture) as long as its pixels are
    contiguous."""
    import torch
    check_settings(quality, subsampling)
    images = list(images)
    if not images:
        raise ValueError("no pictures to encode")
    for k, image in enumerate(images):
        _check_picture(k, image)
    ctx = ctx or _lib.default_context()
    ctx.follow_torch_stream()
    dev = torch.device("cuda", ctx.device)
    keep, table = [_pictures.device_rows(image, dev, (3, 1)) for image in images], (_lib.JpegImage * len(images))()
    for row, t in zip(table, keep):
        row.data, row.height, row.width, row.pitch = t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)
    n, code = len(images), _lib.JPEG_SUBSAMPLING[subsampling]
    offsets, total, sizes = np.zeros(n, np.int64), _lib.c_int64(0), np.zeros(n, np.int64)
    _lib.check(ctx.lib.hive_jpeg_layout(table, n, code, _lib.ptr(offsets), total))
    out = torch.empty(total.value, dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.hive_jpeg_encode(ctx.handle, table, n, int(quality), code, out.data_ptr(), total.value, _lib.ptr(sizes)))
    return out, offsets, sizes


def encode(images, quality=90, subsampling="4:2:0", ctx=None):
    """The JPEG file of one (H, W, 3) uint8 picture as ``bytes``, or of a list of pictures as a list of ``bytes``: one encoder call and one download for all."""
    single = not isinstance(images, (list, tuple))
    files = _pictures.files_of(*encode_to_device([images] if single else images, quality, subsampling, ctx))
    return files[0] if single else files
