"""PNG on the device: ``encode`` / ``encode_to_device`` over csrc/png.hip (``hive_png_layout`` / ``hive_png_encode``: a batch of gray 8, gray 16 and RGB 8 pictures
of different sizes in fourteen launches, the rules in include/hive_mi355x.h).  Lossless: any PNG reader gives back the input's pixels; the bytes are this encoder's
own (not zlib's) and the same on every run and in every batch; tests/png_restatement.py restates them in numpy.  The host encoders (Pillow / zlib) stay the default
of every caller: ``png_encoder="gpu"`` selects this one.
"""
import numpy as np

from hive_amd import _lib, _pictures

ENCODERS = ("host", "gpu")
KINDS = tuple(_lib.PNG_KIND)


def check_encoder(png_encoder):
    """ValueError unless ``png_encoder`` is "host" or "gpu"."""
    if png_encoder not in ENCODERS:
        raise ValueError(f"png_encoder {png_encoder!r} is not one of {ENCODERS}")


def write_file(path, data):
    """What a writer thread does with an encoded file."""
    with open(path, "wb") as f:
        f.write(data)


def kind_of(k, image):
    """"gray8" | "gray16" | "rgb8" of an (H, W) uint8 / uint16 or (H, W, 3) uint8 array or tensor; ValueError otherwise."""
    dtype, shape = str(image.dtype).replace("torch.", ""), tuple(image.shape)
    if dtype == "uint8" and len(shape) == 2:
        kind = "gray8"
    elif dtype == "uint16" and len(shape) == 2:
        kind = "gray16"
    elif dtype == "uint8" and len(shape) == 3 and shape[2] == 3:
        kind = "rgb8"
    else:
        raise ValueError(f"picture {k}: an (H, W) uint8 or uint16 or an (H, W, 3) uint8 array or tensor, got {dtype} {shape}")
    if not (1 <= shape[0] <= 65535 and 1 <= shape[1] <= 65535):
        raise ValueError(f"picture {k}: {shape[0]} x {shape[1]} (sides of 1 .. 65535)")
    return kind


def layout(shapes_and_kinds):
    """(offsets, total) of ``hive_png_layout`` for pictures of these ((H, W), kind): the all-stored bound of every file.  Host only."""
    n = len(shapes_and_kinds)
    table = (_lib.PngImage * max(n, 1))()
    for row, ((h, w), kind) in zip(table, shapes_and_kinds):
        row.height, row.width, row.kind = int(h), int(w), _lib.PNG_KIND[kind]
        row.pitch = int(w) * (1, 2, 3)[row.kind]
    offsets, total = np.zeros(max(n, 1), np.int64), _lib.c_int64(0)
    _lib.check(_lib.load().hive_png_layout(table, n, _lib.ptr(offsets), total))
    return offsets[:n], int(total.value)


def encode_to_device(images, ctx=None):
    """(packed uint8 device tensor, offsets, sizes) of a list of pictures (device tensors, or host arrays, which are uploaded as they are), kinds and sizes
    mixed freely: file ``k`` is ``packed[offsets[k]:offsets[k] + sizes[k]]``.  A device tensor may be a row-pitched view (a crop of a larger picture) as long as
    the pixels of a row are contiguous.  One encoder call: at most 2^27 bytes of rows (the library refuses more, naming the picture)."""
    import torch
    images = list(images)
    if not images:
        raise ValueError("no pictures to encode")
    kinds = [kind_of(k, image) for k, image in enumerate(images)]
    ctx = ctx or _lib.default_context()
    ctx.follow_torch_stream()
    dev = torch.device("cuda", ctx.device)
    keep = [_pictures.device_rows(image, dev, (3, 1) if kind == "rgb8" else (1,)) for image, kind in zip(images, kinds)]
    table = (_lib.PngImage * len(images))()
    for row, t, kind in zip(table, keep, kinds):
        row.pixels, row.height, row.width, row.kind = t.data_ptr(), t.shape[0], t.shape[1], _lib.PNG_KIND[kind]
        row.pitch = t.stride(0) * t.element_size()
    n = len(images)
    offsets, total, sizes = np.zeros(n, np.int64), _lib.c_int64(0), np.zeros(n, np.int64)
    _lib.check(ctx.lib.hive_png_layout(table, n, _lib.ptr(offsets), total))
    out = torch.empty(total.value, dtype=torch.uint8, device=dev)
    ctx.check(ctx.lib.hive_png_encode(ctx.handle, table, n, out.data_ptr(), total.value, _lib.ptr(sizes)))
    return out, offsets, sizes


def encode(images, ctx=None):
    """The PNG file of one picture as ``bytes``, or of a list of pictures as a list of ``bytes``: one encoder call and one download for all."""
    single = not isinstance(images, (list, tuple))
    files = _pictures.files_of(*encode_to_device([images] if single else images, ctx))
    return files[0] if single else files
