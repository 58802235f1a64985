"""What the picture encoders' wrappers (jpeg.py, png.py) share: pictures in, packed files out."""
import numpy as np


def is_torch(x):
    return type(x).__module__.startswith("torch")


def device_rows(image, dev, inner):
    """``image`` (a tensor, or a host array, which is uploaded as it is) as a tensor on ``dev`` whose rows the library can read: the strides behind the first are
    ``inner`` (in elements) and rows do not overlap.  A row-pitched view stays as it is; anything else is re-laid contiguous."""
    import torch
    t = image if is_torch(image) else torch.from_numpy(np.ascontiguousarray(image))
    t = t.to(dev)
    if t.stride()[1:] != inner or t.stride(0) < t.shape[1] * inner[0]:
        t = t.contiguous()
    return t


def files_of(packed, offsets, sizes):
    """The files of a packed device buffer as a list of ``bytes``.  They fill a part of their bounds: joined on the device, only their bytes are downloaded, once."""
    import torch
    pieces = [packed[int(o):int(o + s)] for o, s in zip(offsets, sizes)]
    host = (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).cpu().numpy().tobytes()
    ends = np.cumsum(sizes)
    return [host[int(e - s):int(e)] for e, s in zip(ends, sizes)]
