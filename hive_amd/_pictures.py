"""The one place for "arrays or tensors in": what the wrappers around the library share.  ``is_torch`` (every module that takes either kind), ``device_of`` and
``on_device`` (evaluation.py, features.py: the device of a set of inputs, and an input brought there as a contiguous tensor behind the caller's own check and
error text), ``device_rows`` and ``files_of`` (the picture encoders jpeg.py and png.py: pictures in, packed files out).  The context that goes with a device is
``_lib.context_for``."""
import warnings

import numpy as np


def is_torch(x):
    return type(x).__module__.startswith("torch")


def device_of(*inputs):
    """The device of the first input that is a device tensor; torch's current device when every input is a host array (or None)."""
    import torch
    return next((a.device for a in inputs if is_torch(a) and a.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())


def on_device(a, dev, *, check=None, error=None, shape=None, dtype=None):
    """``a`` (a tensor, or a host array, which is uploaded; never modified) as a contiguous tensor on ``dev``, of ``dtype`` and reshaped to ``shape`` where
    given.  ``check(dtype name, shape)`` is asked first, about ``a`` as it came: where it says no, ValueError(``error(a)``), the caller's own words."""
    import torch
    if check is not None and not check(str(a.dtype).replace("torch.", ""), tuple(a.shape)):
        raise ValueError(error(a))
    if not is_torch(a):
        with warnings.catch_warnings():  # a read-only array is fine: it is only copied to the device
            warnings.simplefilter("ignore", UserWarning)
            a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.to(dev) if dtype is None else a.to(dev, dtype)
    return (a if shape is None else a.reshape(shape)).contiguous()


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
