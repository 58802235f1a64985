"""The motion segmentation's rules (include/hive_mi355x.h, above hive_motion_mask) in numpy and scipy.ndimage, literally: what csrc/segment.hip must reproduce
exactly.  Nothing here has a tolerance: the motion rule is float32 with every operation rounded once, the rest is integers."""
import math

import numpy as np
from scipy import ndimage

f32 = np.float32
BOX = np.ones((3, 3), bool)
CROSS = ndimage.generate_binary_structure(2, 1)


def motion_mask(live, model, min_difference=0.05, relative_difference=0.0):
    """Rule `motion` -> uint8 0 / 1."""
    live, model = np.asarray(live, f32), np.asarray(model, f32)
    with np.errstate(all="ignore"):
        rel = f32(relative_difference) * model
        thr = np.where(f32(min_difference) > rel, f32(min_difference), rel).astype(f32)
        diff = model - live
        return ((live > 0) & (model > 0) & (diff > thr)).astype(np.uint8)


def open_mask(mask, iterations=1):
    """Rule `open` for one picture: erosions whose border counts as set, dilations whose border counts as clear, i.e. pixels outside take no part."""
    mask = np.asarray(mask)
    if iterations == 0:
        return mask.astype(np.uint8).copy()
    eroded = ndimage.binary_erosion(mask != 0, BOX, iterations=iterations, border_value=1)
    return ndimage.binary_dilation(eroded, BOX, iterations=iterations, border_value=0).astype(np.uint8)


def label(mask, connectivity=8, min_area=0):
    """Rule `label` for one picture -> (labels int32 (H, W), k, areas int64 (k,)): scipy's numbering (ascending first pixel in raster order), components below
    ``min_area`` removed, the rest renumbered in the same order."""
    assert connectivity in (4, 8)
    raw, k = ndimage.label(np.asarray(mask) != 0, structure=BOX if connectivity == 8 else CROSS)
    areas = np.bincount(raw.ravel(), minlength=k + 1)[1:]
    keep = areas >= min_area
    renumber = np.zeros(k + 1, np.int32)
    renumber[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return renumber[raw].astype(np.int32), int(keep.sum()), areas[keep]


def min_area_of(share, height, width):
    return int(math.ceil(share * (height * width)))


def motion_masks(live, model, min_difference=0.05, relative_difference=0.0, opening_iterations=1, min_area_share=0.01, connectivity=8):
    """The three rules composed over a batch -> (ids uint8 (n, H, W), counts (n,)); more than 255 objects in a frame is an error here as in the library."""
    live, model = np.asarray(live, f32), np.asarray(model, f32)
    ids, counts = np.zeros(live.shape, np.uint8), np.zeros(len(live), np.int32)
    for i in range(len(live)):
        raw = motion_mask(live[i], model[i], min_difference, relative_difference)
        lab, k, _ = label(open_mask(raw, opening_iterations), connectivity, min_area_of(min_area_share, *raw.shape))
        assert k <= 255
        ids[i], counts[i] = lab, k
    return ids, counts
