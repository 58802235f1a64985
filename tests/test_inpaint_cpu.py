"""The inpainting specification's own known answers, on the numpy restatement (tests/inpaint_restatement.py), and the mode handling of
``dataset_adaptors.inpaint_frame_data``.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_restatement as R  # noqa: E402


@pytest.mark.parametrize("radius", [2, 5, 30])
def test_constant_and_ramp_come_back_exactly_on_interior_holes(radius):
    """A constant image and an integer ramp that does not wrap the type are fixed points on holes away from the border (the first-order term
    is exact where a one-sided difference exists); known pixels are never written; the weight sum stays positive."""
    mask = R.interior_holes()
    info = {}
    # the three channels of one call: a u8 ramp, a u8 constant, and random values (for the known-pixel check)
    image = np.stack([R.ramp(48, 64, np.uint8), np.full((48, 64), 201, np.uint8), R.random_image(48, 64, np.uint8, seed=3)], axis=2)
    out = R.inpaint(image, mask, radius, info)
    assert np.array_equal(out[:, :, 0], image[:, :, 0]) and np.array_equal(out[:, :, 1], image[:, :, 1])
    assert np.array_equal(out[mask == 0], image[mask == 0])
    assert not np.array_equal(out[:, :, 2], image[:, :, 2])  # the random channel was filled
    assert info["min_weight_sum"] > 0.0
    image16 = np.stack([R.ramp(48, 64, np.uint16), np.full((48, 64), 54321, np.uint16)], axis=2)  # (the restatement takes any channel count)
    assert np.array_equal(R.inpaint(image16, mask, radius), image16)


def test_levels():
    """Every hole pixel has an 8-neighbour of lower level; a disc of radius 11 has 12 levels; a row that is hole from side to side counts its
    levels up and down."""
    for mask in (R.interior_holes(), R.border_holes(), R.all_border_holes(), R.disc(48, 64, 24, 30, 11)):
        hole = mask != 0
        level = R.levels_of(hole, R.squared_distances(hole))
        assert (level[hole] >= 1).all() and (level[~hole] == 0).all()
        H, W = hole.shape
        padded = np.full((H + 2, W + 2), 1 << 30, np.int64)
        padded[1:-1, 1:-1] = level
        lowest = np.min([padded[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
        assert (lowest[hole] < level[hole]).all()
    info = {}
    R.inpaint(np.zeros((48, 64), np.uint8), R.disc(48, 64, 24, 30, 11), 2, info)
    assert info["level_count"] == 12
    hole = R.border_holes() != 0
    level = R.levels_of(hole, R.squared_distances(hole))
    assert level[20:23, 30].tolist() == [1, 2, 1]


def test_squared_distances_match_brute_force():
    rng = np.random.default_rng(5)
    hole = rng.random((13, 17)) < 0.6
    hole[4] = True  # a full row
    d2 = R.squared_distances(hole)
    v, u = np.mgrid[0:13, 0:17]
    for y in range(13):
        for x in range(17):
            other = hole != hole[y, x]
            assert d2[y, x] == ((v - y) ** 2 + (u - x) ** 2)[other].min()


def test_no_hole_copies_and_no_known_pixel_raises():
    image = R.random_image(5, 7, np.uint16)
    assert np.array_equal(R.inpaint(image, np.zeros((5, 7), np.uint8), 5), image)
    with pytest.raises(ValueError):
        R.inpaint(image, np.ones((5, 7), np.uint8), 5)
    with pytest.raises(ValueError):
        R.inpaint(image, np.zeros((5, 7), np.uint8), 1)


def test_inpaint_frame_data_mode_handling(tmp_path):
    """Off is a no-op (nothing is opened, nothing is written); the three modes with LaMa raise NotImplementedError naming LaMa."""
    from hive_amd.dataset_adaptors import DatasetAdaptor, inpaint_frame_data
    from hive_amd.options import InpaintingMode
    folder = tmp_path / "not_a_dataset"
    assert inpaint_frame_data(str(folder), InpaintingMode.Off) is None
    assert not folder.exists()
    for mode in (InpaintingMode.Lama_Image_CV2_Depth, InpaintingMode.CV2_Image_Lama_Depth, InpaintingMode.Lama_Image_Depth):
        with pytest.raises(NotImplementedError, match="LaMa"):
            inpaint_frame_data(str(folder), mode)
    assert not folder.exists()
    adaptor = DatasetAdaptor(str(tmp_path), str(folder))
    assert adaptor._inpaint_frame_data(InpaintingMode.Off) is None
    with pytest.raises(NotImplementedError, match="LaMa"):
        adaptor._inpaint_frame_data(InpaintingMode.Lama_Image_Depth)
