"""The motion segmentation without a GPU: the restatement (tests/segmentation_restatement.py) against hand-written expectations, the new entry points
declared, exported and bound, the host side of hive_amd.segmentation, and the CPU chain over the moving-sphere sequence (oracle volume -> restated ray cast ->
restated masks) against the analytic silhouette, with the figures printed before they are asserted."""
import ctypes
import os
import re

import numpy as np
import pytest

import segmentation_cases as sc
import segmentation_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hive_motion_mask", "hive_mask_open", "hive_label_components", "hive_motion_segment")


def test_label_restatement_by_hand():
    m = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 1],
                  [0, 0, 0, 0],
                  [1, 1, 0, 1]], np.uint8)
    lab8, k8, areas8 = sr.label(m, 8)
    assert k8 == 4 and areas8.tolist() == [2, 2, 2, 1]
    assert np.array_equal(lab8, [[1, 0, 0, 2], [0, 1, 0, 2], [0, 0, 0, 0], [3, 3, 0, 4]])
    lab4, k4, areas4 = sr.label(m, 4)
    assert k4 == 5 and areas4.tolist() == [1, 2, 1, 2, 1]
    assert np.array_equal(lab4, [[1, 0, 0, 2], [0, 3, 0, 2], [0, 0, 0, 0], [4, 4, 0, 5]])
    # the area filter comes before the numbering; an area equal to min_area stays
    lab, k, areas = sr.label(m, 4, min_area=2)
    assert k == 2 and areas.tolist() == [2, 2] and np.array_equal(lab, [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0], [2, 2, 0, 0]])
    assert sr.label(m, 4, min_area=3)[1] == 0
    # numbering follows the first pixel in raster order, not the order of discovery along a path: the U's root is its top LEFT end
    u = np.array([[1, 0, 1, 0, 1],
                  [1, 0, 1, 0, 0],
                  [1, 1, 1, 0, 0]], np.uint8)
    assert np.array_equal(sr.label(u, 4)[0], [[1, 0, 1, 0, 2], [1, 0, 1, 0, 0], [1, 1, 1, 0, 0]])


def test_open_restatement_by_hand():
    m = np.zeros((5, 6), np.uint8)
    m[0:3, 0:3] = 1      # a 3 x 3 block in the corner: the border takes no part, so it survives
    m[4, 5] = 1          # a speck in the opposite corner: its neighbours inside the picture are clear, so it goes
    m[2, 4] = 7
    want = np.zeros((5, 6), np.uint8)
    want[0:3, 0:3] = 1
    assert np.array_equal(sr.open_mask(m, 1), want)
    assert np.array_equal(sr.open_mask(m, 0), m)
    assert np.array_equal(sr.open_mask(m, 2), want)  # the 5 x 5 window of (0, 0) that lies inside the picture is the block itself
    inner = np.zeros((7, 7), np.uint8)
    inner[2:5, 2:5] = 1  # the same block away from the border: one erosion leaves its centre, two leave nothing
    assert np.array_equal(sr.open_mask(inner, 1), inner) and not sr.open_mask(inner, 2).any()
    assert sr.open_mask(np.ones((4, 4), np.uint8), 3).all()


def test_motion_restatement_by_hand():
    f = np.float32
    model = f(2.0)
    live = f(model - f(0.05))
    d = f(model - live)
    cases = [  # live, model, min_difference, relative_difference, set?
        (0.0, 2.0, 0.05, 0.0, 0), (1.0, 0.0, 0.05, 0.0, 0), (-1.0, 2.0, 0.05, 0.0, 0),   # invalid live depth, no model surface, negative depth
        (live, model, d, 0.0, 0), (live, model, np.nextafter(d, f(0)), 0.0, 1),          # exactly at the threshold; one ulp above it
        (live, model, 0.0, 0.5, 0), (live, model, 0.0, 0.01, 1), (live, model, 0.01, 0.026, 0),  # the relative term wins: 0.026 * 2 = 0.052 > 0.05
        (2.5, 2.0, 0.05, 0.0, 0), (np.nan, 2.0, 0.05, 0.0, 0), (1.0, np.inf, 0.0, 0.0, 0)]  # behind the model; not a number; a threshold that is not a number
    for live_, model_, a, b, want in cases:
        assert int(sr.motion_mask(np.array([[live_]], f), np.array([[model_]], f), a, b)[0, 0]) == want, (live_, model_, a, b)
    assert sr.min_area_of(0.01, 48, 64) == 31 and sr.min_area_of(0.01, 480, 640) == 3072 and sr.min_area_of(0.0, 5, 5) == 0


def test_case_pictures_are_what_their_names_say():
    th, tw = sc.TILE_H, sc.TILE_W
    assert sum(1 for h, w in sc.SIZES if h % th and w % tw and h > 1 and w > 1) >= 2 and any(h < th and w < tw for h, w in sc.SIZES)
    for h, w in sc.SIZES:
        pics = sc.pictures(h, w)
        for name, m in pics.items():
            if name.startswith("pair"):
                assert int((m != 0).sum()) == 2 and sr.label(m, 8)[1] == 1 and sr.label(m, 4)[1] == 2, name
        assert sr.label(pics["checkerboard"], 4)[1] == (h * w + 1) // 2
        assert sr.label(pics["checkerboard"], 8)[1] == (1 if min(h, w) > 1 else (h * w + 1) // 2)  # (one pixel thick: no diagonal to join along)
        for name in ("serpentine", "serpentine, columns", "spiral", "comb", "full"):
            assert sr.label(pics[name], 4)[1] == 1, name
        assert sr.label(pics["empty"], 8)[1] == 0
    big = sc.pictures(97, 131)
    assert {"pair corner \\", "pair corner /", "pair row edge \\", "pair column edge /"} <= set(big)
    assert (big["serpentine"] != 0).sum() > 97 * 131 // 2 and (big["spiral"] != 0).sum() > 97 * 131 // 3  # long chains through every tile


def test_entry_points_are_declared_exported_and_bound():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert int(re.search(r"#define HIVE_ABI_VERSION (\d+)", header).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().hive_abi_version()
    for rule in ("Rule `motion`", "Rule `open`", "Rule `label`"):
        assert rule in header


def test_segmentation_imports_without_a_gpu():
    import torch
    from hive_amd import segmentation as seg
    o = seg.MotionSegmentationOptions()
    assert (o.min_difference, o.relative_difference, o.opening_iterations, o.min_area_share, o.connectivity) == (0.05, 0.0, 1, 0.01, 8)
    assert o.min_area(48, 64) == 31 == sr.min_area_of(0.01, 48, 64) and o.min_area(480, 640) == 3072
    assert "not measured" in seg.MotionSegmentationOptions.__doc__
    for bad in (dict(connectivity=6), dict(opening_iterations=17), dict(min_difference=-1.0), dict(min_area_share=1.5), dict(relative_difference=float("nan"))):
        with pytest.raises(ValueError):
            seg.MotionSegmentationOptions(**bad)
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            seg.label_components(np.zeros((2, 2), np.uint8))


def test_convert_keeps_its_signature_and_gains_the_keyword():
    import inspect
    from hive_amd.dataset_adaptors import TUMAdaptor
    p = inspect.signature(TUMAdaptor.convert).parameters
    assert p["segment_motion"].default is False and list(p)[-1] == "segment_motion"
    assert "detectron2" in TUMAdaptor.convert.__doc__ and "segment_motion" in TUMAdaptor.convert.__doc__


def test_the_sequence_has_objects_and_empty_frames():
    """The condition that keeps the sequence tests honest, asserted about the truth."""
    truth = sc.sphere_sequence()["truth"]
    sizes = truth.reshape(len(truth), -1).sum(axis=1)
    print("silhouette pixels per frame:", sizes.tolist())
    assert len(truth) == 12 and (sizes >= 100).sum() >= 6 and (sizes == 0).sum() >= 2
    assert sizes.tolist() == [0, 0, 159, 478, 701, 665, 664, 692, 451, 138, 0, 0]


def test_cpu_chain_finds_the_sphere(oracle_lib):
    seq, chain = sc.sphere_sequence(), sc.cpu_chain(oracle_lib)
    truth, raw = seq["truth"], chain["raw"].astype(bool)
    wrong = [int((r != t).sum()) for r, t in zip(raw, truth)]
    print("raw rule at 0.05 m, pixels that differ from the truth per frame:", wrong)
    assert wrong == [0] * 12
    raw10 = np.stack([sr.motion_mask(l, m, 0.10) for l, m in zip(seq["live"], chain["model"])]).astype(bool)
    print("raw rule at 0.10 m, pixels that differ:", int((raw10 != truth).sum()))
    assert np.array_equal(raw10, truth)
    ids, counts = sr.motion_masks(seq["live"], chain["model"])
    found = ids != 0
    false_pos = [int((f & ~t).sum()) for f, t in zip(found, truth)]
    false_neg = [int((t & ~f).sum()) for f, t in zip(found, truth)]
    print("opened and labelled: objects per frame", counts.tolist(), "false positives", false_pos, "false negatives", false_neg)
    assert false_pos == [0] * 12
    assert max(false_neg) <= sc.OPENING_FALSE_NEGATIVES_MAX, "the constant records this measurement"
    assert counts.tolist() == [int(t.any()) for t in truth] and ids.max() == 1
