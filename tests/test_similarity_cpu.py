"""The picture-score rules without a GPU: the restatement (tests/similarity_restatement.py) against a second formulation and against known answers, the mask rule,
and what hive_amd.evaluation declares and refuses before it touches a device."""
import json
import math
import os
import re

import numpy as np
import pytest

import similarity_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hive_similarity_ssim_psnr", "hive_similarity_msssim_level", "hive_similarity_finish", "hive_similarity_msssim_combine")


def _skimage_formulation(x, y):
    """structural_similarity(win_size=7) as skimage writes it: uniform_filter on float64 pictures, cropped by 3."""
    from scipy.ndimage import uniform_filter
    x, y = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: uniform_filter(a, size=7)
    cov_norm = 49 / 48
    ux, uy = f(x), f(y)
    uxx, uyy, uxy = f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S[3:-3, 3:-3]


@pytest.mark.parametrize("H,W", [(7, 7), (8, 9), (23, 37), (48, 64)])
def test_ssim_map_agrees_with_the_uniform_filter_formulation(H, W):
    """Within 1e-10 absolute: the float formulation's products reach 255^2 = 65025, one rounding there is 7e-12, under a denominator of at least C2 = 58.5.
    Measured: at most 2.7e-13 over the four sizes."""
    ref, est = SR.smooth_pair(H, W, seed=H)
    gr, ge = SR.gray(ref), SR.gray(est)
    S = SR.ssim_map(gr, ge)
    assert S.shape == (H - 6, W - 6) and S.dtype == np.float64
    worst = float(np.abs(S - _skimage_formulation(gr, ge)).max())
    print(f"{H} x {W}: largest difference {worst:.3g}")
    assert worst <= 1e-10


def test_constants_have_one_value_in_both_spellings():
    """(0.01 * 255) ** 2 of the original and the product the kernel writes are the same float64."""
    assert (0.01 * 255) ** 2 == (0.01 * 255) * (0.01 * 255) and (0.03 * 255) ** 2 == (0.03 * 255) * (0.03 * 255)
    assert 0.01 ** 2 == 0.01 * 0.01 and 0.03 ** 2 == 0.03 * 0.03


def test_identical_pictures():
    ref, _ = SR.smooth_pair(176, 208, seed=3)
    r = SR.compare(ref, ref)
    assert (r["map"] == 1.0).all() and r["ssim"] == 1.0 and r["sse"] == 0 and r["psnr"] == math.inf
    assert abs(SR.ms_ssim(ref, ref) - 1.0) <= 1e-12


@pytest.mark.parametrize("a,b", [(0, 0), (10, 200), (255, 254), (255, 255), (37, 37)])
def test_constant_pictures(a, b):
    x, y = np.full((9, 12), a, np.uint8), np.full((9, 12), b, np.uint8)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    S = SR.ssim_map(x, y)
    # both variances and the covariance are exactly 0 (uxx = a a exactly: 49 a a / 49), so C2 stands alone in both second factors: S is
    # (2ab + C1) / (a^2 + b^2 + C1) up to the two roundings of those products (S <= 1, one ulp is 1.1e-16)
    assert np.array_equal(S, np.full((3, 6), ((2.0 * a * b + C1) * C2) / ((a * a + b * b + C1) * C2)))
    assert np.abs(S - (2.0 * a * b + C1) / (a * a + b * b + C1)).max() <= 4e-16
    assert SR.sse(x, y) == 9 * 12 * (a - b) ** 2


def test_gray_known_answers():
    px = lambda *c: np.array([[c]], np.uint8)
    assert SR.gray(px(255, 255, 255))[0, 0] == 255 and SR.gray(px(0, 0, 0))[0, 0] == 0
    assert SR.gray(px(255, 255, 255), "rgb")[0, 0] == 255
    # (1868 * 200 + 9617 * 100 + 4899 * 50 + 8192) >> 14 = 1588442 >> 14 = 96;  (4899 * 200 + 9617 * 100 + 1868 * 50 + 8192) >> 14 = 2043092 >> 14 = 124
    assert 1868 * 200 + 9617 * 100 + 4899 * 50 + 8192 == 1588442 and 1588442 >> 14 == 96
    assert 4899 * 200 + 9617 * 100 + 1868 * 50 + 8192 == 2043092 and 2043092 >> 14 == 124
    assert SR.gray(px(200, 100, 50))[0, 0] == 96
    assert SR.gray(px(200, 100, 50), "rgb")[0, 0] == 124
    assert SR.gray(px(200, 100, 50), "bgr")[0, 0] == SR.gray(px(50, 100, 200), "rgb")[0, 0]


def test_mask_rule_is_per_channel():
    ref = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) + 10
    est = np.full((2, 3, 3), 99, np.uint8)
    est[0, 1] = (255, 7, 8)          # one channel white: only that channel of the frame is whitened
    est[1, 2] = (255, 255, 255)      # a background pixel: the whole pixel
    est[1, 0] = (1, 255, 255)
    before = ref.copy()
    masked = SR.mask_background(ref, est)
    assert np.array_equal(ref, before), "the frame itself is left alone"
    want = ref.copy()
    want[0, 1, 0] = 255
    want[1, 2] = 255
    want[1, 0, 1:] = 255
    assert np.array_equal(masked, want)
    assert masked[0, 1, 1] == ref[0, 1, 1] and masked[0, 1, 2] == ref[0, 1, 2], "a per-pixel rule would be another rule"
    # and it matters to the score
    r, e = SR.smooth_pair(12, 14, seed=5, whites=9)
    assert SR.compare(SR.mask_background(r, e), e)["sse"] != SR.compare(r, e)["sse"]


def test_ms_ssim_levels_of_the_noise_pair_stay_clear_of_the_relu():
    ref, est = SR.smooth_pair(161, 161, seed=1)
    score, levels = SR.ms_ssim(ref, est, return_levels=True)
    assert levels.shape == (5, 3) and levels.min() >= 0.5 and 0.5 < score < 1.0
    with pytest.raises(ValueError):
        SR.ms_ssim(ref[:160], est[:160])


def test_window_matches_the_package():
    from hive_amd import evaluation
    assert np.array_equal(evaluation.ms_ssim_window(), SR.ms_window()) and abs(SR.ms_window().sum() - 1.0) < 1e-15


def test_entry_points_are_declared():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int " + name + r"\(hive_ctx \*ctx,", header, flags=re.M), name
    assert _lib.ABI_VERSION >= 3
    assert "_obj/similarity.o" in open(os.path.join(ROOT, "hive_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments():
    """Without a context nothing runs; the library still answers with its error code."""
    from hive_amd import _lib
    lib = _lib.load()
    assert lib.hive_similarity_ssim_psnr(None, None, None, 1, 8, 8, 0, 1, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.hive_similarity_msssim_level(None, None, None, None, None, 1, 161, 161, 1, None, None, None, None) == _lib.ERR_INVALID
    assert lib.hive_similarity_finish(None, None, 1, 1, 1.0, None) == _lib.ERR_INVALID
    assert lib.hive_similarity_msssim_combine(None, None, 1, None) == _lib.ERR_INVALID


def test_image_similarity_refuses_before_it_needs_a_device():
    from hive_amd.evaluation import image_similarity
    a = np.zeros((16, 16, 3), np.uint8)
    cases = {
        "shapes differ": (a, np.zeros((16, 17, 3), np.uint8), {}),
        "batch sizes differ": (np.zeros((2, 16, 16, 3), np.uint8), np.zeros((3, 16, 16, 3), np.uint8), {}),
        "float pictures": (a.astype(np.float32), a.astype(np.float32), {}),
        "one float picture": (a, a.astype(np.float64), {}),
        "H below 7": (np.zeros((6, 16, 3), np.uint8), np.zeros((6, 16, 3), np.uint8), {}),
        "W below 7": (np.zeros((16, 6, 3), np.uint8), np.zeros((16, 6, 3), np.uint8), {}),
        "not three channels": (np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8), {}),
        "MS-SSIM at 160": (np.zeros((160, 200, 3), np.uint8), np.zeros((160, 200, 3), np.uint8), {"ms_ssim": True}),
        "channel order": (a, a, {"channel_order": "gbr"}),
    }
    for what, (ref, est, kw) in cases.items():
        with pytest.raises(ValueError):
            image_similarity(ref, est, **kw)
            pytest.fail(what)
    import torch
    with pytest.raises(ValueError):
        image_similarity(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))


def test_save_results_round_trips(tmp_path):
    from hive_amd.evaluation import NAN, save_results
    rows = [{"dataset": "fern", "camera_feed": 0, "config": "kinect", "ssim": 0.75, "psnr": 21.5, "lpips": NAN, "ssim_masked": 1.0, "psnr_masked": math.inf,
             "lpips_masked": NAN},
            {"dataset": "fern", "camera_feed": 1, "config": "kinect", "ssim": 0.5, "psnr": 18.25, "lpips": NAN, "ssim_masked": NAN, "psnr_masked": NAN,
             "lpips_masked": NAN, "ms_ssim": 0.625, "ms_ssim_masked": NAN}]
    path = tmp_path / "metrics.json"
    save_results(rows, str(path))
    back = json.load(open(path))
    assert isinstance(back, list) and len(back) == 2 and [list(b) for b in back] == [list(r) for r in rows]
    for got, want in zip(back, rows):
        for key, value in want.items():
            assert got[key] == value or (isinstance(value, float) and math.isnan(value) and math.isnan(got[key])), key
