"""The LPIPS rules without a GPU: the restatement (tests/lpips_restatement.py) at its fixed points and against its float32 formulation, the weight spellings
hive_amd.evaluation.LPIPS reads and refuses, and what the module declares and does before it touches a device."""
import json
import math
import os
import re
import types

import numpy as np
import pytest

import lpips_restatement as LR
import similarity_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hive_lpips_create", "hive_lpips_destroy", "hive_lpips_layer", "hive_lpips_forward")
SIZES = [(31, 31), (35, 47), (48, 64), (67, 93), (120, 160)]

_cache = {}


def _model():
    from hive_amd.evaluation import LPIPS
    if "model" not in _cache:
        _cache["model"] = LPIPS.seeded(1)
    return _cache["model"]


def _pair(H, W):
    return SR.smooth_pair(H, W, seed=100 * H + W, whites=max(3, H * W // 40))


def test_input_table():
    """Known answers: byte 255 is 1.0 and byte 0 is -1.0 before the scaling layer; the table is float32 and increasing."""
    table = LR.input_table()
    assert table.shape == (3, 256) and table.dtype == np.float32 and (np.diff(table, axis=1) > 0).all()
    for k in range(3):
        assert table[k, 255] == (np.float32(1.0) - np.float32(LR.SHIFT[k])) / np.float32(LR.SCALE[k])
        assert table[k, 0] == (np.float32(-1.0) - np.float32(LR.SHIFT[k])) / np.float32(LR.SCALE[k])
    # byte 128: (128 / 255) * 2 - 1 = 1 / 255 in float64 up to rounding, then float32
    assert table[0, 128] == (np.float32((128 / 255) * 2.0 - 1.0) - np.float32(-.030)) / np.float32(.458)
    picture = np.array([[[0, 128, 255]]], np.uint8)
    assert np.array_equal(LR.scaled_input(picture)[0, 0], [table[0, 0], table[1, 128], table[2, 255]]), "channel k of the picture is channel k of the network"


def test_feature_sizes_and_the_smallest_picture():
    assert LR.feature_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert LR.feature_sizes(480, 640) == [(119, 159), (59, 79), (29, 39), (29, 39), (29, 39)]
    assert LR.feature_sizes(30, 31)[2][0] == 0, "30 rows leave nothing after the second pool"
    from hive_amd import evaluation
    assert evaluation.lpips_feature_sizes(67, 93) == LR.feature_sizes(67, 93) and evaluation.LPIPS_MIN_SIDE == 31
    maps = LR.features(_pair(31, 31)[0][None], _model())
    assert [m.shape for m in maps] == [(1, 7, 7, 64), (1, 3, 3, 192), (1, 1, 1, 384), (1, 1, 1, 256), (1, 1, 1, 256)]


def test_fixed_points_of_the_restatement():
    """Equal pictures give exactly 0; the score is symmetric in its arguments; the masked variant of an estimate with no 255 byte is the plain one."""
    model = _model()
    ref, est = _pair(35, 47)
    assert LR.score(ref, ref, model) == (0.0, [0.0] * 5)
    assert LR.score(ref, est, model) == LR.score(est, ref, model)
    dark = np.minimum(est, 254)
    assert np.array_equal(LR.mask_background(ref, dark), ref)
    assert LR.score(LR.mask_background(ref, dark), dark, model) == LR.score(ref, dark, model)
    assert LR.score(LR.mask_background(ref, est), est, model)[0] != LR.score(ref, est, model)[0]


def test_a_layer_score_ignores_the_scale_of_its_features():
    """Scaling every channel of a layer's two feature maps by a positive constant leaves that layer's score unchanged within rounding.  The 1e-10 in the two
    denominators is not scaled with them: a unit vector moves by at most 1e-10 / norm, the norms here are above 0.1 (asserted), and the two unit vectors are
    about sqrt(d) >= 0.03 apart (asserted), so d moves by less than 2 * 2 * 1e-9 / 0.03 < 2e-7 relative; float64 rounding is far below that.  A factor of 3
    rounds every float32 value once more (6e-8 relative, against the same 0.03): 1e-5."""
    model = _model()
    ref, est = _pair(48, 64)
    fa, fb = LR.features(ref[None], model, np.float32), LR.features(est[None], model, np.float32)
    for l in range(5):
        base = LR.layer_score(LR.distance_map(fa[l][0], fb[l][0], model.lin_w[l]))
        norms = np.sqrt((fa[l][0].astype(np.float64) ** 2).sum(-1))
        assert base >= 0.03 ** 2 * float(model.lin_w[l].mean()) and norms.min() > 0.1, (l, base, norms.min())
        for scale, tolerance in ((4.0, 2e-7), (0.5, 2e-7), (3.0, 1e-5)):
            scaled = LR.layer_score(LR.distance_map(np.float32(scale) * fa[l][0], np.float32(scale) * fb[l][0], model.lin_w[l]))
            print(f"layer {l}, factor {scale}: relative change {abs(scaled - base) / base:.3g}")
            assert abs(scaled - base) <= tolerance * base, (l, scale, scaled, base)


@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_agrees_with_its_float32_formulation(H, W):
    """The float64 restatement against the float32 torch-CPU operators arranged as the lpips package arranges them.  The two differ by float32 rounding in every
    convolution and in the tail; measured with seeded weights of this kind the score differed by at most 2.4e-7 relative and a layer score by at most 3e-6
    (here: 1.5e-7 and 1.2e-6).  Asserted at four times those distances: a different CPU sums its convolutions in another order."""
    model = _model()
    ref, est = _pair(H, W)
    for frame in (ref, LR.mask_background(ref, est)):
        s64, l64 = LR.score(frame, est, model)
        s32, l32 = LR.score_f32(frame, est, model)
        layer_distance = max(abs(a - b) / b for a, b in zip(l32, l64))
        print(f"{H} x {W}: score {s64!r}, float32 formulation off by {abs(s32 - s64) / s64:.3g} relative, a layer by at most {layer_distance:.3g}")
        assert 1e-3 < s64 < 1.0 and all(v > 0 for v in l64)
        assert abs(s32 - s64) / s64 <= 4 * 2.4e-7 and layer_distance <= 4 * 3e-6


def test_integer_rows_are_exact_in_float32_too():
    """The integer formulation of a row equals the same row computed by float32 operators: every partial sum is an integer below 2^24."""
    rng = np.random.default_rng(5)
    weights = types.SimpleNamespace(conv_w=[rng.integers(-2, 3, (cout, cin, k, k)).astype(np.float32) for cin, cout, k, _, _, _ in LR.LAYERS],
                                    conv_b=[rng.integers(-3, 4, cout).astype(np.float32) for _, cout, _, _, _, _ in LR.LAYERS])
    for index, (h, w) in enumerate(((31, 39), (16, 20), (17, 17), (5, 13), (1, 1))):
        x = rng.integers(-2, 3, (2, h, w, LR.LAYERS[index][0])).astype(np.float32)
        want = LR.layer_int(index, x, weights)
        assert want.dtype == np.float32 and np.array_equal(want, LR.layer(index, x, weights, np.float32))
    with pytest.raises(AssertionError):
        LR.layer_int(0, np.full((1, 31, 31, 3), 0.5, np.float32), weights)


def test_the_three_spellings_load_the_same_arrays():
    import torch
    from hive_amd.evaluation import LPIPS
    model = _model()
    whole = model.state_dict()
    assert sorted(whole)[:3] == ["lin0.model.1.weight", "lin1.model.1.weight", "lin2.model.1.weight"] and "net.slice3.6.bias" in whole
    noisy = dict(whole)  # what the package's own state dict carries besides
    noisy.update({"scaling_layer.shift": np.zeros((1, 3, 1, 1), np.float32), "scaling_layer.scale": np.ones((1, 3, 1, 1), np.float32)})
    noisy.update({f"lins.{l}.model.1.weight": -np.ones_like(whole[f"lin{l}.model.1.weight"]) for l in range(5)})
    index = (0, 3, 6, 8, 10)
    alexnet = {f"features.{index[l]}.{kind}": whole[f"net.slice{l + 1}.{index[l]}.{kind}"] for l in range(5) for kind in ("weight", "bias")}
    alexnet.update({"classifier.1.weight": np.zeros((4, 4), np.float32)})
    linear = {f"lin{l}.model.1.weight": torch.from_numpy(whole[f"lin{l}.model.1.weight"]) for l in range(5)}
    for loaded in (LPIPS.from_state_dict(whole), LPIPS.from_state_dict(noisy), LPIPS.from_state_dict(alexnet, linear),
                   LPIPS.from_state_dict({k: torch.from_numpy(v) for k, v in alexnet.items()}, linear)):
        for l in range(5):
            assert np.array_equal(loaded.conv_w[l], model.conv_w[l]) and np.array_equal(loaded.conv_b[l], model.conv_b[l])
            assert np.array_equal(loaded.lin_w[l], model.lin_w[l]) and loaded.lin_w[l].shape == (LR.LAYERS[l][1],) and loaded.conv_w[l].dtype == np.float32


def test_from_files(tmp_path):
    import torch
    from hive_amd.evaluation import LPIPS
    model = _model()
    whole = {k: torch.from_numpy(v) for k, v in model.state_dict().items()}
    torch.save(whole, tmp_path / "whole.pth")
    index = (0, 3, 6, 8, 10)
    torch.save({f"features.{index[l]}.{kind}": whole[f"net.slice{l + 1}.{index[l]}.{kind}"] for l in range(5) for kind in ("weight", "bias")}, tmp_path / "alexnet.pth")
    torch.save({k: v for k, v in whole.items() if k.startswith("lin")}, tmp_path / "alex.pth")
    for loaded in (LPIPS.from_files(str(tmp_path / "whole.pth")), LPIPS.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth"))):
        assert all(np.array_equal(a, b) for a, b in zip(loaded.conv_w + loaded.conv_b + loaded.lin_w, model.conv_w + model.conv_b + model.lin_w))
    with pytest.raises(ValueError, match="lin0.model.1.weight"):
        LPIPS.from_files(str(tmp_path / "alexnet.pth"))


def test_malformed_weights_raise_naming_the_key():
    from hive_amd.evaluation import LPIPS
    whole = _model().state_dict()
    without = lambda key: {k: v for k, v in whole.items() if k != key}
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.bias"):
        LPIPS.from_state_dict(without("net.slice2.3.bias"))
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        LPIPS.from_state_dict(without("net.slice1.0.weight"))
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        LPIPS.from_state_dict(without("lin4.model.1.weight"))
    with pytest.raises(ValueError, match=r"net\.slice3\.6\.weight.*shape"):
        LPIPS.from_state_dict({**whole, "net.slice3.6.weight": whole["net.slice3.6.weight"][:, :, :2]})
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight.*shape"):
        LPIPS.from_state_dict({**whole, "lin1.model.1.weight": whole["lin1.model.1.weight"].reshape(-1)})
    negative = whole["lin2.model.1.weight"].copy()
    negative[0, 5] = -1e-3
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*negative"):
        LPIPS.from_state_dict({**whole, "lin2.model.1.weight": negative})
    m = _model()
    with pytest.raises(ValueError, match=r"conv_b\[1\]"):
        LPIPS(m.conv_w, [m.conv_b[0], m.conv_b[1][:-1], *m.conv_b[2:]], m.lin_w)
    with pytest.raises(ValueError, match=r"lin_w\[0\].*negative"):
        LPIPS(m.conv_w, m.conv_b, [-m.lin_w[0] - 1, *m.lin_w[1:]])


def test_seeded_weights_repeat_and_differ_by_seed():
    from hive_amd.evaluation import LPIPS
    a, b, c = LPIPS.seeded(3), LPIPS.seeded(3), LPIPS.seeded(4)
    assert all(np.array_equal(x, y) for x, y in zip(a.conv_w + a.conv_b + a.lin_w, b.conv_w + b.conv_b + b.lin_w))
    assert not np.array_equal(a.conv_w[0], c.conv_w[0])
    for l, (cin, cout, k, _, _, _) in enumerate(LR.LAYERS):
        assert a.conv_w[l].shape == (cout, cin, k, k) and (a.lin_w[l] >= 0).all() and a.lin_w[l].max() < 4.0 / cout
        assert abs(a.conv_w[l].std() / math.sqrt(2.0 / (cin * k * k)) - 1) < 0.05


def test_the_model_refuses_before_it_needs_a_device():
    model = _model()
    ok = np.zeros((31, 31, 3), np.uint8)
    for ref, est in ((np.zeros((30, 40, 3), np.uint8),) * 2, (np.zeros((40, 30, 3), np.uint8),) * 2, (ok, np.zeros((31, 32, 3), np.uint8)),
                     (ok.astype(np.float32), ok.astype(np.float32)), (ok[..., :2], ok[..., :2])):
        with pytest.raises(ValueError):
            model(ref, est)


def test_compare_images_takes_only_this_modules_model(monkeypatch):
    """compare_images hands image_similarity the model when lpips_fn is an LPIPS of this module and nothing otherwise: a foreign object (the existing GPU test
    passes object()) and None give nan as before.  image_similarity is replaced: no device is needed."""
    from hive_amd import evaluation
    seen = []

    def fake(ref, est, **kw):
        seen.append(kw)
        one = np.array([0.5])
        return evaluation.SimilarityResult(ssim=one, psnr=one * 40, ms_ssim=one * np.nan, sse=np.array([3]), lpips=None if kw.get("lpips") is None else one / 2)

    monkeypatch.setattr(evaluation, "image_similarity", fake)
    a = np.zeros((31, 31, 3), np.uint8)
    for foreign in (None, object(), lambda x, y: 0.125):
        ssim, psnr, lpips = evaluation.compare_images(a, a, lpips_fn=foreign)
        assert (ssim, psnr) == (0.5, 20.0) and math.isnan(lpips) and seen[-1].get("lpips") is None
    model = _model()
    assert evaluation.compare_images(a, a, lpips_fn=model) == (0.5, 20.0, 0.25) and seen[-1]["lpips"] is model
    four = evaluation.compare_images(a, a, lpips_fn=model, return_mifd=True)
    assert four[:3] == (0.5, 20.0, 0.25) and math.isnan(four[3])
    r = evaluation.SimilarityResult(ssim=None, psnr=None, ms_ssim=None, sse=None)
    assert r.lpips is None and r.lpips_masked is None, "the new fields default to None: existing constructions keep working"


def test_save_results_keeps_finite_and_nan_lpips(tmp_path):
    from hive_amd.evaluation import NAN, save_results
    rows = [{"dataset": "fern", "camera_feed": 0, "config": "kinect", "ssim": 0.75, "psnr": 21.5, "lpips": 0.0078125, "ssim_masked": 1.0, "psnr_masked": math.inf,
             "lpips_masked": 0.00390625},
            {"dataset": "fern", "camera_feed": 1, "config": "kinect", "ssim": 0.5, "psnr": 18.25, "lpips": NAN, "ssim_masked": NAN, "psnr_masked": NAN, "lpips_masked": NAN}]
    path = tmp_path / "metrics.json"
    save_results(rows, str(path))
    back = json.load(open(path))
    assert [list(b) for b in back] == [list(r) for r in rows]
    assert back[0]["lpips"] == 0.0078125 and back[0]["lpips_masked"] == 0.00390625 and math.isnan(back[1]["lpips"]) and math.isnan(back[1]["lpips_masked"])


def test_entry_points_are_declared():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
    assert _lib.ABI_VERSION >= 4
    assert "_obj/lpips.o" in open(os.path.join(ROOT, "hive_amd", "csrc", "Makefile")).read()
    assert "not pinned against lpips" in header


def test_entry_points_refuse_without_a_model():
    """Without a model nothing runs; the library still answers with its error code."""
    from hive_amd import _lib
    lib = _lib.load()
    assert lib.hive_lpips_create(None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.hive_lpips_layer(None, 0, None, 1, 31, 31, None) == _lib.ERR_INVALID
    assert lib.hive_lpips_forward(None, None, None, 1, 31, 31, 1, None, None, None, None) == _lib.ERR_INVALID
    assert lib.hive_lpips_destroy(None) == _lib.OK
