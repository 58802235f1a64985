"""LPIPS on the GPU (csrc/lpips.hip behind hive_amd.evaluation.LPIPS) against the restatement of its rules (tests/lpips_restatement.py): every feature row bit for
bit on integer-valued data and within the float32 summation bound on real data, the distance maps bit for bit, the scores with the same bits in every batch and
run, the whole score against float64, and the Python surface."""
import math
import types
import warnings

import numpy as np
import pytest

import lpips_restatement as LR
import render_cases as C
import render_restatement as RR
import similarity_restatement as SR

pytestmark = pytest.mark.gpu

SIZES = [(31, 31), (35, 47), (48, 64), (67, 93), (120, 160)]

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _model(seed=1):
    from hive_amd.evaluation import LPIPS
    return _once(("model", seed), lambda: LPIPS.seeded(seed))


def _batch(H, W, n=3):
    """n seeded pairs of one size, each estimate with single channels at exactly 255 so that the masked variant differs; computed once, read-only."""
    def make():
        pairs = [SR.smooth_pair(H, W, seed=100 * H + W + k, whites=max(3, H * W // 40)) for k in range(n)]
        ref, est = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ref.setflags(write=False), est.setflags(write=False)
        return ref, est
    return _once(("batch", H, W, n), make)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- exact, per layer ----------------------------------------------------------------------------------------------------------------------------------------
# The convolution kernel's tile is 64 output pixels (the pictures' maps laid end to end) x 64 channels, over k chunks of 16.  Every C_out (64, 192, 384, 256) is a
# multiple of 64, so no channel tail exists; K = 363 of row 0 ends 11 values into its last chunk, every other K is a multiple of 16.  The sizes below give maps of
# 7 x 9 = 63, 8 x 8 = 64 and 5 x 13 = 65 pixels: one picture ends one pixel before, at, and one pixel after the tile edge, and three pictures (189, 192, 195) do
# the same at the third edge, with pictures 1 and 2 starting in the middle of a tile.  Then the smallest input with an output (1 x 1), the smallest legal picture
# (row 0: 31 x 31) and, for the rows behind a pool, inputs one larger than an odd size so that floor mode drops a row and a column (16 x 20 pools like 15 x 19).
# Widths 39, 35, 55, 19, 27, 9, 13, ... are no multiple of 4.
def _sizes_for(index):
    maps = [(7, 9), (8, 8), (5, 13)]
    if index == 0:
        return [(4 * h + 3, 4 * w + 3) for h, w in maps] + [(7, 7), (31, 31), (10, 9)]  # (10, 9): a 1 x 1 map from the largest such height
    if LR.LAYERS[index][5]:
        return [(2 * h + 1, 2 * w + 1) for h, w in maps] + [(3, 3), (16, 20), (4, 12)]
    return maps + [(1, 1), (3, 2)]


EXACT_CASES = [(index, h, w) for index in range(5) for h, w in _sizes_for(index)]


def _integer_model():
    """Integer weights in [-2, 2] and biases in [-3, 3]; channel 0 of every row has the bias -20000, below every sum (at most 4 * 3456): its pre-activation is
    negative everywhere and the ReLU gives exact zeros.  Every partial sum stays below 4 * 3456 + 20000 < 2^24."""
    def make():
        from hive_amd.evaluation import LPIPS
        rng = np.random.default_rng(7)
        conv_w = [rng.integers(-2, 3, (cout, cin, k, k)).astype(np.float32) for cin, cout, k, _, _, _ in LR.LAYERS]
        conv_b = [rng.integers(-3, 4, cout).astype(np.float32) for _, cout, _, _, _, _ in LR.LAYERS]
        for b in conv_b:
            b[0] = -20000.0
        return LPIPS(conv_w, conv_b, [np.ones(layer[1], np.float32) for layer in LR.LAYERS])
    return _once("integer model", make)


@pytest.mark.parametrize("index,h,w", EXACT_CASES)
def test_feature_rows_are_exact_on_integer_data(gpu_ctx, index, h, w):
    """hive_lpips_layer on integer-valued inputs in [-2, 2]: bit for bit the integer restatement, at N = 3 and N = 1; a picture's values do not depend on N."""
    import torch
    model = _integer_model()
    rng = np.random.default_rng(1000 * index + 10 * h + w)
    x = rng.integers(-2, 3, (3, h, w, LR.LAYERS[index][0])).astype(np.float32)
    want = LR.layer_int(index, x, model)
    assert (want[..., 0] == 0).all() and (want[..., 1:] > 0).any()
    got3 = model.layer(index, torch.from_numpy(x).cuda()).cpu().numpy()
    assert got3.shape == want.shape and got3.dtype == np.float32
    assert _bits(got3) == _bits(want), f"row {index}, {h} x {w}, N = 3: {int((got3 != want).sum())} values differ"
    got1 = model.layer(index, torch.from_numpy(x[1:2]).cuda()).cpu().numpy()
    assert _bits(got1) == _bits(want[1:2]), f"row {index}, {h} x {w}, N = 1: {int((got1 != want[1:2]).sum())} values differ"


# ---- the forward call: composition, the tail, reproducibility --------------------------------------------------------------------------------------------------
def _forward(H, W):
    """One masked forward call with every map, N = 3, seeded weights; shared by the tests below."""
    def make():
        ref, est = _batch(H, W)
        return _model()(ref, est, mask_background=True, return_maps=True)
    return _once(("forward", H, W), make)


def _sets(H, W):
    """The three picture sets of the batch as the forward call orders them: reference, masked reference, estimate -> uint8 (3, N, H, W, 3)."""
    ref, est = _batch(H, W)
    return np.stack([ref, np.stack([LR.mask_background(r, e) for r, e in zip(ref, est)]), est])


@pytest.mark.parametrize("H,W", SIZES)
def test_forward_is_the_chained_layers_and_the_stated_tail(gpu_ctx, H, W):
    """The forward's features equal the chained hive_lpips_layer calls on the table's values bit for bit (sets: reference, masked reference, estimate); from
    those features the five distance maps are bit for bit the numpy restatement, plain and masked; each layer score is within 1e-10 of fsum(map) / size; the pair
    score is the five layer scores added in order, with the same bits."""
    import torch
    model, got = _model(), _forward(H, W)
    sizes = LR.feature_sizes(H, W)
    x = torch.from_numpy(LR.scaled_input(_sets(H, W)).reshape(9, H, W, 3)).cuda()
    for l in range(5):
        x = model.layer(l, x)
        assert tuple(got.features[l].shape) == (3, 3, *sizes[l], LR.LAYERS[l][1])
        assert torch.equal(x.reshape(got.features[l].shape), got.features[l]), f"layer {l}"
    feats = [f.cpu().numpy() for f in got.features]
    for v, (scores, layers) in enumerate(((got.lpips, got.layers), (got.lpips_masked, got.layers_masked))):
        for k in range(3):
            total = None
            for l in range(5):
                want = LR.distance_map(feats[l][v, k], feats[l][2, k], model.lin_w[l])
                d = got.dist[l][v, k].cpu().numpy()
                assert d.shape == want.shape and _bits(d) == _bits(want), f"variant {v}, picture {k}, layer {l}: {int((d != want).sum())} values differ"
                mean = LR.layer_score(want)
                assert abs(layers[l, k] - mean) <= 1e-10, (v, k, l, layers[l, k], mean)
                total = layers[l, k] if total is None else total + layers[l, k]
            assert _bits(scores[k]) == _bits(total), (v, k)
    assert (got.lpips != got.lpips_masked).all(), "the mask must matter to these pairs"


@pytest.mark.parametrize("H,W", SIZES)
def test_scores_do_not_depend_on_the_batch_the_run_or_the_slot(gpu_ctx, H, W):
    """A picture's score has the same bytes at N = 1 and inside N = 3, and in two runs; model(x, x) is exactly 0.0; model(a, b) == model(b, a) bitwise; a plain
    call gives the plain scores of the masked call."""
    model, got = _model(), _forward(H, W)
    ref, est = _batch(H, W)
    again = model(ref, est, mask_background=True)
    assert again.features is None and again.dist is None
    for field in ("lpips", "lpips_masked", "layers", "layers_masked"):
        assert _bits(getattr(again, field)) == _bits(getattr(got, field)), field
    one = model(ref[1], est[1], mask_background=True)
    assert one.lpips.shape == (1,) and one.lpips.dtype == np.float64 and one.layers.shape == (5, 1)
    assert _bits(one.lpips[0]) == _bits(got.lpips[1]) and _bits(one.lpips_masked[0]) == _bits(got.lpips_masked[1])
    assert _bits(one.layers[:, 0]) == _bits(got.layers[:, 1])
    plain = model(ref, est)
    assert plain.lpips_masked is None and plain.layers_masked is None and _bits(plain.lpips) == _bits(got.lpips)
    same = model(ref, ref)
    assert _bits(same.lpips) == _bits(np.zeros(3)) and _bits(same.layers) == _bits(np.zeros((5, 3)))
    swapped = model(est, ref)
    assert _bits(swapped.lpips) == _bits(got.lpips) and _bits(swapped.layers) == _bits(got.layers)


def test_a_batch_larger_than_one_chunk(gpu_ctx):
    """30000 pairs of 31 x 31 need 2.3 GB of features: the forward call runs them in chunks over its workspace (1 GiB at most: 14119 pairs a chunk, the last one
    short).  Every copy of a pair scores with the bytes of the N = 3 call, wherever it sits."""
    import torch
    ref, est = _batch(31, 31)
    got = _forward(31, 31)
    reps = 10000
    ref_d, est_d = (torch.from_numpy(a.copy()).cuda().repeat(reps, 1, 1, 1) for a in (ref, est))
    big = _model()(ref_d, est_d, mask_background=True)
    for field in ("lpips", "lpips_masked"):
        assert _bits(getattr(big, field).reshape(reps, 3)) == _bits(np.tile(getattr(got, field), (reps, 1))), field
    assert _bits(big.layers.reshape(5, reps, 3)) == _bits(np.tile(got.layers[:, None], (1, reps, 1)))


# ---- real values, per layer ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(5))
def test_feature_rows_stay_inside_the_float32_summation_bound(gpu_ctx, index):
    """Seeded weights, 67 x 93, the three sets of three pictures, and the GPU's own float32 input to the row (row 0: the table's values), so errors do not compound:
    |got - want| <= gamma_K (sum |w| |x| + |b|) elementwise against the float64 restatement, gamma_K = K u / (1 - K u), u = 2^-24, K the row's products plus the
    bias.  The bound holds for a float32 sum in any order (and the ReLU does not widen a difference), so it is a condition, not a tolerance."""
    H, W = 67, 93
    model, got = _model(), _forward(H, W)
    x = LR.scaled_input(_sets(H, W)).reshape(9, H, W, 3) if index == 0 else got.features[index - 1].cpu().numpy().reshape(9, *got.features[index - 1].shape[2:])
    want, bound = LR.layer(index, x, model), LR.layer_bound(index, x, model)
    have = got.features[index].cpu().numpy().reshape(want.shape).astype(np.float64)
    assert bound.min() > 0 and (want > 0).mean() > 0.1
    ratio = np.abs(have - want) / bound
    print(f"row {index}: largest |got - want| / bound = {ratio.max():.3g} over {ratio.size} values")
    assert ratio.max() <= 1.0


# ---- the whole score against float64 ---------------------------------------------------------------------------------------------------------------------------
def _whole_reference():
    """Per size the restatement's float64 scores of pairs 0 and 1, plain and masked, and the yardstick: the largest relative distance of the float32 torch-CPU
    formulation (the reference's arithmetic) from them over all these pairs.  Computed once."""
    def make():
        model = _model()
        want, yardstick = {}, 0.0
        for H, W in SIZES:
            ref, est = _batch(H, W)
            for k in range(2):
                for v, frame in enumerate((ref[k], LR.mask_background(ref[k], est[k]))):
                    s64, s32 = LR.score(frame, est[k], model)[0], LR.score_f32(frame, est[k], model)[0]
                    want[(H, W, k, v)] = s64
                    yardstick = max(yardstick, abs(s32 - s64) / s64)
        return want, yardstick
    return _once("whole", make)


@pytest.mark.parametrize("H,W", SIZES)
def test_whole_score_against_float64(gpu_ctx, H, W):
    """The GPU score against the float64 restatement, seeded weights, smooth seeded pairs whose estimates have single channels at exactly 255, plain and masked.
    The yardstick is the float32 torch-CPU formulation's own largest relative distance from the float64 restatement over the test's twenty scores, computed
    here; the GPU must be within 64 x that (a k-ordered chain's error grows like K u where torch's blocked sums grow like sqrt(K) u: sqrt(3457) = 59).
    Measured on an MI355X box: yardstick 2.45e-7 (1.5e-7 on another CPU, whose convolutions sum in another order), so the bound is 1.57e-5; the GPU's largest
    distance per size was 1.07e-7, 2.55e-7, 1.34e-7, 7.26e-8 and 2.5e-8, in the order of SIZES."""
    want, yardstick = _whole_reference()
    got = _forward(H, W)
    assert 0 < yardstick < 1e-5
    worst = 0.0
    for k in range(2):
        for v, scores in enumerate((got.lpips, got.lpips_masked)):
            worst = max(worst, abs(scores[k] - want[(H, W, k, v)]) / want[(H, W, k, v)])
    print(f"{H} x {W}: largest relative distance of the GPU score from float64 {worst:.3g}; yardstick (float32 torch-CPU) {yardstick:.3g}, bound {64 * yardstick:.3g}")
    assert worst <= 64 * yardstick


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------------------
def test_image_similarity_and_compare_images_with_a_model(gpu_ctx):
    from hive_amd.evaluation import compare_images, image_similarity
    model = _model()
    ref, est = _batch(48, 64)
    got = _forward(48, 64)
    want, yardstick = _whole_reference()
    with_model = image_similarity(ref, est, mask_background=True, lpips=model)
    assert _bits(with_model.lpips) == _bits(got.lpips) and _bits(with_model.lpips_masked) == _bits(got.lpips_masked)
    plain = image_similarity(ref, est, lpips=model)
    assert _bits(plain.lpips) == _bits(got.lpips) and plain.lpips_masked is None
    without = image_similarity(ref, est, mask_background=True)
    assert without.lpips is None and without.lpips_masked is None
    for field in ("ssim", "psnr", "sse", "ssim_masked", "psnr_masked", "sse_masked"):
        assert _bits(getattr(without, field)) == _bits(getattr(with_model, field)), field
    ssim, psnr, lpips = compare_images(ref[0], est[0], lpips_fn=model)
    assert (ssim, psnr) == (without.ssim[0], without.psnr[0]) and _bits(np.float64(lpips)) == _bits(got.lpips[0])
    assert abs(lpips - want[(48, 64, 0, 0)]) / want[(48, 64, 0, 0)] <= 64 * yardstick
    four = compare_images(ref[0], est[0], lpips_fn=model, return_mifd=True)
    assert four[:3] == (ssim, psnr, lpips) and math.isnan(four[3])
    for other in (None, object(), lambda a, b: 0.5):
        assert math.isnan(compare_images(ref[0], est[0], lpips_fn=other)[2])


def test_compare_renders_with_a_model(gpu_ctx):
    """The rows' LPIPS are the model's scores of the frames against the rasteriser restatement's pictures, plain and masked; without a model they are nan and
    everything else is unchanged."""
    from hive_amd.evaluation import compare_renders
    model = _model()
    H, W = 48, 64
    pose = C.general_pose()
    K, quad = C.quad_scene(H, W, pose=pose)
    _, fan = C.fan_scene(H, W)
    fan = dict(fan, vertices=C.to_world(fan["vertices"], pose))
    frames = np.stack([SR.smooth_pair(H, W, seed=k)[0] for k in range(2)])
    pictures = np.stack([RR.render([fan], K, pose[:3, :3], pose[:3, 3], H, W)[0], RR.render([fan, quad], K, pose[:3, :3], pose[:3, 3], H, W)[0]])
    assert (pictures[0] == 255).all(-1).any() and not (pictures[0] == 255).all()
    renders, rows = compare_renders(K, [pose, pose], frames, [(fan,), (fan, quad)], size=(H, W), lpips=model)
    assert np.array_equal(renders.cpu().numpy(), pictures)
    direct = model(frames, pictures, mask_background=True)
    _, yardstick = _whole_reference()
    for k in range(2):
        assert _bits(np.float64(rows[k]["lpips"])) == _bits(direct.lpips[k]) and _bits(np.float64(rows[k]["lpips_masked"])) == _bits(direct.lpips_masked[k])
        for key, frame in (("lpips", frames[k]), ("lpips_masked", LR.mask_background(frames[k], pictures[k]))):
            want = LR.score(frame, pictures[k], model)[0]
            assert math.isfinite(rows[k][key]) and abs(rows[k][key] - want) / want <= 64 * yardstick, (k, key, rows[k][key], want)
    assert rows[0]["lpips"] != rows[0]["lpips_masked"]
    _, bare = compare_renders(K, [pose, pose], frames, [(fan,), (fan, quad)], size=(H, W))
    for k in range(2):
        assert math.isnan(bare[k]["lpips"]) and math.isnan(bare[k]["lpips_masked"])
        assert {key: v for key, v in bare[k].items() if "lpips" not in key} == {key: v for key, v in rows[k].items() if "lpips" not in key}


def test_small_pictures_warn_and_give_nan_and_bad_arguments_raise(gpu_ctx):
    from hive_amd.evaluation import compare_images, compare_renders, image_similarity
    model = _model()
    ref, est = SR.smooth_pair(30, 40, seed=3)
    with pytest.raises(ValueError, match="31"):
        model(ref, est)
    with pytest.warns(UserWarning, match="31"):
        ssim, psnr, lpips = compare_images(ref, est, lpips_fn=model)
    assert math.isnan(lpips) and (ssim, psnr) == compare_images(ref, est)[:2]
    with pytest.warns(UserWarning, match="31"):
        r = image_similarity(ref, est, mask_background=True, lpips=model)
    assert np.isnan(r.lpips).all() and np.isnan(r.lpips_masked).all() and np.isfinite(r.ssim).all()
    H, W = 24, 32
    s = C.grid_scene(H, W)
    with pytest.warns(UserWarning, match="31"):
        _, rows = compare_renders(s["K"], [C.IDENTITY], s["image"][None], (s["textured"],), size=(H, W), lpips=model)
    assert math.isnan(rows[0]["lpips"]) and math.isnan(rows[0]["lpips_masked"]) and math.isfinite(rows[0]["ssim"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        compare_images(ref, est)  # no model, no warning
    big = np.zeros((31, 31, 3), np.uint8)
    for bad_ref, bad_est in ((big.astype(np.float32), big), (big, big[:, :30]), (big[..., :2], big[..., :2]), (np.zeros((0, 31, 31, 3), np.uint8),) * 2):
        with pytest.raises(ValueError):
            model(bad_ref, bad_est)


def test_entry_points_refuse_bad_arguments_with_a_message(gpu_ctx):
    """Null pointers, a side below 31, N below 1, a variant count other than 1 or 2 and a layer outside 0 .. 4 return HIVE_ERR_INVALID and leave a message; nothing
    is launched."""
    import torch
    from hive_amd import _lib
    from hive_amd._lib import ptr
    model = _model()
    lib, net = gpu_ctx.lib, model.native(gpu_ctx)
    pic = torch.zeros((1, 31, 31, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    forward = lambda ref, est, n, h, w, variants, scores: lib.hive_lpips_forward(net, ptr(ref), ptr(est), n, h, w, variants, ptr(scores), None, None, None)
    for what, args in (("NULL", (None, pic, 1, 31, 31, 1, out)), ("NULL", (pic, None, 1, 31, 31, 1, out)), ("NULL", (pic, pic, 1, 31, 31, 1, None)),
                       ("31 x 31", (pic, pic, 1, 30, 31, 1, out)), ("31 x 31", (pic, pic, 1, 31, 30, 1, out)), ("N = 0", (pic, pic, 0, 31, 31, 1, out)),
                       ("variants = 3", (pic, pic, 1, 31, 31, 3, out))):
        rc = forward(*args)
        assert rc == _lib.ERR_INVALID
        with pytest.raises(_lib.HiveError, match=what):
            gpu_ctx.check(rc)
    x = torch.zeros((1, 8, 8, 64), dtype=torch.float32, device="cuda")
    y = torch.full((1, 8, 8, 384), 7.0, dtype=torch.float32, device="cuda")
    assert lib.hive_lpips_layer(net, 5, ptr(x), 1, 8, 8, ptr(y)) == _lib.ERR_INVALID
    assert lib.hive_lpips_layer(net, -1, ptr(x), 1, 8, 8, ptr(y)) == _lib.ERR_INVALID
    assert lib.hive_lpips_layer(net, 1, None, 1, 8, 8, ptr(y)) == _lib.ERR_INVALID
    assert lib.hive_lpips_layer(net, 1, ptr(x), 0, 8, 8, ptr(y)) == _lib.ERR_INVALID
    assert lib.hive_lpips_layer(net, 1, ptr(x), 1, 2, 8, ptr(y)) == _lib.ERR_INVALID, "nothing to pool"
    assert lib.hive_lpips_layer(net, 0, ptr(x), 1, 6, 8, ptr(y)) == _lib.ERR_INVALID, "an 11 x 11 window needs 7 rows"
    assert lib.hive_lpips_layer(None, 1, ptr(x), 1, 8, 8, ptr(y)) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (y == 7.0).all(), "a refused call writes nothing"
    with pytest.raises(ValueError):
        model.layer(1, x[..., :3])
