"""The picture scores on the GPU (csrc/similarity.hip behind hive_amd.evaluation) against the restatement of their rules (tests/similarity_restatement.py): gray
planes, the S map, the squared-difference sum and the PSNR exactly; the SSIM score within the summation bound and with the same bits in every batch and run;
MS-SSIM within 1e-9; compare_renders against the rasteriser's restatement."""
import math

import numpy as np
import pytest

import render_cases as C
import render_restatement as RR
import similarity_restatement as SR

pytestmark = pytest.mark.gpu

# The SSIM kernel's tile is 32 x 32 values of the (H - 6, W - 6) map and reads 38 x 38 pixels.  (39, 71): the map is 33 x 65, a tile edge one value before its
# end in each direction; (37, 69): 31 x 63, one value after it.  (33, 65) and (31, 63) put the picture's own end there.  Every W but 8, 64 and 160 is no multiple of 4.
SIZES = [(7, 7), (8, 9), (23, 37), (48, 64), (120, 160), (39, 71), (37, 69), (33, 65), (31, 63)]

_pairs = {}


def _batch(H, W, n=3):
    """n seeded pairs of one size, different pictures, each estimate with single channels at exactly 255; computed once."""
    if (H, W, n) not in _pairs:
        pairs = [SR.smooth_pair(H, W, seed=100 * H + W + k, whites=max(3, H * W // 40)) for k in range(n)]
        ref, est = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ref.setflags(write=False), est.setflags(write=False)
        _pairs[(H, W, n)] = (ref, est)
    return _pairs[(H, W, n)]


def _check_exact(got, ref, est, order, masked):
    """Every exact output of one call against the restatement, picture by picture."""
    for k in range(len(ref)):
        for variant in ("plain", "masked") if masked else ("plain",):
            frame = SR.mask_background(ref[k], est[k]) if variant == "masked" else ref[k]
            want = SR.compare(frame, est[k], order)
            m = variant == "masked"
            gray_ref, S = (got.gray_ref_masked, got.ssim_map_masked) if m else (got.gray_ref, got.ssim_map)
            sse, psnr, ssim = (got.sse_masked, got.psnr_masked, got.ssim_masked) if m else (got.sse, got.psnr, got.ssim)
            where = f"picture {k}, {variant}, {order}"
            assert np.array_equal(gray_ref[k].cpu().numpy(), want["gray_ref"]), where
            assert np.array_equal(got.gray_est[k].cpu().numpy(), want["gray_est"]), where
            S = S[k].cpu().numpy()
            assert S.shape == want["map"].shape and np.array_equal(S, want["map"]), f"{where}: S differs at {int((S != want['map']).sum())} places"
            assert int(sse[k]) == want["sse"], where
            assert psnr[k] == want["psnr"], where  # (both sides: the same host expression on the same integer)
            mean = math.fsum(want["map"].ravel()) / want["map"].size
            print(f"{where}: ssim {ssim[k]!r}, |ssim - fsum mean| = {abs(ssim[k] - mean):.3g}")
            assert abs(ssim[k] - mean) <= 1e-10, where
            assert ssim[k] == want["ssim"], f"{where}: the sum's stated order gives {want['ssim']!r}"


@pytest.mark.parametrize("H,W", SIZES)
def test_exact_outputs_at_every_size(gpu_ctx, H, W):
    """N = 3 and N = 1, plain and masked, both channel orders; the score of a picture has the same bits in either batch."""
    from hive_amd.evaluation import image_similarity
    ref, est = _batch(H, W)
    for order in ("bgr", "rgb"):
        got = image_similarity(ref, est, mask_background=True, channel_order=order, return_maps=True)
        assert got.ssim.shape == got.psnr.shape == got.ssim_masked.shape == (3,) and got.ssim.dtype == np.float64 and np.isnan(got.ms_ssim).all()
        _check_exact(got, ref, est, order, masked=True)
        one = image_similarity(ref[1], est[1], mask_background=True, channel_order=order, return_maps=True)
        _check_exact(one, ref[1:2], est[1:2], order, masked=True)
        assert one.ssim[0].tobytes() == got.ssim[1].tobytes() and one.ssim_masked[0].tobytes() == got.ssim_masked[1].tobytes()
    plain = image_similarity(ref, est, return_maps=True)
    assert plain.ssim_masked is None and plain.psnr_masked is None and plain.ssim_map_masked is None
    _check_exact(plain, ref, est, "bgr", masked=False)


def test_the_mask_changes_the_scores_where_single_channels_are_white(gpu_ctx):
    """A pair whose estimate has exact 255s in single channels: the masked variant differs from the plain one and from a per-pixel rule."""
    from hive_amd.evaluation import image_similarity
    ref, est = _batch(23, 37)
    single = (est == 255).any(-1) & ~(est == 255).all(-1)
    assert single.any()
    got = image_similarity(ref, est, mask_background=True, return_maps=True)
    assert (got.sse != got.sse_masked).all()
    per_pixel = ref.copy()
    per_pixel[(est == 255).all(-1)] = 255
    assert any(SR.compare(per_pixel[k], est[k])["sse"] != int(got.sse_masked[k]) for k in range(3))


def test_scores_repeat_and_inputs_stay(gpu_ctx):
    """Two calls give the same bits; numpy inputs and device tensors give the same results; nothing is written to either."""
    import torch
    from hive_amd.evaluation import image_similarity
    ref, est = _batch(120, 160)
    ref_d, est_d = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(est.copy()).cuda()
    a = image_similarity(ref, est, mask_background=True)
    b = image_similarity(ref, est, mask_background=True)
    c = image_similarity(ref_d, est_d, mask_background=True)
    for other in (b, c):
        for field in ("ssim", "psnr", "sse", "ssim_masked", "psnr_masked", "sse_masked"):
            assert getattr(a, field).tobytes() == getattr(other, field).tobytes(), field
    assert np.array_equal(ref_d.cpu().numpy(), ref) and np.array_equal(est_d.cpu().numpy(), est)
    assert np.array_equal(ref, _batch(120, 160)[0]) and not ref.flags.writeable
    # a non-contiguous device view is read, not written
    wide = torch.zeros((3, 120, 200, 3), dtype=torch.uint8, device="cuda")
    wide[:, :, :160] = ref_d
    d = image_similarity(wide[:, :, :160], est_d)
    assert d.ssim.tobytes() == a.ssim.tobytes() and int(wide[:, :, 160:].max()) == 0


def test_identical_pictures_and_compare_images(gpu_ctx):
    from hive_amd.evaluation import compare_images, image_similarity
    ref, est = _batch(48, 64)
    same = image_similarity(ref, ref)
    assert (same.ssim == 1.0).all() and np.isinf(same.psnr).all() and (same.sse == 0).all()
    want = SR.compare(ref[0], est[0])
    ssim, psnr, lpips = compare_images(ref[0], est[0], lpips_fn=object())
    assert ssim == want["ssim"] and psnr == want["psnr"] and math.isnan(lpips)
    four = compare_images(ref[0], est[0], return_mifd=True)
    assert len(four) == 4 and four[:2] == (ssim, psnr) and math.isnan(four[2]) and math.isnan(four[3])


_ms_want = {}


def _ms_reference(H, W):
    """The restatement's MS-SSIM of the two pairs of one size, plain and masked, with the level values; computed once."""
    if (H, W) not in _ms_want:
        ref, est = _batch(H, W, n=2)
        rows = []
        for k in range(2):
            rows.append([SR.ms_ssim(frame, est[k], return_levels=True) for frame in (ref[k], SR.mask_background(ref[k], est[k]))])
        _ms_want[(H, W)] = rows
    return _ms_want[(H, W)]


@pytest.mark.parametrize("H,W", [(161, 161), (176, 208), (163, 189)])
def test_ms_ssim_against_the_restatement(gpu_ctx, H, W):
    """Within 1e-9 absolute, N = 2, plain and masked.  Filtered values in [0, 1] carry about 2e-15 of error under denominators of at least C2 = 9e-4: about 1e-11
    per level, and the powers are below 1.  All level values are >= 0.5 in the restatement (asserted first), so no rounding crosses the relu."""
    from hive_amd.evaluation import image_similarity
    ref, est = _batch(H, W, n=2)
    want = _ms_reference(H, W)
    for k in range(2):
        for score, levels in want[k]:
            assert levels.min() >= 0.5, levels
    got = image_similarity(ref, est, ms_ssim=True, mask_background=True)
    for k in range(2):
        for name, value, (score, _) in (("plain", got.ms_ssim[k], want[k][0]), ("masked", got.ms_ssim_masked[k], want[k][1])):
            print(f"{H} x {W}, picture {k}, {name}: {value!r} against {score!r}, difference {abs(value - score):.3g}")
            assert abs(value - score) <= 1e-9
    assert want[0][0][0] != want[0][1][0], "the mask must matter to this pair"
    # the other scores of the same call are those of a call without MS-SSIM, and a picture's MS-SSIM does not depend on its batch
    plain = image_similarity(ref, est, mask_background=True)
    assert plain.ssim.tobytes() == got.ssim.tobytes() and plain.psnr_masked.tobytes() == got.psnr_masked.tobytes()
    one = image_similarity(ref[1], est[1], ms_ssim=True)
    assert one.ms_ssim[0].tobytes() == got.ms_ssim[1].tobytes()


def test_ms_ssim_of_identical_pictures_and_its_size_limit(gpu_ctx):
    from hive_amd.evaluation import image_similarity
    ref, _ = _batch(161, 161, n=2)
    assert np.abs(image_similarity(ref, ref, ms_ssim=True).ms_ssim - 1.0).max() <= 1e-12
    small = np.zeros((160, 200, 3), np.uint8)
    with pytest.raises(ValueError):
        image_similarity(small, small, ms_ssim=True)


def test_compare_renders_of_a_scene_from_its_own_pose(gpu_ctx):
    """grid_scene from its own pose returns its image on the covered block [0:H-1, 0:W-1] and white elsewhere: against that frame every score is perfect."""
    from hive_amd.evaluation import compare_renders
    H, W = 24, 32
    s = C.grid_scene(H, W)
    frame = np.full((H, W, 3), 255, np.uint8)
    frame[:H - 1, :W - 1] = s["image"][:H - 1, :W - 1]
    renders, rows = compare_renders(s["K"], [C.IDENTITY], frame[None], (s["textured"],), size=(H, W))
    assert np.array_equal(renders.cpu().numpy()[0], frame)
    (row,) = rows
    assert row["ssim"] == 1.0 and row["psnr"] == math.inf and row["ssim_masked"] == 1.0 and row["psnr_masked"] == math.inf
    assert math.isnan(row["lpips"]) and math.isnan(row["lpips_masked"]) and "ms_ssim" not in row
    assert list(row)[:3] == ["dataset", "camera_feed", "config"] and row["camera_feed"] == 0


def test_compare_renders_at_a_general_pose(gpu_ctx):
    """Rows equal the similarity restatement applied to the rasteriser restatement's picture; the per-view and the shared form of `meshes` agree."""
    from hive_amd.evaluation import compare_renders
    H, W = 24, 32
    pose = C.general_pose()
    K, quad = C.quad_scene(H, W, pose=pose)
    _, fan = C.fan_scene(H, W)
    fan = dict(fan, vertices=C.to_world(fan["vertices"], pose))
    poses = [pose, pose]
    frames = np.stack([SR.smooth_pair(H, W, seed=k)[0] for k in range(2)])
    frames[0, 5:9, 5:9] = 255  # some frame pixels that are white already
    pictures = [RR.render([fan], K, pose[:3, :3], pose[:3, 3], H, W)[0], RR.render([fan, quad], K, pose[:3, :3], pose[:3, 3], H, W)[0]]
    assert (pictures[0] == 255).all(-1).any() and not (pictures[0] == 255).all(), "the fan leaves background and covers something"
    renders, rows = compare_renders(K, poses, frames, [(fan,), (fan, quad)], size=(H, W), names=[{"dataset": "a", "config": "fan"}, "both"])
    assert rows[0]["dataset"] == "a" and rows[0]["config"] == "fan" and rows[0]["camera_feed"] == 0 and rows[1]["config"] == "both" and rows[1]["camera_feed"] == 1
    for k in range(2):
        assert np.array_equal(renders[k].cpu().numpy(), pictures[k])
        plain, masked = SR.compare(frames[k], pictures[k]), SR.compare(SR.mask_background(frames[k], pictures[k]), pictures[k])
        assert rows[k]["psnr"] == plain["psnr"] and rows[k]["psnr_masked"] == masked["psnr"]
        assert rows[k]["ssim"] == plain["ssim"] and rows[k]["ssim_masked"] == masked["ssim"]
    assert rows[0]["psnr"] != rows[0]["psnr_masked"]
    # the same meshes for every view: one tuple, or that tuple per view
    _, shared = compare_renders(K, poses, frames, (fan, quad), size=(H, W))
    _, each = compare_renders(K, poses, frames, [(fan, quad), (fan, quad)], size=(H, W))
    assert shared == each and shared[1] == {**rows[1], "dataset": "", "config": ""}


def test_compare_renders_turns_a_masked_perfect_match_into_nan(gpu_ctx):
    """The rule of experiments.py:1609-1610, on pictures large enough for MS-SSIM: the frame is the render, so the masked PSNR is infinite."""
    from hive_amd.evaluation import compare_renders
    from hive_amd.render import render_mesh
    H = W = 161
    s = C.grid_scene(H, W, seed=2)
    frame = render_mesh(s["K"], C.IDENTITY, s["textured"], size=(H, W))
    noisy = SR.smooth_pair(H, W, seed=9)[0]
    import torch
    frames = torch.stack([frame, torch.from_numpy(noisy).cuda()])
    _, rows = compare_renders(s["K"], [C.IDENTITY, C.IDENTITY], frames, (s["textured"],), ms_ssim=True, size=(H, W))
    perfect, other = rows
    assert perfect["psnr"] == math.inf and perfect["ssim"] == 1.0 and abs(perfect["ms_ssim"] - 1.0) <= 1e-12
    assert all(math.isnan(perfect[key]) for key in ("ssim_masked", "psnr_masked", "lpips_masked", "ms_ssim_masked"))
    assert all(math.isfinite(other[key]) for key in ("ssim", "psnr", "ms_ssim", "ssim_masked", "psnr_masked", "ms_ssim_masked"))


def test_entry_points_refuse_bad_arguments_with_a_message(gpu_ctx):
    """Null pointers, H or W below 7 and N below 1 return HIVE_ERR_INVALID and leave a message; nothing is launched."""
    import torch
    from hive_amd import _lib
    from hive_amd._lib import ptr
    lib, handle = gpu_ctx.lib, gpu_ctx.handle
    pic = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    sse = out[8:].view(torch.int64)
    ssim = lambda ref, est, n, h, w, partials, sums: lib.hive_similarity_ssim_psnr(handle, ptr(ref), ptr(est), n, h, w, 0, 1, ptr(partials), ptr(sums), None, None, None)
    for what, args in (("NULL", (None, pic, 1, 8, 8, out, sse)), ("NULL", (pic, pic, 1, 8, 8, None, sse)), ("NULL", (pic, pic, 1, 8, 8, out, None)),
                       ("7 x 7", (pic, pic, 1, 6, 8, out, sse)), ("7 x 7", (pic, pic, 1, 8, 6, out, sse)), ("N = 0", (pic, pic, 0, 8, 8, out, sse))):
        rc = ssim(*args)  # (the message is that of the context's last failure: read it before the next call)
        assert rc == _lib.ERR_INVALID
        with pytest.raises(_lib.HiveError, match=what):
            gpu_ctx.check(rc)
    window = np.ones(11) / 11
    level = lambda a, b, x, y, n, h, w, win, partials: lib.hive_similarity_msssim_level(handle, ptr(a), ptr(b), ptr(x), ptr(y), n, h, w, 1, ptr(win), ptr(partials), None, None)
    assert level(None, None, None, None, 1, 11, 11, window, out) == _lib.ERR_INVALID
    assert level(pic, pic, out, out, 1, 11, 11, window, out) == _lib.ERR_INVALID, "one kind of input"
    assert level(pic, pic, None, None, 1, 10, 11, window, out) == _lib.ERR_INVALID
    assert level(pic, pic, None, None, 0, 11, 11, window, out) == _lib.ERR_INVALID
    assert level(pic, pic, None, None, 1, 11, 11, None, out) == _lib.ERR_INVALID
    assert level(pic, pic, None, None, 1, 11, 11, window, None) == _lib.ERR_INVALID
    assert lib.hive_similarity_finish(handle, None, 1, 1, 1.0, ptr(out)) == _lib.ERR_INVALID
    assert lib.hive_similarity_finish(handle, ptr(out), 0, 1, 1.0, ptr(out)) == _lib.ERR_INVALID
    assert lib.hive_similarity_msssim_combine(handle, ptr(out), 0, ptr(out)) == _lib.ERR_INVALID
    assert lib.hive_similarity_msssim_combine(handle, None, 1, ptr(out)) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call writes nothing"
