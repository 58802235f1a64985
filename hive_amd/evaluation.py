"""Score renders against held-out frames on the MI355X: the scoring half of the reference's experiment loops (/root/reference/scripts/experiments.py:775-858
for LLFF, :1554-1637 for HyperNeRF) -- ``compare_images`` (scripts/compare_image_pair.py:110-133: cv2 gray, skimage SSIM and PSNR) and
``pytorch_msssim.ms_ssim`` (:1627-1635), plain and with the frame whitened where the render shows background (:846-848) -- by the kernels of
csrc/similarity.hip.  Pictures stay on the device; the only copy back is the scores.

The rules are stated in include/hive_mi355x.h above ``hive_similarity_ssim_psnr`` and restated in tests/similarity_restatement.py.  cv2, skimage and
pytorch_msssim cannot be run beside this code: the gray conversion is not pinned against cv2, SSIM and PSNR are not pinned against skimage, MS-SSIM is not
pinned against pytorch_msssim.  LPIPS (AlexNet weights) and MIFD (SIFT) are absent: their slots hold nan."""
import json
import warnings
from dataclasses import dataclass

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr

NAN = float("nan")
_MS_LEVELS = 5


def _is_torch(x):
    return type(x).__module__.startswith("torch")


@dataclass
class SimilarityResult:
    """Scores of N pairs: float64 arrays of length N (``ms_ssim`` nan when not asked for).  The ``*_masked`` fields are None without ``mask_background``;
    ``sse`` / ``sse_masked`` are the integer sums of squared gray differences behind the PSNR.  With ``return_maps``: ``ssim_map`` (N, H - 6, W - 6) float64,
    ``gray_ref`` and ``gray_est`` (N, H, W) uint8 and, masked, ``ssim_map_masked`` and ``gray_ref_masked``, as device tensors."""
    ssim: np.ndarray
    psnr: np.ndarray
    ms_ssim: np.ndarray
    sse: np.ndarray
    ssim_masked: np.ndarray = None
    psnr_masked: np.ndarray = None
    ms_ssim_masked: np.ndarray = None
    sse_masked: np.ndarray = None
    ssim_map: object = None
    ssim_map_masked: object = None
    gray_ref: object = None
    gray_ref_masked: object = None
    gray_est: object = None


def _checked_shapes(ref, est, ms_ssim, channel_order):
    """(N, H, W, batched) after every check that needs no device."""
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order: 'bgr' (the reference's numbers) or 'rgb', got {channel_order!r}")
    for name, a in (("ref", ref), ("est", est)):
        dtype = str(a.dtype).replace("torch.", "")
        if dtype != "uint8":
            raise ValueError(f"{name}: uint8 pictures, got {dtype}")
    rs, es = tuple(ref.shape), tuple(est.shape)
    if rs != es:
        raise ValueError(f"shapes differ: {rs} and {es}")
    if len(rs) not in (3, 4) or rs[-1] != 3:
        raise ValueError(f"pictures are (H, W, 3) or (N, H, W, 3), got {rs}")
    batched = len(rs) == 4
    n, h, w = (rs[0] if batched else 1), rs[-3], rs[-2]
    if n < 1:
        raise ValueError("no picture to compare")
    if h < 7 or w < 7:
        raise ValueError(f"{h} x {w} is smaller than the 7 x 7 window of SSIM")
    if ms_ssim and min(h, w) <= 160:
        raise ValueError(f"MS-SSIM needs a smaller side above 160 (five levels of an 11-tap window), got {h} x {w}")
    return n, h, w, batched


def _psnr(sse, h, w):
    """10 log10(255^2 / mse) in float64 from the integer sums; inf where the planes are equal."""
    out = np.full(sse.shape, np.inf)
    some = sse != 0
    out[some] = 10 * np.log10(65025.0 / (sse[some] / (h * w)))
    return out


def ms_ssim_window():
    """The 11-tap Gaussian of pytorch_msssim (sigma 1.5), float64, normalised by its sum."""
    g = np.exp(-(np.arange(11, dtype=np.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return np.ascontiguousarray(g / g.sum())


def image_similarity(ref, est, *, ms_ssim=False, mask_background=False, channel_order="bgr", return_maps=False, ctx=None):
    """SSIM and PSNR of the gray pictures, as ``compare_images`` of scripts/compare_image_pair.py:110-133 computes them, and on request MS-SSIM of the colour
    pictures as experiments.py:1627-1635 does, for one pair or a batch, on the GPU.

    ``ref`` (the held-out frames) and ``est`` (the renders): uint8 (H, W, 3) or (N, H, W, 3), numpy arrays (uploaded once) or device tensors (used in place);
    never modified.  ``channel_order="bgr"`` gives channel 0 the blue weight of cv2's COLOR_BGR2GRAY, which is what the reference's numbers contain (it hands RGB
    pictures to a BGR conversion); ``"rgb"`` swaps the outer weights.  ``mask_background``: also score against the frame whitened where the render shows
    background, ``masked_frame[color_np == [255, 255, 255]] = 255`` (:846-848) -- per channel, as that comparison broadcasts; the whitened frame is never
    written.  Returns a ``SimilarityResult``.  ValueError: shapes that differ, a dtype other than uint8, H or W below 7, a smaller side of 160 or less with
    ``ms_ssim``, an unknown ``channel_order``.  One call holds at most 65535 / 2 pairs (65535 / 6 with ``ms_ssim``): the variant, the picture and the channel are
    one grid dimension.  The only device-to-host copy is the scores."""
    n, h, w, batched = _checked_shapes(ref, est, ms_ssim, channel_order)
    import torch
    dev = next((a.device for a in (ref, est) if _is_torch(a) and a.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    ctx = ctx or _lib.default_context(dev.index or 0)
    ctx.follow_torch_stream()
    lib, handle = ctx.lib, ctx.handle

    def as_dev(a):
        if not _is_torch(a):
            a = np.ascontiguousarray(a)
            with warnings.catch_warnings():  # a read-only array is fine: it is only copied to the device
                warnings.simplefilter("ignore", UserWarning)
                a = torch.from_numpy(a)
        return a.to(dev).reshape(n, h, w, 3).contiguous()

    ref_d, est_d = as_dev(ref), as_dev(est)
    variants = 2 if mask_background else 1
    vn = variants * n
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    # one block of results: [0, vn) the squared-difference sums (int64 bits), [vn, 2 vn) SSIM, [2 vn, 3 vn) MS-SSIM
    results = f64(3 * vn)
    results[2 * vn:] = NAN
    sse = results[:vn].view(torch.int64)
    tiles = -(-(h - 6) // 32) * -(-(w - 6) // 32)
    partials = f64(vn, tiles)
    maps = f64(variants, n, h - 6, w - 6) if return_maps else None
    gray_ref = torch.empty((variants, n, h, w), dtype=torch.uint8, device=dev) if return_maps else None
    gray_est = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if return_maps else None
    ctx.check(lib.hive_similarity_ssim_psnr(handle, ptr(ref_d), ptr(est_d), n, h, w, int(channel_order == "rgb"), variants, ptr(partials), ptr(sse), ptr(maps),
                                            ptr(gray_ref), ptr(gray_est)))
    ctx.check(lib.hive_similarity_finish(handle, ptr(partials), vn, tiles, float((h - 6) * (w - 6)), ptr(results[vn:])))
    if ms_ssim:
        window = ms_ssim_window()
        means = f64(_MS_LEVELS, 2, vn, 3)
        x = y = None
        lh, lw = h, w
        for level in range(_MS_LEVELS):
            lt = -(-(lh - 10) // 16) * -(-(lw - 10) // 32)
            level_partials = f64(2, vn * 3, lt)
            last = level == _MS_LEVELS - 1
            nh, nw = (lh + 1) // 2, (lw + 1) // 2
            x_next, y_next = (None, None) if last else (f64(variants, n, 3, nh, nw), f64(n, 3, nh, nw))
            ctx.check(lib.hive_similarity_msssim_level(handle, ptr(ref_d) if level == 0 else None, ptr(est_d) if level == 0 else None, ptr(x), ptr(y), n, lh, lw,
                                                       variants, ptr(window), ptr(level_partials), ptr(x_next), ptr(y_next)))
            ctx.check(lib.hive_similarity_finish(handle, ptr(level_partials), 2 * vn * 3, lt, float((lh - 10) * (lw - 10)), ptr(means[level])))
            x, y, lh, lw = x_next, y_next, nh, nw
        ctx.check(lib.hive_similarity_msssim_combine(handle, ptr(means), vn, ptr(results[2 * vn:])))
    host = results.cpu().numpy()  # the only copy back
    sse_h = host[:vn].view(np.int64).reshape(variants, n)
    ssim_h, ms_h = host[vn:2 * vn].reshape(variants, n), host[2 * vn:].reshape(variants, n)
    psnr_h = _psnr(sse_h, h, w)
    out = SimilarityResult(ssim=ssim_h[0].copy(), psnr=psnr_h[0], ms_ssim=ms_h[0].copy(), sse=sse_h[0].copy())
    if mask_background:
        out.ssim_masked, out.psnr_masked, out.ms_ssim_masked, out.sse_masked = ssim_h[1].copy(), psnr_h[1], ms_h[1].copy(), sse_h[1].copy()
    if return_maps:
        out.ssim_map, out.gray_ref, out.gray_est = maps[0], gray_ref[0], gray_est
        if mask_background:
            out.ssim_map_masked, out.gray_ref_masked = maps[1], gray_ref[1]
    return out


def compare_images(ref_image, est_image, lpips_fn=None, return_mifd=False):
    """``compare_images`` of scripts/compare_image_pair.py:110-133 for one pair of uint8 (H, W, 3) pictures: ``(ssim, psnr, lpips)``, with ``mifd`` behind it when
    ``return_mifd`` is set.  SSIM and PSNR come from ``image_similarity`` with the default channel order.  LPIPS needs AlexNet weights and MIFD needs SIFT;
    neither exists here, so both are nan and a non-None ``lpips_fn`` is ignored."""
    r = image_similarity(ref_image, est_image)
    scores = (float(r.ssim[0]), float(r.psnr[0]), NAN)
    return (*scores, NAN) if return_mifd else scores


def compare_renders(camera_matrix, poses, frames, meshes, *, ms_ssim=False, size=None, names=None):
    """The render-and-score loop of experiments.py:833-852 (and :1594-1614 with ``ms_ssim``): view i is ``render.render_mesh(camera_matrix, poses[i],
    *meshes_i)``, all views share one ``RenderBuffers``, the renders are stacked on the device and scored against ``frames`` (uint8 (N, H, W, 3), numpy or
    device) by one ``image_similarity(..., mask_background=True)`` call.

    ``meshes``: one tuple of meshes used for every view, or a sequence with one tuple per view (the HyperNeRF loop: a per-frame foreground and a shared
    background).  ``names``: per view a dict whose items lead the row (``dataset``, ``camera_feed``, ``config`` of the reference's ``RenderResult``,
    :663-675) or a string taken as ``config``; by default ``camera_feed`` is the view's index.

    Returns ``(renders, rows)``: the uint8 (N, H, W, 3) device tensor and one dict per view with ``ssim``, ``psnr``, ``lpips``, ``ssim_masked``,
    ``psnr_masked``, ``lpips_masked`` (LPIPS nan) behind the names.  With ``ms_ssim`` rows also carry ``ms_ssim`` and ``ms_ssim_masked``, and the rule of
    :1609-1610 applies: a masked result with infinite PSNR or an MS-SSIM of exactly 1.0 becomes all nan."""
    import torch
    from hive_amd import render
    n = len(poses)
    if len(frames) != n:
        raise ValueError(f"{n} poses but {len(frames)} frames")
    if n == 0:
        raise ValueError("no view to compare")
    per_view = not isinstance(meshes, tuple)
    if per_view and len(meshes) != n:
        raise ValueError(f"meshes: one tuple for every view, or a sequence of {n} tuples, got {len(meshes)} entries")
    if names is not None and len(names) != n:
        raise ValueError(f"{n} poses but {len(names)} names")
    h, w = (int(v) for v in (size if size is not None else tuple(frames.shape[1:3])))
    buffers = render.RenderBuffers(h, w)
    renders = torch.stack([render.render_mesh(camera_matrix, poses[i], *(meshes[i] if per_view else meshes), size=(h, w), buffers=buffers) for i in range(n)])
    r = image_similarity(frames, renders, ms_ssim=ms_ssim, mask_background=True)
    rows = []
    for i in range(n):
        name = names[i] if names is not None else {}
        row = dict(name) if isinstance(name, dict) else {"config": str(name)}
        for key, default in (("dataset", ""), ("camera_feed", i), ("config", "")):
            row.setdefault(key, default)
        row.update(ssim=float(r.ssim[i]), psnr=float(r.psnr[i]), lpips=NAN, ssim_masked=float(r.ssim_masked[i]), psnr_masked=float(r.psnr_masked[i]),
                   lpips_masked=NAN)
        if ms_ssim:
            row.update(ms_ssim=float(r.ms_ssim[i]), ms_ssim_masked=float(r.ms_ssim_masked[i]))
            if np.isinf(row["psnr_masked"]) or row["ms_ssim_masked"] == 1.0:
                row.update(ssim_masked=NAN, psnr_masked=NAN, lpips_masked=NAN, ms_ssim_masked=NAN)
        rows.append(row)
    return renders, rows


def save_results(rows, path):
    """The JSON list experiments.py:856-857 writes: one object per row (nan and inf in Python's spelling, as ``json.dump`` writes them there)."""
    with open(path, "w") as f:
        json.dump([dict(row) for row in rows], f)
