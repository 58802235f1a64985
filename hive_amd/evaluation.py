"""Score renders against held-out frames on the MI355X: the scoring half of the reference's experiment loops (/root/reference/scripts/experiments.py:775-858
for LLFF, :1554-1637 for HyperNeRF) -- ``compare_images`` (scripts/compare_image_pair.py:110-133: cv2 gray, skimage SSIM and PSNR, LPIPS),
``pytorch_msssim.ms_ssim`` (:1627-1635), plain and with the frame whitened where the render shows background (:846-848) -- by the kernels of
csrc/similarity.hip and csrc/lpips.hip, and ``mifd`` (compare_image_pair.py:44-97) by the SIFT detector and the exact matcher of csrc/sift.hip
(``hive_amd.features``).  Pictures stay on the device; the only copy back is the scores (and, for MIFD, the keypoint counts).

The rules are stated in include/hive_mi355x.h above ``hive_similarity_ssim_psnr`` and ``hive_lpips_create`` and restated in tests/similarity_restatement.py and
tests/lpips_restatement.py.  cv2, skimage, pytorch_msssim, lpips and torchvision cannot be run beside this code: the gray conversion is not pinned against cv2,
SSIM and PSNR are not pinned against skimage, MS-SSIM is not pinned against pytorch_msssim, LPIPS is not pinned against lpips / torchvision.  LPIPS needs the
AlexNet and linear-layer weights (``LPIPS.from_files``); without a model its slots hold nan.  MIFD needs a ``features.SIFT`` object (``mifd=`` / ``sift=``);
without one its slot holds nan.  Its SIFT is restated from recall of OpenCV 4.x and not pinned against cv2; its matcher is the exact nearest-neighbour search
and not pinned against the reference's approximate FLANN matcher (include/hive_mi355x.h above ``hive_sift_create``, tests/sift_restatement.py)."""
import json
import warnings
from dataclasses import dataclass

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr
from hive_amd._pictures import device_of, is_torch, on_device

NAN = float("nan")
_MS_LEVELS = 5
LPIPS_MIN_SIDE = 31  # conv1 gives 7, the two pools 3 and 1: the smallest picture with an output in every layer
# lpips.LPIPS(net='alex'): (C_in, C_out, kernel, stride, padding, a maxpool 3 / 2 in front) of the five convolutions whose ReLU maps are compared, and their
# indices in torchvision's alexnet().features
_LPIPS_LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
_ALEX_INDEX = (0, 3, 6, 8, 10)


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
    lpips: np.ndarray = None  # with ``image_similarity(..., lpips=model)``
    lpips_masked: np.ndarray = None
    mifd: np.ndarray = None  # with ``image_similarity(..., mifd=sift)``: float64 (N,), nan where a pair has no score
    mifd_matches: np.ndarray = None  # int32 (N,): the ratio-test survivors behind ``mifd``
    mifd_masked: np.ndarray = None


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


def image_similarity(ref, est, *, ms_ssim=False, mask_background=False, channel_order="bgr", return_maps=False, ctx=None, lpips=None, mifd=None):
    """SSIM and PSNR of the gray pictures, as ``compare_images`` of scripts/compare_image_pair.py:110-133 computes them, and on request MS-SSIM of the colour
    pictures as experiments.py:1627-1635 does, for one pair or a batch, on the GPU.

    ``ref`` (the held-out frames) and ``est`` (the renders): uint8 (H, W, 3) or (N, H, W, 3), numpy arrays (uploaded once) or device tensors (used in place);
    never modified.  ``channel_order="bgr"`` gives channel 0 the blue weight of cv2's COLOR_BGR2GRAY, which is what the reference's numbers contain (it hands RGB
    pictures to a BGR conversion); ``"rgb"`` swaps the outer weights.  ``mask_background``: also score against the frame whitened where the render shows
    background, ``masked_frame[color_np == [255, 255, 255]] = 255`` (:846-848) -- per channel, as that comparison broadcasts; the whitened frame is never
    written.  Returns a ``SimilarityResult``.  ValueError: shapes that differ, a dtype other than uint8, H or W below 7, a smaller side of 160 or less with
    ``ms_ssim``, an unknown ``channel_order``.  One call holds at most 65535 / 2 pairs (65535 / 6 with ``ms_ssim``): the variant, the picture and the channel are
    one grid dimension.  The only device-to-host copy is the scores.

    ``lpips``: an ``LPIPS`` model; the result then carries ``lpips`` and, with ``mask_background``, ``lpips_masked`` from the same device tensors (a second
    copy back of scores).  A picture with a side below 31 has no LPIPS: the fields are nan and a warning says so.

    ``mifd``: a ``features.SIFT`` object; the result then carries ``mifd`` (``mifd(ref_gray, est_gray)`` of compare_image_pair.py:44-97 with its defaults),
    ``mifd_matches`` and, with ``mask_background``, ``mifd_masked``, from the gray planes the SSIM kernel wrote, which never leave the device (the keypoint counts
    and the scores are copied back).  A pair without a score is nan, with the reference's warning; so is a picture with a side below 6, which SIFT cannot handle."""
    n, h, w, batched = _checked_shapes(ref, est, ms_ssim, channel_order)
    import torch
    dev = device_of(ref, est)
    ctx = _lib.context_for(ctx, dev)
    lib, handle = ctx.lib, ctx.handle

    # numpy arrays are uploaded, device tensors used in place when contiguous
    ref_d, est_d = on_device(ref, dev, shape=(n, h, w, 3)), on_device(est, dev, shape=(n, h, w, 3))
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
    want_gray = return_maps or mifd is not None
    gray_ref = torch.empty((variants, n, h, w), dtype=torch.uint8, device=dev) if want_gray else None
    gray_est = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if want_gray else None
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
    if lpips is not None:
        if min(h, w) < LPIPS_MIN_SIDE:
            warnings.warn(f"{h} x {w} is smaller than {LPIPS_MIN_SIDE} x {LPIPS_MIN_SIDE}: no LPIPS, its scores are nan")
            out.lpips = np.full(n, NAN)
            out.lpips_masked = np.full(n, NAN) if mask_background else None
        else:
            scored = lpips(ref_d, est_d, mask_background=mask_background, ctx=ctx)
            out.lpips, out.lpips_masked = scored.lpips, scored.lpips_masked
    if mifd is not None:
        from hive_amd import features
        if min(h, w) < features.SIFT_MIN_SIDE:
            warnings.warn(f"{h} x {w} is smaller than {features.SIFT_MIN_SIDE} x {features.SIFT_MIN_SIDE}: no SIFT, the MIFD scores are nan")
            out.mifd, out.mifd_matches = np.full(n, NAN), np.zeros(n, dtype=np.int32)
            out.mifd_masked = np.full(n, NAN) if mask_background else None
        else:
            # pictures [0, vn): the reference planes (plain, then masked), [vn, vn + n): the estimates; pair (variant, i) is picture variant * n + i against vn + i
            found = mifd.detect_device(torch.cat([gray_ref.reshape(vn, h, w), gray_est]), None, ctx)
            scored = [features.score_pairs(mifd, found, v * n, vn, n, ctx) for v in range(variants)]
            counts = found[2].cpu().numpy()
            mifd.check_counts(counts)
            scores_h = np.stack([s[0].cpu().numpy() for s in scored])
            matches_h = np.stack([s[1].cpu().numpy() for s in scored])
            for v in range(variants):
                for i in range(n):
                    if np.isnan(scores_h[v, i]):
                        features.warn_no_score(int(counts[v * n + i, 2]), int(counts[vn + i, 2]), int(matches_h[v, i]))
            out.mifd, out.mifd_matches = scores_h[0], matches_h[0]
            out.mifd_masked = scores_h[1] if mask_background else None
    return out


def lpips_feature_sizes(h, w):
    """[(h_l, w_l)] of the five feature maps of an h x w picture."""
    sizes = []
    for _, _, k, stride, pad, pool in _LPIPS_LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        sizes.append((h, w))
    return sizes


@dataclass
class LPIPSResult:
    """``lpips`` float64 (N,); ``layers`` float64 (5, N), the per-layer scores whose left-to-right sum it is.  ``lpips_masked`` / ``layers_masked``: the same
    against the whitened frame, None without ``mask_background``.  With ``return_maps``, device tensors per layer: ``features[l]`` float32 (sets, N, h_l, w_l, C_l)
    with the sets (reference, masked reference when asked, estimate), ``dist[l]`` float64 (variants, N, h_l, w_l)."""
    lpips: np.ndarray
    layers: np.ndarray
    lpips_masked: np.ndarray = None
    layers_masked: np.ndarray = None
    features: list = None
    dist: list = None


class LPIPS:
    """``lpips.LPIPS(net='alex')`` (version 0.1, eval mode) as scripts/compare_image_pair.py:29-41 calls it, on the GPU (csrc/lpips.hip), from weights alone:
    ``conv_w[l]`` float32 OIHW and ``conv_b[l]`` of the five AlexNet convolutions, ``lin_w[l]`` float32 (C_l,) of the 1 x 1 linear layers (never negative).
    The lpips package and torchvision are absent here, so the network is restated from its published definition (include/hive_mi355x.h above
    ``hive_lpips_create``) and not pinned against them."""

    def __init__(self, conv_w, conv_b, lin_w):
        self.conv_w, self.conv_b, self.lin_w = [], [], []
        for l, (cin, cout, k, _, _, _) in enumerate(_LPIPS_LAYERS):
            for name, a, shape, dest in ((f"conv_w[{l}]", conv_w[l], (cout, cin, k, k), self.conv_w), (f"conv_b[{l}]", conv_b[l], (cout,), self.conv_b),
                                         (f"lin_w[{l}]", lin_w[l], (cout,), self.lin_w)):
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.shape != shape:
                    raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
                dest.append(a)
            if (self.lin_w[l] < 0).any():
                raise ValueError(f"lin_w[{l}]: a linear weight is negative")
        self._native = {}  # id(ctx) -> (ctx, handle)

    @staticmethod
    def _array(value):
        return np.asarray(value.detach().cpu().numpy() if is_torch(value) else value)

    @classmethod
    def from_state_dict(cls, *state_dicts):
        """From one or more state dicts (tensors or arrays), searched in order, in any of three spellings (key names from the packages' published code, which
        is absent here): a whole ``lpips.LPIPS`` state dict, ``net.slice{1..5}.{0,3,6,8,10}.weight|bias`` and ``lin{0..4}.model.1.weight`` (its ``lins.*``
        duplicates and ``scaling_layer.*`` buffers are ignored: the shift and scale are constants of the definition); a torchvision AlexNet state dict,
        ``features.{0,3,6,8,10}.weight|bias``; the package's five-tensor ``alex.pth``, ``lin{k}.model.1.weight`` of shape (1, C, 1, 1).  ValueError naming the
        key: a missing key, a wrong shape, a negative linear weight."""
        def find(names):
            for sd in state_dicts:
                for name in names:
                    if name in sd:
                        return name, cls._array(sd[name])
            raise ValueError(f"missing key: {' or '.join(names)}")
        conv_w, conv_b, lin_w = [], [], []
        for l, (cin, cout, k, _, _, _) in enumerate(_LPIPS_LAYERS):
            for kind, shape, dest in (("weight", (cout, cin, k, k), conv_w), ("bias", (cout,), conv_b)):
                name, a = find((f"net.slice{l + 1}.{_ALEX_INDEX[l]}.{kind}", f"features.{_ALEX_INDEX[l]}.{kind}"))
                if a.shape != shape:
                    raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
                dest.append(a)
            name, a = find((f"lin{l}.model.1.weight",))
            if a.shape != (1, cout, 1, 1):
                raise ValueError(f"{name}: shape {a.shape}, expected {(1, cout, 1, 1)}")
            if (a < 0).any():
                raise ValueError(f"{name}: a linear weight is negative")
            lin_w.append(a.reshape(cout))
        return cls(conv_w, conv_b, lin_w)

    @classmethod
    def from_files(cls, alexnet_path, linear_path=None):
        """``alexnet_path``: a whole lpips.LPIPS state dict, or torchvision's AlexNet weights with the package's ``alex.pth`` as ``linear_path``."""
        import torch
        paths = [alexnet_path] + ([linear_path] if linear_path is not None else [])
        return cls.from_state_dict(*(torch.load(p, map_location="cpu", weights_only=True) for p in paths))

    @classmethod
    def seeded(cls, seed=0):
        """Seeded weights for tests and probes: He-scaled normal convolution weights, biases 0.1 normal, linear weights 4 U[0, 1) / C."""
        rng = np.random.default_rng(seed)
        conv_w, conv_b, lin_w = [], [], []
        for cin, cout, k, _, _, _ in _LPIPS_LAYERS:
            conv_w.append((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
            conv_b.append((0.1 * rng.standard_normal(cout)).astype(np.float32))
            lin_w.append((4.0 * rng.random(cout) / cout).astype(np.float32))
        return cls(conv_w, conv_b, lin_w)

    def state_dict(self):
        """The whole-model spelling ``from_state_dict`` reads, as numpy arrays."""
        sd = {}
        for l in range(5):
            sd[f"net.slice{l + 1}.{_ALEX_INDEX[l]}.weight"], sd[f"net.slice{l + 1}.{_ALEX_INDEX[l]}.bias"] = self.conv_w[l], self.conv_b[l]
            sd[f"lin{l}.model.1.weight"] = self.lin_w[l].reshape(1, -1, 1, 1)
        return sd

    def native(self, ctx):
        """The ``hive_lpips`` handle of this model on ``ctx`` (made on first use)."""
        import ctypes
        entry = self._native.get(id(ctx))
        if entry is None:
            arrays = lambda seq: (ctypes.c_void_p * 5)(*(a.ctypes.data for a in seq))
            handle = ctypes.c_void_p()
            ctx.check(ctx.lib.hive_lpips_create(ctx.handle, arrays(self.conv_w), arrays(self.conv_b), arrays(self.lin_w), ctypes.byref(handle)))
            entry = self._native[id(ctx)] = (ctx, handle)
        return entry[1]

    def close(self):
        for ctx, handle in self._native.values():
            if _lib.alive() and getattr(ctx, "handle", None):
                ctx.lib.hive_lpips_destroy(handle)
        self._native = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def layer(self, index, x, ctx=None):
        """One row of the feature table (``hive_lpips_layer``): ``x`` a float32 device tensor (N, h, w, C_in), the previous row's ReLU map un-pooled (row 0: the
        scaled picture) -> float32 (N, ho, wo, C_out)."""
        import torch
        cin, cout, k, stride, pad, pool = _LPIPS_LAYERS[index]
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[-1] != cin or not x.is_cuda:
            raise ValueError(f"layer {index}: a float32 device tensor (N, h, w, {cin}), got {x.dtype} {tuple(x.shape)}")
        n, h, w = (int(v) for v in x.shape[:3])
        hp, wp = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if pool else (h, w)
        if min(h, w) < (3 if pool else 1) or min(hp, wp) + 2 * pad < k:
            raise ValueError(f"layer {index} has no output at {h} x {w}")
        ctx = _lib.context_for(ctx, x.device)
        x = x.contiguous()
        out = torch.empty((n, (hp + 2 * pad - k) // stride + 1, (wp + 2 * pad - k) // stride + 1, cout), dtype=torch.float32, device=x.device)
        ctx.check(ctx.lib.hive_lpips_layer(self.native(ctx), index, ptr(x), n, h, w, ptr(out)))
        return out

    def __call__(self, ref, est, mask_background=False, return_maps=False, ctx=None):
        """The LPIPS of one pair or a batch: uint8 (H, W, 3) or (N, H, W, 3), numpy arrays or device tensors, never modified; channel k of the picture is
        channel k of the network.  ``mask_background`` as in ``image_similarity``.  Returns an ``LPIPSResult``.  ValueError: the checks of
        ``image_similarity``, with 31 as the smallest side.  The only copy back is the scores."""
        import ctypes
        import torch
        n, h, w, _ = _checked_shapes(ref, est, False, "bgr")
        if min(h, w) < LPIPS_MIN_SIDE:
            raise ValueError(f"{h} x {w} is smaller than {LPIPS_MIN_SIDE} x {LPIPS_MIN_SIDE}, the smallest picture with an output in every LPIPS layer")
        dev = device_of(ref, est)
        ctx = _lib.context_for(ctx, dev)
        ref_d, est_d = on_device(ref, dev, shape=(n, h, w, 3)), on_device(est, dev, shape=(n, h, w, 3))
        variants = 2 if mask_background else 1
        vn = variants * n
        results = torch.empty(6 * vn, dtype=torch.float64, device=dev)  # [0, vn) the scores, then the layer scores [5][variants][n]
        features = dist = None
        feature_ptrs = dist_ptrs = None
        if return_maps:
            sizes = lpips_feature_sizes(h, w)
            features = [torch.empty((variants + 1, n, fh, fw, layer[1]), dtype=torch.float32, device=dev) for (fh, fw), layer in zip(sizes, _LPIPS_LAYERS)]
            dist = [torch.empty((variants, n, fh, fw), dtype=torch.float64, device=dev) for fh, fw in sizes]
            feature_ptrs, dist_ptrs = ((ctypes.c_void_p * 5)(*(ptr(t) for t in seq)) for seq in (features, dist))
        ctx.check(ctx.lib.hive_lpips_forward(self.native(ctx), ptr(ref_d), ptr(est_d), n, h, w, variants, ptr(results), ptr(results[vn:]), feature_ptrs, dist_ptrs))
        host = results.cpu().numpy()  # the only copy back
        scores, layers = host[:vn].reshape(variants, n), host[vn:].reshape(5, variants, n)
        out = LPIPSResult(lpips=scores[0].copy(), layers=layers[:, 0].copy(), features=features, dist=dist)
        if mask_background:
            out.lpips_masked, out.layers_masked = scores[1].copy(), layers[:, 1].copy()
        return out


def compare_images(ref_image, est_image, lpips_fn=None, return_mifd=False, sift=None):
    """``compare_images`` of scripts/compare_image_pair.py:110-133 for one pair of uint8 (H, W, 3) pictures: ``(ssim, psnr, lpips)``, with ``mifd`` behind it when
    ``return_mifd`` is set.  SSIM and PSNR come from ``image_similarity`` with the default channel order.  ``lpips_fn``: an ``LPIPS`` model of this module gives
    the third score (nan, with a warning, for a picture with a side below 31); anything else -- None, or the lpips package's own callable -- is ignored and the
    score is nan.  ``sift``: a ``features.SIFT`` object gives the fourth score, ``mifd(ref_gray, est_gray)`` on the gray planes of the SSIM (nan, with the
    reference's warning, for a pair without enough descriptors or matches); without one the fourth value stays nan."""
    model = lpips_fn if isinstance(lpips_fn, LPIPS) else None
    r = image_similarity(ref_image, est_image, lpips=model, mifd=sift if return_mifd else None)
    scores = (float(r.ssim[0]), float(r.psnr[0]), float(r.lpips[0]) if model is not None else NAN)
    return (*scores, float(r.mifd[0]) if r.mifd is not None else NAN) if return_mifd else scores


def compare_renders(camera_matrix, poses, frames, meshes, *, ms_ssim=False, size=None, names=None, lpips=None, mifd=None):
    """The render-and-score loop of experiments.py:833-852 (and :1594-1614 with ``ms_ssim``): view i is ``render.render_mesh(camera_matrix, poses[i],
    *meshes_i)``, all views share one ``RenderBuffers``, the renders are stacked on the device and scored against ``frames`` (uint8 (N, H, W, 3), numpy or
    device) by one ``image_similarity(..., mask_background=True)`` call.

    ``meshes``: one tuple of meshes used for every view, or a sequence with one tuple per view (the HyperNeRF loop: a per-frame foreground and a shared
    background).  ``names``: per view a dict whose items lead the row (``dataset``, ``camera_feed``, ``config`` of the reference's ``RenderResult``,
    :663-675) or a string taken as ``config``; by default ``camera_feed`` is the view's index.

    Returns ``(renders, rows)``: the uint8 (N, H, W, 3) device tensor and one dict per view with ``ssim``, ``psnr``, ``lpips``, ``ssim_masked``,
    ``psnr_masked``, ``lpips_masked`` behind the names; the two LPIPS scores come from ``lpips``, an ``LPIPS`` model, on the same device tensors, and are nan without
    one (or, with a warning, for pictures with a side below 31).  With ``ms_ssim`` rows also carry ``ms_ssim`` and ``ms_ssim_masked``, and the rule of
    :1609-1610 applies: a masked result with infinite PSNR, an MS-SSIM of exactly 1.0 or (with a model) an LPIPS of exactly 0.0 becomes all nan.
    ``mifd``: a ``features.SIFT`` object; rows then also carry ``mifd`` and ``mifd_masked`` (only then)."""
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
    r = image_similarity(frames, renders, ms_ssim=ms_ssim, mask_background=True, lpips=lpips, mifd=mifd)
    rows = []
    for i in range(n):
        name = names[i] if names is not None else {}
        row = dict(name) if isinstance(name, dict) else {"config": str(name)}
        for key, default in (("dataset", ""), ("camera_feed", i), ("config", "")):
            row.setdefault(key, default)
        row.update(ssim=float(r.ssim[i]), psnr=float(r.psnr[i]), lpips=NAN if lpips is None else float(r.lpips[i]), ssim_masked=float(r.ssim_masked[i]),
                   psnr_masked=float(r.psnr_masked[i]), lpips_masked=NAN if lpips is None else float(r.lpips_masked[i]))
        if ms_ssim:
            row.update(ms_ssim=float(r.ms_ssim[i]), ms_ssim_masked=float(r.ms_ssim_masked[i]))
            if np.isinf(row["psnr_masked"]) or row["ms_ssim_masked"] == 1.0 or row["lpips_masked"] == 0.0:
                row.update(ssim_masked=NAN, psnr_masked=NAN, lpips_masked=NAN, ms_ssim_masked=NAN)
        if mifd is not None:
            row.update(mifd=float(r.mifd[i]), mifd_masked=float(r.mifd_masked[i]))
        rows.append(row)
    return renders, rows


def save_results(rows, path):
    """The JSON list experiments.py:856-857 writes: one object per row (nan and inf in Python's spelling, as ``json.dump`` writes them there)."""
    with open(path, "w") as f:
        json.dump([dict(row) for row in rows], f)
