"""The picture-score rules (include/hive_mi355x.h, above hive_similarity_ssim_psnr) stated literally: gray, the mask, SSIM and PSNR in numpy with integer window
sums by summed-area tables, MS-SSIM in torch on the CPU in float64 through conv2d and avg_pool2d.  What csrc/similarity.hip must reproduce: the gray planes, the S
map, the squared-difference sum and the PSNR bit for bit; MS-SSIM within a stated tolerance.  numpy's element-wise float64 operators round once per operation (no
fused multiply-add), like the kernels' build.  Imports nothing from the package."""
import numpy as np

WIN = 7
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gray(image, channel_order="bgr"):
    """cv2's 8-bit COLOR_BGR2GRAY (OpenCV 3.4, from recall) on the channels in memory order; "rgb" swaps the outer weights."""
    w0, w2 = {"bgr": (1868, 4899), "rgb": (4899, 1868)}[channel_order]
    c = np.asarray(image).astype(np.int64)
    return ((w0 * c[..., 0] + 9617 * c[..., 1] + w2 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def mask_background(ref, est):
    """masked_frame[color_np == [255, 255, 255]] = 255: per channel."""
    out = np.array(ref, copy=True)
    out[np.asarray(est) == [255, 255, 255]] = 255
    return out


def _window_sums(a):
    """Exact sums of the int64 plane over every 7 x 7 window inside it, by a summed-area table -> (H - 6, W - 6)."""
    t = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    t[1:, 1:] = a.cumsum(0).cumsum(1)
    return t[WIN:, WIN:] - t[:-WIN, WIN:] - t[WIN:, :-WIN] + t[:-WIN, :-WIN]


def ssim_map(ref_gray, est_gray):
    """The map S (H - 6, W - 6) of skimage's structural_similarity(win_size=7) on uint8, cropped by 3."""
    x, y = np.asarray(ref_gray).astype(np.int64), np.asarray(est_gray).astype(np.int64)
    Sx, Sy, Sxx, Syy, Sxy = (_window_sums(p).astype(np.float64) for p in (x, y, x * x, y * y, x * y))
    ux, uy, uxx, uyy, uxy = Sx / 49.0, Sy / 49.0, Sxx / 49.0, Syy / 49.0, Sxy / 49.0
    vx = (49.0 / 48.0) * (uxx - ux * ux)
    vy = (49.0 / 48.0) * (uyy - uy * uy)
    vxy = (49.0 / 48.0) * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def _tree(v):
    """v[t] += v[t + off] for t < off, off = 128 .. 1 -> v[0]."""
    off = 128
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off //= 2
    return v[0]


def ssim_score(S):
    """The mean of the map in the kernels' stated order: per 32 x 32 tile (p = 32 r + c) thread t of 256 adds its values p = t, t + 256, t + 512, t + 768 to 0.0
    (values outside the map are not added: here + 0.0, which changes nothing), the tree gives the tile's partial; the partials, tiles row-major, are added the
    same way (thread t takes partials t, t + 256, ...), and the sum is divided by the number of values."""
    Hm, Wm = S.shape
    partials = []
    for i0 in range(0, Hm, 32):
        for j0 in range(0, Wm, 32):
            tile = np.zeros((32, 32))
            part = S[i0:i0 + 32, j0:j0 + 32]
            tile[:part.shape[0], :part.shape[1]] = part
            v = np.zeros(256)
            for chunk in tile.reshape(4, 256):
                v = v + chunk
            partials.append(_tree(v))
    padded = np.zeros(-(-len(partials) // 256) * 256)
    padded[:len(partials)] = partials
    v = np.zeros(256)
    for chunk in padded.reshape(-1, 256):
        v = v + chunk
    return float(_tree(v) / float(Hm * Wm))


def sse(ref_gray, est_gray):
    d = np.asarray(ref_gray).astype(np.int64) - np.asarray(est_gray).astype(np.int64)
    return int((d * d).sum())


def psnr_from_sse(total, H, W):
    if total == 0:
        return float("inf")
    return float(10 * np.log10(65025.0 / (total / (H * W))))


def compare(ref, est, channel_order="bgr"):
    """-> dict(gray_ref, gray_est, map, ssim, sse, psnr) of one pair; ssim is the mean of the map summed in the kernels' stated order."""
    gr, ge = gray(ref, channel_order), gray(est, channel_order)
    S = ssim_map(gr, ge)
    total = sse(gr, ge)
    return {"gray_ref": gr, "gray_est": ge, "map": S, "ssim": ssim_score(S), "sse": total, "psnr": psnr_from_sse(total, *gr.shape)}


def ms_window():
    """The 11-tap Gaussian, sigma 1.5, float64."""
    g = np.exp(-(np.arange(11, dtype=np.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def ms_ssim(ref, est, return_levels=False):
    """pytorch_msssim.ms_ssim(X, Y, data_range=1.0, size_average=True) of one uint8 (H, W, 3) pair in float64."""
    import torch
    import torch.nn.functional as F
    ref, est = np.asarray(ref), np.asarray(est)
    if min(ref.shape[:2]) <= 160:
        raise ValueError("the smaller side must exceed 160")
    X = torch.from_numpy((ref / 255.).transpose((2, 0, 1)).reshape((1, 3, *ref.shape[:2])).copy())
    Y = torch.from_numpy((est / 255.).transpose((2, 0, 1)).reshape((1, 3, *est.shape[:2])).copy())
    g = torch.from_numpy(ms_window())
    win_h, win_w = g.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)
    G = lambda t: F.conv2d(F.conv2d(t, win_h, groups=3), win_w, groups=3)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    values = []
    for level in range(5):
        mu1, mu2 = G(X), G(Y)
        s1, s2, s12 = G(X * X) - mu1 * mu1, G(Y * Y) - mu2 * mu2, G(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map_ = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        values.append(torch.relu((cs_map if level < 4 else ssim_map_).flatten(2).mean(-1)))  # (1, 3)
        if level < 4:
            padding = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=padding), F.avg_pool2d(Y, kernel_size=2, padding=padding)
    stack = torch.stack(values, 0)  # (5, 1, 3)
    score = float(torch.prod(stack ** torch.tensor(MS_WEIGHTS, dtype=torch.float64).view(-1, 1, 1), dim=0).mean())
    return (score, stack[:, 0].numpy()) if return_levels else score


def smooth_pair(H, W, seed=0, whites=0):
    """A reference that is smooth plus noise and an estimate that is the reference plus integer noise in [-20, 20], uint8 (H, W, 3); `whites` channel values of
    the estimate (single channels, seeded places) are then set to 255."""
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 70 * np.sin(ii / 9.0 + k) * np.cos(jj / 11.0 - k) for k in range(3)], -1)
    ref = np.clip(np.rint(base + rng.normal(0, 6, base.shape)), 0, 255).astype(np.uint8)
    est = np.clip(ref.astype(np.int64) + rng.integers(-20, 21, ref.shape), 0, 255).astype(np.uint8)
    for _ in range(whites):
        est[rng.integers(H), rng.integers(W), rng.integers(3)] = 255
    return ref, est
