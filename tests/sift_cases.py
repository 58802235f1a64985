"""Seeded pictures for the SIFT tests, shared by the CPU and the GPU tests: Gaussian blobs and boxes on a flat canvas, a window of it as the reference picture and
the window moved by (dy, dx) = (3, 4) as the estimate (so the mean distance between matched keypoints is near 5), optionally with uniform noise of +-3."""
import numpy as np

MARGIN = 8
SHIFT = (3, 4)  # (dy, dx)
# (H, W, seed, noise): the committed cases; tests/test_sift_cpu.py proves that none of them is empty
CASES = ((48, 64, 0, False), (48, 64, 1, True), (61, 83, 0, False), (61, 83, 2, True), (96, 128, 0, False), (96, 128, 1, True))
# at least this many keypoints per picture and ratio-test survivors per pair
MINIMA = {(48, 64): (8, 5), (61, 83): (8, 5), (96, 128): (25, 15)}


def canvas(H, W, seed):
    rng = np.random.default_rng(seed)
    ch, cw = H + 2 * MARGIN, W + 2 * MARGIN
    img = np.full((ch, cw), 110.0)
    yy, xx = np.mgrid[0:ch, 0:cw].astype(np.float64)
    for _ in range(max(12, H * W // 400)):
        cy, cx = rng.uniform(0, ch), rng.uniform(0, cw)
        sigma, amp = rng.uniform(1.2, 5.0), rng.uniform(40.0, 110.0) * rng.choice((-1.0, 1.0))
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    for _ in range(max(4, H * W // 1500)):
        bh, bw = rng.integers(4, 14), rng.integers(4, 14)
        y0, x0 = rng.integers(0, ch - bh), rng.integers(0, cw - bw)
        img[y0:y0 + bh, x0:x0 + bw] += rng.uniform(30.0, 80.0) * rng.choice((-1.0, 1.0))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), rng


def pair(H, W, seed, noise=False):
    """(ref, est): uint8 (H, W) gray pictures."""
    img, rng = canvas(H, W, seed)
    ref = img[MARGIN:MARGIN + H, MARGIN:MARGIN + W]
    est = img[MARGIN + SHIFT[0]:MARGIN + SHIFT[0] + H, MARGIN + SHIFT[1]:MARGIN + SHIFT[1] + W]
    if noise:
        est = np.clip(est.astype(np.int64) + rng.integers(-3, 4, size=est.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(ref), np.ascontiguousarray(est)


def mask_for(H, W):
    """A uint8 mask that is zero on the right third and on a band at the top."""
    m = np.ones((H, W), dtype=np.uint8)
    m[:, 2 * W // 3:] = 0
    m[:H // 6] = 0
    return m


def gray_to_bgr(gray):
    """(H, W, 3) whose cv2-style gray conversion gives back ``gray``: three equal channels."""
    return np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=2))


_RESTATED = {}


def restated(H, W, seed, noise=False, which="ref", mask=False, nfeatures=0):
    """tests/sift_restatement.py's stages of one picture of a case (a dict: pyramid, candidates, keypoints, descriptors), computed once a process."""
    import sift_restatement
    key = (H, W, seed, noise, which, mask, nfeatures)
    if key not in _RESTATED:
        picture = pair(H, W, seed, noise)[0 if which == "ref" else 1]
        _RESTATED[key] = sift_restatement.detect_and_compute(picture, mask_for(H, W) if mask else None, nfeatures=nfeatures, stages=True)
    return _RESTATED[key]


def restated_score(H, W, seed, noise=False):
    """(score, survivors) of the case by the restatement, without its warnings."""
    import warnings

    import sift_restatement
    a, b = restated(H, W, seed, noise, "ref"), restated(H, W, seed, noise, "est")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return sift_restatement.mifd_from_features(a["keypoints"], a["descriptors"], b["keypoints"], b["descriptors"])
