"""The pictures and settings both JPEG test files run (tests/test_jpeg_cpu.py against Pillow, tests/test_jpeg_gpu.py against the restatement), and the
restatement's result of every case, computed once per process."""
import functools

import numpy as np

import jpeg_restatement as R

# 72 x 104, 24 x 40: H mod 16 = 8, where the chroma rows of 4:2:0 repeat AFTER down-sampling; 9 x 17, 37 x 61, 57 x 131, 40 x 24: dummy luminance blocks right
# and below; 16 x 2064: 129 MCUs in one interval (past a wave and a workgroup); 1040 x 16: 65 intervals in 4:2:0 and 130 in 4:4:4 (the RST index wraps)
SIZES = ((1, 1), (8, 8), (16, 16), (9, 17), (37, 61), (24, 40), (40, 24), (72, 104), (57, 131), (16, 2064), (1040, 16))
QUALITIES = (1, 30, 90, 100)
SUBSAMPLINGS = ("4:4:4", "4:2:0")
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}
CONTENTS = ("gradient_noise", "noise", "flat", "blocks", "impulses")
LARGE = (480, 640)
# 257 MCU rows in one picture, outside SIZES: the picture-level scan of the intervals takes a second chunk of 256.  (height, width, content, quality, subsampling)
LONG = ((2056, 8, "gradient_noise", 90, "4:4:4"), (4112, 8, "gradient_noise", 90, "4:2:0"))


@functools.lru_cache(maxsize=None)
def picture(height, width, content):
    """An (H, W, 3) uint8 picture, the same in every process (read-only)."""
    rng = np.random.default_rng(1000 * height + width)
    yy, xx = np.mgrid[0:height, 0:width]
    if content == "gradient_noise":  # a gradient with a noise patch in its middle
        a = np.stack([(3 * xx + yy) % 256, (2 * yy + 64) % 256, (xx + 2 * yy) // 2 % 256], axis=2).astype(np.uint8)
        h0, h1, w0, w1 = height // 4, max(height // 4 + 1, 3 * height // 4), width // 4, max(width // 4 + 1, 3 * width // 4)
        a[h0:h1, w0:w1] = rng.integers(0, 256, (h1 - h0, w1 - w0, 3), dtype=np.uint8)
    elif content == "noise":
        a = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    elif content == "flat":
        a = np.full((height, width, 3), (200, 120, 40), np.uint8)
    elif content == "blocks":  # 8 x 8 blocks of all 0 and all 255 in turn along a row (the largest DC difference), rows offset by one
        a = np.repeat((((xx // 8 + yy // 8) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    elif content == "impulses":  # single pixels on flat ground
        a = np.full((height, width, 3), 128, np.uint8)
        for _ in range(max(1, height * width // 200)):
            a[rng.integers(height), rng.integers(width)] = rng.integers(0, 256, 3)
    else:
        raise ValueError(content)
    a.setflags(write=False)
    return a


def cases(with_large=False):
    """(height, width, content) of every picture of the list; with ``with_large`` one 480 x 640 picture more."""
    out = [(h, w, c) for h, w in SIZES for c in CONTENTS]
    return out + [LARGE + ("gradient_noise",)] if with_large else out


@functools.lru_cache(maxsize=None)
def restated(height, width, content, quality, subsampling):
    """(file, counters) of the restatement for one case."""
    return R.encode_counted(picture(height, width, content), quality, subsampling)
