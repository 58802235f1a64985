"""numpy restatement of the inpainting that ``hive_inpaint_telea`` specifies in include/hive_mi355x.h, written from that text: exact
distances, float64 level set, level order, the window offsets k in ascending order into 64 partial sums, the fixed pairwise tree.  Vectorised
over the pixels of a level (they never read each other) and over the 64 partial sums.  Not a test module; the CPU and GPU inpainting tests import it."""
import numpy as np

FAR = np.int64(1) << 40


def squared_distances(hole):
    """(d_in2 on the hole, d_out2 outside) in one int64 array: the exact squared Euclidean distance to the nearest pixel of the other kind
    (FAR where there is none).  A row scan followed by a column minimum."""
    hole = np.asarray(hole, bool)
    H, W = hole.shape
    xs = np.arange(W)
    ys = np.arange(H)

    def to_kind(kind):  # squared distance of every pixel to the nearest pixel with hole == kind
        row = np.full((H, W), FAR, np.int64)
        for y in range(H):
            at = np.nonzero(hole[y] == kind)[0]
            if len(at):
                row[y] = np.abs(xs[:, None] - at[None, :]).min(axis=1)
        row2 = np.where(row >= FAR, FAR, row * row)
        dy2 = (ys[:, None] - ys[None, :]).astype(np.int64) ** 2  # [y][y']
        return np.minimum((row2[None, :, :] + dy2[:, :, None]).min(axis=1), FAR)

    return np.where(hole, to_kind(False), to_kind(True))


def levels_of(hole, d2):
    """level = the smallest integer L with L * L >= d_in2 on the hole, 0 on known pixels."""
    root = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    root = root - (root * root > d2) + ((root + 1) * (root + 1) <= d2)  # floor of the square root, in integers
    return np.where(hole, root + (root * root < d2), 0)


def inpaint_batch(images, masks, radius, info=None):
    """``images``: arrays [n][H][W] or [n][H][W][C] of one integer type each, filled under the same ``masks`` [n][H][W] (the weights are computed once,
    as the frame form of the library does for colour and depth).  Returns the filled arrays.  The pixels of a level (of all frames) are one vector;
    the 64 partial sums are a second axis, so that one step of the loop adds offset k = base + j to partial j for all j -- every partial still gets
    its terms one at a time in ascending k.  ``info`` receives ``levels`` [n][H][W], ``level_count`` [n] and ``min_weight_sum``."""
    hole = np.asarray(masks) != 0
    n, H, W = hole.shape
    eps = int(radius)
    if not 2 <= eps <= 64:
        raise ValueError("radius must be 2 .. 64")
    if hole.reshape(n, -1).all(axis=1).any():
        raise ValueError("no known pixel")
    images = [np.asarray(image) for image in images]
    tops = [np.iinfo(image.dtype).max for image in images]
    works = [image.reshape(n, H, W, -1).astype(np.float64) for image in images]  # the stored values: integers, exact in float64
    d2 = np.stack([squared_distances(hole[f]) for f in range(n)])
    level = levels_of(hole, d2)
    root = np.sqrt(d2.astype(np.float64))
    T = np.where(hole, root, 1.0 - root)
    side = 2 * eps + 1
    if info is not None:
        info.update(levels=level, level_count=level.reshape(n, -1).max(axis=1), min_weight_sum=np.inf)
    lanes = np.arange(64)[:, None]
    for L in range(1, int(level.max()) + 1):
        fs, ys, xs = np.nonzero(level == L)
        P = len(ys)
        if P == 0:
            continue
        usable = (level < L).ravel()  # flat [n * H * W] views: one index array serves every plane
        Tf = T.ravel()
        Tp = T[fs, ys, xs]
        gTx = (T[fs, ys, np.minimum(xs + 1, W - 1)] - T[fs, ys, np.maximum(xs - 1, 0)]) / 2.0
        gTy = (T[fs, np.minimum(ys + 1, H - 1), xs] - T[fs, np.maximum(ys - 1, 0), xs]) / 2.0
        frame_at = (fs * (H * W))[None, :]
        part_s = np.zeros((64, P))
        part_a = [np.zeros((64, P, work.shape[3])) for work in works]
        for base in range(0, side * side, 64):
            k = base + lanes  # offset of partial j in this step
            dy, dx = k // side - eps, k % side - eps
            r2i = dx * dx + dy * dy
            qx, qy = xs[None, :] + dx, ys[None, :] + dy
            ok = (k < side * side) & (r2i > 0) & (r2i <= eps * eps) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)  # (offsets without a term are computed on clamped coordinates and dropped)
            q = frame_at + qy * W + qx
            ok &= usable.take(q)
            if not ok.any():
                continue
            rx, ry, r2 = (-dx).astype(np.float64), (-dy).astype(np.float64), np.maximum(r2i, 1).astype(np.float64)
            dst = 1.0 / (r2 * np.sqrt(r2))
            lev = 1.0 / (1.0 + np.abs(Tf.take(q) - Tp[None, :]))
            direction = np.abs(rx * gTx[None, :] + ry * gTy[None, :])
            direction = np.where(direction <= 0.01, 1e-6, direction)
            w = (dst * lev) * direction
            ql, qr, qu, qd = q - (qx > 0), q + (qx < W - 1), q - W * (qy > 0), q + W * (qy < H - 1)  # (clamped; a clamped neighbour does not qualify)
            left, right = (qx > 0) & usable.take(ql), (qx < W - 1) & usable.take(qr)
            up, down = (qy > 0) & usable.take(qu), (qy < H - 1) & usable.take(qd)
            both_x, both_y = left & right, up & down
            for work, acc in zip(works, part_a):
                for c in range(work.shape[3]):
                    I = work[:, :, :, c].ravel()
                    centre, Il, Ir, Iu, Id = I.take(q), I.take(ql), I.take(qr), I.take(qu), I.take(qd)
                    gx = np.where(both_x, (Ir - Il) / 2.0, np.where(right, Ir - centre, np.where(left, centre - Il, 0.0)))
                    gy = np.where(both_y, (Id - Iu) / 2.0, np.where(down, Id - centre, np.where(up, centre - Iu, 0.0)))
                    acc[:, :, c] = np.where(ok, acc[:, :, c] + w * (centre + (gx * rx + gy * ry)), acc[:, :, c])
            part_s = np.where(ok, part_s + w, part_s)
        for off in (32, 16, 8, 4, 2, 1):
            part_s[:off] = part_s[:off] + part_s[off:2 * off]
            for acc in part_a:
                acc[:off] = acc[:off] + acc[off:2 * off]
        s = part_s[0]
        if info is not None:
            info["min_weight_sum"] = min(info["min_weight_sum"], float(s.min()))
        for work, acc, top in zip(works, part_a, tops):
            work[fs, ys, xs, :] = np.clip(np.floor(acc[0] / s[:, None] + 0.5), 0, top)
    outs = []
    for image, work in zip(images, works):
        out = image.copy()
        out.reshape(n, H, W, -1)[hole] = work[hole].astype(image.dtype)
        outs.append(out)
    return outs


def inpaint(image, mask, radius, info=None):
    """One image [H][W] or [H][W][C]: the filled image (same dtype and shape).  ``info``: ``levels`` [H][W], ``level_count``, ``min_weight_sum``."""
    out = inpaint_batch([np.asarray(image)[None]], np.asarray(mask)[None], radius, info)[0][0]
    if info is not None:
        info.update(levels=info["levels"][0], level_count=int(info["level_count"][0]))
    return out


def dilate_box(mask, kh=5, kw=5, iterations=5):
    """cv2.dilate with a full kh x kw element (odd sides), `iterations` times, of `mask != 0`: one box maximum, pixels outside ignored."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    ry, rx = iterations * (kh // 2), iterations * (kw // 2)
    out = np.zeros_like(m)
    for y, x in zip(*np.nonzero(m)):
        out[max(0, y - ry):y + ry + 1, max(0, x - rx):x + rx + 1] = True
    return out.astype(np.uint8)


# ---- the holes and images the CPU and GPU tests share ----------------------------------------------------------------------------------------
def disc(H, W, cy, cx, r):
    v, u = np.mgrid[0:H, 0:W]
    return ((v - cy) ** 2 + (u - cx) ** 2 <= r * r).astype(np.uint8)


def interior_holes(H=48, W=64):
    """A disc of radius 11, a square and an ellipse, all away from the border."""
    v, u = np.mgrid[0:H, 0:W]
    m = disc(H, W, 24, 20, 11)
    m[8:15, 40:47] = 1
    m |= (((v - 32) / 9.0) ** 2 + ((u - 48) / 5.0) ** 2 <= 1.0).astype(np.uint8)
    return m


def border_holes(H=48, W=64):
    """Rectangles on the border; rows 20 .. 22 are hole from side to side (their nearest known pixels are only above or below)."""
    m = np.zeros((H, W), np.uint8)
    m[0:6, 0:9] = 1
    m[20:23, :] = 1
    m[H - 5:, W - 12:] = 1
    m[30:41, W - 4:] = 1
    return m


def all_border_holes(H=37, W=53):
    """Holes touching all four borders, and one inside."""
    m = np.zeros((H, W), np.uint8)
    m[0:4, 10:30] = 1
    m[H - 3:, 5:20] = 1
    m[8:25, 0:5] = 1
    m[12:30, W - 6:] = 1
    m |= disc(H, W, 18, 26, 6)
    return m


def ramp(H, W, dtype, C=1):
    """An integer ramp that does not wrap the type: 2 x + y + 5 (u8), 40 x + 25 y + 100 (u16); channel c adds c."""
    v, u = np.mgrid[0:H, 0:W]
    base = 2 * u + v + 5 if np.dtype(dtype) == np.uint8 else 40 * u + 25 * v + 100
    assert base.max() + C <= np.iinfo(dtype).max
    img = np.stack([base + c for c in range(C)], axis=2).astype(dtype)
    return img[:, :, 0] if C == 1 else img


def random_image(H, W, dtype, C=1, seed=0):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, int(np.iinfo(dtype).max) + 1, size=(H, W, C)).astype(dtype)
    return img[:, :, 0] if C == 1 else img
