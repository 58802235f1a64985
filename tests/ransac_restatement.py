"""The pair filter and the homography RANSAC of csrc/pairs.hip restated in numpy: the rules above ``hive_pairs_match`` in include/hive_mi355x.h, operation by
operation, so that the device's H, mask, winning trial and counts can be compared bit for bit.  numpy's element-wise float64 arithmetic rounds once per
operation and never fuses a multiply with an add; sqrt and / are correctly rounded.  The RANSAC is a rule of this project: cv2's USAC_MAGSAC is randomised and
absent, and nothing here is pinned against cv2."""
import numpy as np

import sift_restatement

F = np.float32
EPS = 2.0 ** -40  # a pivot with |a| <= EPS rejects the trial
SQRT2 = 1.4142135623730951
U32 = np.uint64(0xFFFFFFFF)


# ---- the filter ----
def rounded_depth(depth, x, y):
    """depth[rint(y)][rint(x)], half-even on the float32 coordinate, clamped into the picture."""
    h, w = depth.shape
    r = np.clip(np.rint(np.asarray(y, dtype=F)), 0, h - 1).astype(np.int64)
    c = np.clip(np.rint(np.asarray(x, dtype=F)), 0, w - 1).astype(np.int64)
    return depth[r, c]


def match_filter(kp_i, desc_i, kp_j, desc_j, depth_i, depth_j, ratio=0.7, min_features=20):
    """A dict: ``indices`` / ``distances`` the raw 2-NN table (None for a pair below the minimum), ``query`` / ``train`` / ``points_i`` / ``points_j`` /
    ``depth_i`` / ``depth_j`` the survivors in query order, ``ratio_survivors`` and ``survivors`` the two counts."""
    empty = dict(indices=None, distances=None, query=np.zeros(0, np.int32), train=np.zeros(0, np.int32), points_i=np.zeros((0, 2), F), points_j=np.zeros((0, 2), F),
                 depth_i=np.zeros(0, F), depth_j=np.zeros(0, F), ratio_survivors=0, survivors=0)
    if min(len(kp_i), len(kp_j)) < max(min_features, 2):
        return empty
    idx, dist = sift_restatement.knn(desc_i, desc_j)
    by_ratio = ~(dist[:, 0].astype(np.float64) > float(ratio) * dist[:, 1].astype(np.float64))
    q = np.nonzero(by_ratio)[0]
    t = idx[q, 0]
    pi, pj = kp_i[q][:, :2].astype(F), kp_j[t][:, :2].astype(F)
    zi, zj = rounded_depth(depth_i, pi[:, 0], pi[:, 1]), rounded_depth(depth_j, pj[:, 0], pj[:, 1])
    keep = (zi != 0) & (zj != 0)
    return dict(indices=idx, distances=dist, query=q[keep].astype(np.int32), train=t[keep].astype(np.int32), points_i=pi[keep], points_j=pj[keep],
                depth_i=zi[keep].astype(F), depth_j=zj[keep].astype(F), ratio_survivors=int(by_ratio.sum()), survivors=int(keep.sum()))


# ---- the draw ----
def mix(x):
    """lowbias32 on uint32 values held in uint64."""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & U32
    return x ^ (x >> np.uint64(16))


def base_key(seed, pair_key):
    u = lambda v: np.uint64(int(v) & 0xFFFFFFFF)
    return mix(mix(mix(u(seed)) ^ u(pair_key[0])) ^ u(pair_key[1]))


def draw(base, trials, M):
    """(T, 4) int64: the four distinct indices of every trial of ``trials`` (an array), in the order drawn."""
    h = mix(base ^ np.asarray(trials, dtype=np.uint64))
    mulhi = lambda k: (mix(h ^ np.uint64(k)) * np.uint64(M - k)) >> np.uint64(32)
    one = np.uint64(1)
    a = mulhi(0)
    b = mulhi(1)
    b = b + (b >= a) * one
    s0, s1 = np.minimum(a, b), np.maximum(a, b)
    c = mulhi(2)
    c = c + (c >= s0) * one
    c = c + (c >= s1) * one
    u0, u1, u2 = np.minimum(s0, c), np.minimum(np.maximum(s0, c), s1), np.maximum(s1, c)
    d = mulhi(3)
    d = d + (d >= u0) * one
    d = d + (d >= u1) * one
    d = d + (d >= u2) * one
    return np.stack([a, b, c, d], axis=1).astype(np.int64)


# ---- the arithmetic ----
def lane_sum(v, rows=None):
    """Lane l adds the items l, l + 64, ... in ascending order to 0.0; the total is 0.0 + lane 0 + ... + lane 63.  ``v``: (M,) or (M, K); ``rows``: the item
    numbers of the rows of ``v`` (ascending) when only some items add."""
    v = np.asarray(v, dtype=np.float64)
    rows = np.arange(len(v)) if rows is None else np.asarray(rows)
    lanes = np.zeros((64,) + v.shape[1:])
    for k, item in zip(rows, v):
        lanes[k % 64] = lanes[k % 64] + item
    acc = np.zeros(v.shape[1:])
    for l in range(64):
        acc = acc + lanes[l]
    return acc


def normalise(points_i, points_j):
    """(cx_i, cy_i, s_i, cx_j, cy_j, s_j) and whether both mean distances are > 0."""
    out, ok = [], True
    for pts in (points_i, points_j):
        x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
        n = float(len(pts))
        cx, cy = lane_sum(x) / n, lane_sum(y) / n
        dx, dy = x - cx, y - cy
        m = lane_sum(np.sqrt(dx * dx + dy * dy)) / n
        ok = ok and bool(m > 0)
        with np.errstate(all="ignore"):
            out += [cx, cy, np.float64(SQRT2) / m]
    return out, ok


def normalised(points_i, points_j, nm):
    """(M, 4) float64: X, Y, U, V."""
    cxi, cyi, si, cxj, cyj, sj = nm
    return np.stack([(points_i[:, 0].astype(np.float64) - cxi) * si, (points_i[:, 1].astype(np.float64) - cyi) * si,
                     (points_j[:, 0].astype(np.float64) - cxj) * sj, (points_j[:, 1].astype(np.float64) - cyj) * sj], axis=1)


def equations(p):
    """The two rows (.., 9) of correspondences p (.., 4), h33 = 1."""
    X, Y, U, V = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    one, zero = np.ones_like(X), np.zeros_like(X)
    r1 = np.stack([X, Y, one, zero, zero, zero, -(U * X), -(U * Y), U], axis=-1)
    r2 = np.stack([zero, zero, zero, X, Y, one, -(V * X), -(V * Y), V], axis=-1)
    return r1, r2


def solve8(a):
    """a (T, 8, 9) -> (h (T, 8), ok (T,)): elimination with partial pivoting, the lowest row on a tie, |pivot| <= EPS rejects; then back substitution."""
    a = np.array(a, dtype=np.float64)
    T = len(a)
    ar = np.arange(T)
    ok = np.ones(T, dtype=bool)
    with np.errstate(all="ignore"):
        for col in range(8):
            sub = np.abs(a[:, col:, col])
            piv = col + np.argmax(sub, axis=1)  # the first maximum: the lowest row
            ok &= sub[ar, piv - col] > EPS
            low = a[ar, piv, :].copy()
            a[ar, piv, :] = a[:, col, :]
            a[:, col, :] = low
            for r in range(col + 1, 8):
                f = a[:, r, col] / a[:, col, col]
                a[:, r, col + 1:] = a[:, r, col + 1:] - f[:, None] * a[:, col, col + 1:]
        h = np.zeros((T, 8))
        for r in range(7, -1, -1):
            acc = a[:, r, 8].copy()
            for k in range(r + 1, 8):
                acc = acc - a[:, r, k] * h[:, k]
            h[:, r] = acc / a[:, r, r]
    return h, ok


def inliers(h, p, thr2):
    """h (T, 8), p (M, 4) -> (T, M) bool."""
    X, Y, U, V = (p[None, :, k] for k in range(4))
    g = [h[:, k, None] for k in range(8)]
    with np.errstate(all="ignore"):
        w = (g[6] * X + g[7] * Y) + 1.0
        pu = (g[0] * X + g[1] * Y) + g[2]
        pv = (g[3] * X + g[4] * Y) + g[5]
        du, dv = pu / w - U, pv / w - V
        e2 = du * du + dv * dv
        return (w > 0) & (e2 <= thr2)


def denormalise(h, nm):
    cxi, cyi, si, cxj, cyj, sj = nm
    h = np.append(h, 1.0).reshape(3, 3)
    A = np.zeros((3, 3))
    for r in range(3):
        A[r, 0], A[r, 1] = h[r, 0] * si, h[r, 1] * si
        A[r, 2] = (h[r, 2] - A[r, 0] * cxi) - A[r, 1] * cyi
    B = np.zeros((3, 3))
    for c in range(3):
        B[0, c] = A[0, c] / sj + cxj * A[2, c]
        B[1, c] = A[1, c] / sj + cyj * A[2, c]
        B[2, c] = A[2, c]
    with np.errstate(all="ignore"):
        return B / B[2, 2]


def ransac(points_i, points_j, threshold=3.0, trials=2000, seed=0, pair_key=(0, 0), min_count=0, chunk=256):
    """A dict: ``H`` float64 (3, 3) (NaN without a model), ``mask`` uint8 (M,), ``trial`` (-1 without a model), ``winner_count``, ``count``."""
    points_i, points_j = np.asarray(points_i, dtype=F).reshape(-1, 2), np.asarray(points_j, dtype=F).reshape(-1, 2)
    M = len(points_i)
    none = dict(H=np.full((3, 3), np.nan), mask=np.zeros(M, np.uint8), trial=-1, winner_count=0, count=0)
    if M < max(min_count, 4):
        return none
    nm, ok = normalise(points_i, points_j)
    if not ok:
        return none
    p = normalised(points_i, points_j, nm)
    thr = float(threshold) * nm[5]
    thr2 = thr * thr
    base = base_key(seed, pair_key)
    best, best_t, best_h = -1, -1, None
    for t0 in range(0, trials, chunk):
        t = np.arange(t0, min(trials, t0 + chunk))
        sample = draw(base, t, M)  # (T, 4)
        r1, r2 = equations(p[sample])  # (T, 4, 9) each
        a = np.stack([r1, r2], axis=2).reshape(len(t), 8, 9)  # rows 2k and 2k + 1
        h, solved = solve8(a)
        count = np.where(solved, inliers(h, p, thr2).sum(axis=1), -1)
        k = int(np.argmax(count))  # the first maximum: the lowest trial
        if count[k] > best:
            best, best_t, best_h = int(count[k]), int(t[k]), h[k].copy()
    if best < 0:
        return none
    mask = inliers(best_h[None], p, thr2)[0]
    rows = np.nonzero(mask)[0]
    r1, r2 = equations(p[rows])
    terms = np.zeros((2, len(rows), 44))
    n = 0
    for a_ in range(8):
        for b_ in range(a_, 8):
            terms[0, :, n], terms[1, :, n] = r1[:, a_] * r1[:, b_], r2[:, a_] * r2[:, b_]
            n += 1
    for a_ in range(8):
        terms[0, :, 36 + a_], terms[1, :, 36 + a_] = r1[:, a_] * r1[:, 8], r2[:, a_] * r2[:, 8]
    # per item first the r1 product, then the r2 product: interleave them as two items of the same lane
    lanes = np.zeros((64, 44))
    for k, first, second in zip(rows, terms[0], terms[1]):
        lanes[k % 64] = lanes[k % 64] + first
        lanes[k % 64] = lanes[k % 64] + second
    total = np.zeros(44)
    for l in range(64):
        total = total + lanes[l]
    a = np.zeros((1, 8, 9))
    n = 0
    for a_ in range(8):
        for b_ in range(a_, 8):
            a[0, a_, b_] = a[0, b_, a_] = total[n]
            n += 1
    a[0, :, 8] = total[36:]
    hr, solved = solve8(a)
    refit_mask = inliers(hr, p, thr2)[0] if solved[0] else np.zeros(M, bool)
    refit = bool(solved[0]) and int(refit_mask.sum()) >= best
    h, final = (hr[0], refit_mask) if refit else (best_h, mask)
    return dict(H=denormalise(h, nm), mask=final.astype(np.uint8), trial=best_t, winner_count=best, count=int(final.sum()))
