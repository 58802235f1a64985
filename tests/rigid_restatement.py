"""The rigid (optionally similarity) RANSAC of csrc/register.hip restated in numpy: the rules above ``hive_ransac_rigid`` in include/hive_mi355x.h, operation by
operation, so that the device's T, scale, rms, mask, winning trial and counts can be compared bit for bit.  numpy's element-wise float64 arithmetic rounds once
per operation and never fuses a multiply with an add; sqrt and / are correctly rounded.  The hash, the draw and the lane sum are tests/ransac_restatement.py's.
The RANSAC is a rule of this project: cv2's estimateAffine3D, Open3D's correspondence RANSAC, BundleFusion and COLMAP are absent, and nothing here is pinned
against them."""
import numpy as np

import ransac_restatement as RR

F = np.float32
SWEEPS = 7            # register.hip's RG_SWEEPS: see tests/register_cases.py, SWEEPS_MEASURED
DEGENERATE = 2.0 ** -20
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---- the points ----
def back_project(rows, camera):
    """rows float32 (M, >= 6) -> (p (M, 3), q (M, 3)) float64.  ``camera`` (fx, fy, cx, cy): a row is x_i, y_i, x_j, y_j, depth_i, depth_j; None: a row is
    X_i Y_i Z_i X_j Y_j Z_j."""
    rows = np.asarray(rows, dtype=F)
    w = rows.astype(np.float64)
    if camera is None:
        return w[:, 0:3].copy(), w[:, 3:6].copy()
    fx, fy, cx, cy = (np.float64(v) for v in camera)
    with np.errstate(all="ignore"):
        side = lambda x, y, z: np.stack([((x - cx) * z) / fx, ((y - cy) * z) / fy, z], axis=1)
        return side(w[:, 0], w[:, 1], w[:, 4]), side(w[:, 2], w[:, 3], w[:, 5])


def camera_of(camera_matrix):
    K = np.asarray(camera_matrix, dtype=np.float64)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def draw3(base, trials, M):
    """(T, 3) int64: the first three draws of the four-draw rule."""
    h = RR.mix(base ^ np.asarray(trials, dtype=np.uint64))
    mulhi = lambda k: (RR.mix(h ^ np.uint64(k)) * np.uint64(M - k)) >> np.uint64(32)
    one = np.uint64(1)
    a = mulhi(0)
    b = mulhi(1)
    b = b + (b >= a) * one
    s0, s1 = np.minimum(a, b), np.maximum(a, b)
    c = mulhi(2)
    c = c + (c >= s0) * one
    c = c + (c >= s1) * one
    return np.stack([a, b, c], axis=1).astype(np.int64)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]],
                    axis=-1)


def degenerate(s):
    """s (T, 3, 3): the three sample points of one side -> (T,) bool."""
    with np.errstate(all="ignore"):
        e1, e2 = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
        n = cross3(e1, e2)
        return dot3(n, n) <= (DEGENERATE * dot3(e1, e1)) * dot3(e2, e2)


# ---- horn ----
def horn_matrix(S):
    """S (T, 3, 3), S[a][b] = sum p'_a q'_b -> Horn's symmetric (T, 4, 4)."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[:, a, b] for a in range(3) for b in range(3))
    N = np.zeros((len(S), 4, 4))
    N[:, 0, 0] = (xx + yy) + zz
    N[:, 1, 1] = (xx - yy) - zz
    N[:, 2, 2] = (yy - xx) - zz
    N[:, 3, 3] = (zz - xx) - yy
    N[:, 0, 1] = N[:, 1, 0] = yz - zy
    N[:, 0, 2] = N[:, 2, 0] = zx - xz
    N[:, 0, 3] = N[:, 3, 0] = xy - yx
    N[:, 1, 2] = N[:, 2, 1] = xy + yx
    N[:, 1, 3] = N[:, 3, 1] = zx + xz
    N[:, 2, 3] = N[:, 3, 2] = yz + zy
    return N


def jacobi(N, sweeps=SWEEPS, history=None):
    """Cyclic Jacobi on symmetric (T, 4, 4): (diagonalised a, eigenvector columns v).  ``history``: a list that receives, after every sweep, the largest
    off-diagonal norm relative to the Frobenius norm of the input."""
    a, T = np.array(N, dtype=np.float64), len(N)
    v = np.tile(np.eye(4), (T, 1, 1))
    frob = np.sqrt((a * a).sum(axis=(1, 2)))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                app, aqq, apq = a[:, p, p].copy(), a[:, q, q].copy(), a[:, p, q].copy()
                turn = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                new = a.copy()
                new[:, p, p], new[:, q, q] = app - t * apq, aqq + t * apq
                new[:, p, q] = new[:, q, p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = a[:, r, p], a[:, r, q]
                        new[:, r, p] = new[:, p, r] = c * arp - s * arq
                        new[:, r, q] = new[:, q, r] = s * arp + c * arq
                nv = v.copy()
                for r in range(4):
                    vrp, vrq = v[:, r, p], v[:, r, q]
                    nv[:, r, p], nv[:, r, q] = c * vrp - s * vrq, s * vrp + c * vrq
                a = np.where(turn[:, None, None], new, a)
                v = np.where(turn[:, None, None], nv, v)
            if history is not None:
                off = a.copy()
                off[:, range(4), range(4)] = 0.0
                history.append(float(np.max(np.where(frob > 0, np.sqrt((off * off).sum(axis=(1, 2))) / np.where(frob > 0, frob, 1.0), 0.0))))
    return a, v


def horn(cp, cq, S, sp, sq, with_scale, sweeps=SWEEPS):
    """Centroids (T, 3), centred sums S (T, 3, 3), sp, sq (T,) -> (A (T, 3, 3) = scale R, t (T, 3), scale (T,), ok (T,))."""
    T = len(S)
    ar = np.arange(T)
    a, v = jacobi(horn_matrix(S), sweeps)
    with np.errstate(all="ignore"):
        k = np.argmax(a[:, range(4), range(4)], axis=1)  # the first maximum: the lowest index
        qt = v[ar, :, k]
        w, x, y, z = (qt[:, i].copy() for i in range(4))
        first = np.where(x != 0.0, x, np.where(y != 0.0, y, z))
        flip = (w < 0.0) | ((w == 0.0) & (first < 0.0))
        sg = np.where(flip, -1.0, 1.0)
        w, x, y, z = sg * w, sg * x, sg * y, sg * z
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        R = np.zeros((T, 3, 3))
        R[:, 0, 0] = ((w * w + x * x) - y * y) - z * z
        R[:, 0, 1] = 2.0 * (x * y - w * z)
        R[:, 0, 2] = 2.0 * (x * z + w * y)
        R[:, 1, 0] = 2.0 * (x * y + w * z)
        R[:, 1, 1] = ((w * w - x * x) + y * y) - z * z
        R[:, 1, 2] = 2.0 * (y * z - w * x)
        R[:, 2, 0] = 2.0 * (x * z - w * y)
        R[:, 2, 1] = 2.0 * (y * z + w * x)
        R[:, 2, 2] = ((w * w - x * x) - y * y) + z * z
        scale = np.sqrt(sq / sp) if with_scale else np.ones(T)
        A = scale[:, None, None] * R
        t = np.stack([cq[:, r] - ((A[:, r, 0] * cp[:, 0] + A[:, r, 1] * cp[:, 1]) + A[:, r, 2] * cp[:, 2]) for r in range(3)], axis=1)
        ok = (sp != 0.0) & (sq != 0.0) & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(t).all(axis=1) & np.isfinite(scale) & np.isfinite(sp) & np.isfinite(sq)
    return A, t, scale, ok


def centred_sums(dp, dq):
    """The terms of one point: dp, dq (.., 3) centred -> (.., 11): p'_a q'_b row-major, |p'|^2, |q'|^2."""
    terms = [dp[..., a] * dq[..., b] for a in range(3) for b in range(3)]
    return np.stack(terms + [dot3(dp, dp), dot3(dq, dq)], axis=-1)


def minimal(p, q, sample, with_scale, sweeps=SWEEPS):
    """The model of the minimal samples ``sample`` (T, 3): sums over the three points in the order drawn, each added to 0.0."""
    sp_, sq_ = p[sample], q[sample]  # (T, 3, 3)
    with np.errstate(all="ignore"):
        bad = degenerate(sp_) | degenerate(sq_)
        cp = ((sp_[:, 0] + sp_[:, 1]) + sp_[:, 2]) / 3.0
        cq = ((sq_[:, 0] + sq_[:, 1]) + sq_[:, 2]) / 3.0
        acc = np.zeros((len(sample), 11))
        for k in range(3):
            acc = acc + centred_sums(sp_[:, k] - cp, sq_[:, k] - cq)
    A, t, scale, ok = horn(cp, cq, acc[:, :9].reshape(-1, 3, 3), acc[:, 9], acc[:, 10], with_scale, sweeps)
    return A, t, scale, ok & ~bad


def residual2(A, t, p, q):
    """A (T, 3, 3), t (T, 3), points (M, 3) -> d . d (T, M)."""
    with np.errstate(all="ignore"):
        d = [(((A[:, r, 0, None] * p[None, :, 0] + A[:, r, 1, None] * p[None, :, 1]) + A[:, r, 2, None] * p[None, :, 2]) + t[:, r, None]) - q[None, :, r] for r in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def inliers(A, t, p, q, thr2):
    with np.errstate(all="ignore"):
        return residual2(A, t, p, q) <= thr2


def refit(p, q, mask, with_scale, sweeps=SWEEPS):
    """``horn`` over the rows of ``mask`` in two passes of lane sums: centroids, then centred sums."""
    rows = np.nonzero(mask)[0]
    n = float(len(rows))
    with np.errstate(all="ignore"):
        cp, cq = RR.lane_sum(p[rows], rows) / n, RR.lane_sum(q[rows], rows) / n
        sums = RR.lane_sum(centred_sums(p[rows] - cp, q[rows] - cq), rows)
    return horn(cp[None], cq[None], sums[None, :9].reshape(1, 3, 3), sums[None, 9], sums[None, 10], with_scale, sweeps)


def ransac(rows, camera=None, threshold=0.05, trials=2000, seed=0, pair_key=(0, 0), min_count=0, with_scale=False, chunk=256, sweeps=SWEEPS):
    """A dict: ``T`` float64 (4, 4), ``scale``, ``rms`` (NaN without a model), ``mask`` uint8 (M,), ``trial`` (-1 without a model), ``winner_count``, ``count``."""
    rows = np.asarray(rows, dtype=F)
    M = len(rows)
    rows = rows.reshape(M, -1) if M else np.zeros((0, 6), dtype=F)
    none = dict(T=np.full((4, 4), np.nan), scale=np.nan, rms=np.nan, mask=np.zeros(M, np.uint8), trial=-1, winner_count=0, count=0)
    if M < max(min_count, 3):
        return none
    p, q = back_project(rows, camera)
    thr2 = np.float64(threshold) * np.float64(threshold)
    base = RR.base_key(seed, pair_key)
    best, best_t, best_model = -1, -1, None
    for t0 in range(0, trials, chunk):
        t = np.arange(t0, min(trials, t0 + chunk))
        A, tr, scale, ok = minimal(p, q, draw3(base, t, M), with_scale, sweeps)
        count = np.where(ok, inliers(A, tr, p, q, thr2).sum(axis=1), -1)
        k = int(np.argmax(count))  # the first maximum: the lowest trial
        if count[k] > best:
            best, best_t, best_model = int(count[k]), int(t[k]), (A[k].copy(), tr[k].copy(), scale[k])
    if best < 0:
        return none
    A, tr, scale = best_model
    mask = inliers(A[None], tr[None], p, q, thr2)[0]
    count = best
    Ar, tr_r, scale_r, ok = refit(p, q, mask, with_scale, sweeps)
    refit_mask = inliers(Ar, tr_r, p, q, thr2)[0] if ok[0] else np.zeros(M, bool)
    if bool(ok[0]) and int(refit_mask.sum()) >= best:
        A, tr, scale, mask, count = Ar[0], tr_r[0], scale_r[0], refit_mask, int(refit_mask.sum())
    rows_in = np.nonzero(mask)[0]
    with np.errstate(all="ignore"):
        rms = np.sqrt(RR.lane_sum(residual2(A[None], tr[None], p[rows_in], q[rows_in])[0], rows_in) / np.float64(count))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = A, tr
    return dict(T=T, scale=float(scale), rms=float(rms), mask=mask.astype(np.uint8), trial=best_t, winner_count=best, count=count)
