"""The rules of include/hive_mi355x.h above ``hive_sift_create`` -- SIFT with cv2.SIFT.create()'s parameters as recalled from OpenCV 4.x, the exact
2-nearest-neighbour matcher and MIFD (scripts/compare_image_pair.py:44-97) -- restated in numpy float32: one rounding per operation, the same polynomial exp /
atan2 / sin / cos, the same summation orders as csrc/sift.hip.  Imports nothing from the package.  cv2 is absent: nothing here is pinned against cv2 or FLANN."""
import warnings

import numpy as np

F = np.float32
NAN = float("nan")
BORDER, STEPS, ORI_BINS, D, NB = 5, 5, 36, 4, 8
FLT_EPSILON = F(np.finfo(np.float32).eps)


# ---- the stated polynomials ----
def sift_exp(x):
    x = np.maximum(np.asarray(x, dtype=F), F(-87.0))
    n = np.rint(x * F(1.4426950408889634))
    r = x - n * F(0.693145751953125)
    r = r - n * F(1.42860682030941723212e-6)
    p = F(1.0 / 5040.0)
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        p = p * r + F(c)
    return np.ldexp(p, n.astype(np.int32)).astype(F)


_P1, _P3 = F(0.9997878412794807 * 57.29577951308232), F(-0.3258083974640975 * 57.29577951308232)
_P5, _P7 = F(0.1555786518463281 * 57.29577951308232), F(-0.04432655554792128 * 57.29577951308232)


def sift_atan2_deg(y, x):
    y, x = np.asarray(y, dtype=F), np.asarray(x, dtype=F)
    ax, ay = np.abs(x), np.abs(y)
    eps = F(2.220446049250313e-16)
    first = ax >= ay
    c = np.where(first, ay, ax) / (np.where(first, ax, ay) + eps)
    c2 = c * c
    poly = (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    a = np.where(first, poly, F(90.0) - poly)
    a = np.where(x < 0, F(180.0) - a, a)
    a = np.where(y < 0, F(360.0) - a, a)
    return a.astype(F)


def sift_sincos_deg(a):
    """(cos, sin) of ``a`` degrees in [0, 360]."""
    a = F(a)
    q = np.rint(a * F(1.0 / 90.0))
    t = (a - q * F(90.0)) * F(3.141592653589793 / 180.0)
    u = t * t
    s = F(1.0 / 362880.0)
    for c in (-1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        s = s * u + F(c)
    s = s * t
    c_ = F(-1.0 / 3628800.0)
    for c in (1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0):
        c_ = c_ * u + F(c)
    k = int(q) & 3
    return ((c_, s), (-s, c_), (-c_, -s), (s, -c_))[k]


# ---- pyramid ----
def blur_sigmas(n_octave_layers=3, sigma=1.6):
    """[0] the base blur, [i] the blur from layer i - 1 to layer i (float64)."""
    sig = [np.sqrt(max(sigma * sigma - 4 * 0.5 * 0.5, 0.01))]
    k = 2.0 ** (1.0 / n_octave_layers)
    for i in range(1, n_octave_layers + 3):
        prev = sigma * k ** (i - 1)
        total = prev * k
        sig.append(np.sqrt(total * total - prev * prev))
    return sig


def gaussian_taps(sig):
    n = int(np.rint(8 * sig + 1)) | 1
    g = np.exp(-(np.arange(n, dtype=np.float64) - n // 2) ** 2 / (2 * sig * sig))
    return (g / g.sum()).astype(F)


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    m = np.mod(i, period)
    return np.where(m < n, m, period - m)


def blur(img, taps):
    """Along the row, then along the column; products added in ascending tap order."""
    h, w = img.shape
    R = len(taps) // 2
    cols = reflect101(np.arange(-R, w + R), w)
    acc = taps[0] * img[:, cols[0:w]]
    for k in range(1, len(taps)):
        acc = acc + taps[k] * img[:, cols[k:k + w]]
    rows = reflect101(np.arange(-R, h + R), h)
    out = taps[0] * acc[rows[0:h], :]
    for k in range(1, len(taps)):
        out = out + taps[k] * acc[rows[k:k + h], :]
    return out.astype(F)


def base_image(gray):
    H, W = gray.shape
    g = gray.astype(F)

    def axis(n_out, n_in):
        s = (np.arange(n_out, dtype=F) + F(0.5)) * F(0.5) - F(0.5)
        i0 = np.floor(s)
        fr = (s - i0).astype(F)
        i0 = i0.astype(np.int64)
        return np.maximum(i0, 0), np.minimum(i0 + 1, n_in - 1), fr
    ya, yb, fy = axis(2 * H, H)
    xa, xb, fx = axis(2 * W, W)
    top = g[ya][:, xa] * (F(1.0) - fx) + g[ya][:, xb] * fx
    bot = g[yb][:, xa] * (F(1.0) - fx) + g[yb][:, xb] * fx
    return (top * (F(1.0) - fy)[:, None] + bot * fy[:, None]).astype(F)


def octave_count(H, W):
    return int(np.rint(np.log(float(2 * min(H, W))) / np.log(2.0) - 2.0)) + 1


def pyramid(gray, n_octave_layers=3, sigma=1.6):
    """[octave] -> float32 (n_octave_layers + 3, rows, cols)."""
    taps = [gaussian_taps(s) for s in blur_sigmas(n_octave_layers, sigma)]
    H, W = gray.shape
    octaves = []
    first = blur(base_image(gray), taps[0])
    for o in range(max(octave_count(H, W), 1)):
        if o:
            first = octaves[-1][n_octave_layers][::2, ::2][:octaves[-1].shape[1] // 2, :octaves[-1].shape[2] // 2]
            if first.size == 0:
                break
        layers = [np.ascontiguousarray(first)]
        for i in range(1, n_octave_layers + 3):
            layers.append(blur(layers[-1], taps[i]))
        octaves.append(np.stack(layers))
    return octaves


# ---- detection ----
def _solve3(a):
    """X of H X = b from the 3 x 4 float32 matrix by elimination with partial pivoting; None on a zero pivot."""
    a = [[F(v) for v in row] for row in a]
    for col in range(3):
        piv = col
        for rr in range(col + 1, 3):
            if abs(a[rr][col]) > abs(a[piv][col]):
                piv = rr
        if a[piv][col] == 0:
            return None
        a[col], a[piv] = a[piv], a[col]
        for rr in range(col + 1, 3):
            f = a[rr][col] / a[col][col]
            for k in range(col + 1, 4):
                a[rr][k] = a[rr][k] - f * a[col][k]
    x2 = a[2][3] / a[2][2]
    x1 = (a[1][3] - a[1][2] * x2) / a[1][1]
    x0 = (a[0][3] - a[0][1] * x1 - a[0][2] * x2) / a[0][0]
    return x0, x1, x2


def _tally(census, key, n=1):
    """census[key] += n when a census is kept (the optional ``census`` dicts below count which branches of the rules a picture reaches; the results do not change)."""
    if census is not None:
        census[key] = census.get(key, 0) + int(n)


CAND_DTYPE = np.dtype([("x", F), ("y", F), ("size", F), ("response", F), ("octave", np.int32), ("layer", np.int32), ("r", np.int32), ("c", np.int32)])


def candidates(pyr, mask=None, picture_shape=None, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10, sigma=1.6, census=None):
    """The refined candidates of every octave (a CAND_DTYPE array, in octave, layer, row, column order of their starting extremum).  ``census`` counts:
    ``extrema`` (starting extrema), ``moves_0`` .. ``moves_4`` (refinements that ended after so many moves), ``layer_moves`` (moves that changed the layer) and
    the ways out ``out_zero_pivot``, ``out_overrun``, ``out_left``, ``out_guard``, ``out_contrast``, ``out_edge``, ``out_mask``."""
    L = n_octave_layers
    ct, et, sg = F(contrast_threshold), F(edge_threshold), F(sigma)
    threshold = F(np.floor(0.5 * float(ct) / L * 255.0))
    s = F(1.0 / 255.0)
    ds, cs = s * F(0.5), s * F(0.25)
    out = []
    with np.errstate(all="ignore"):
        for o, g in enumerate(pyr):
            _, h, w = g.shape
            if h <= 2 * BORDER or w <= 2 * BORDER:
                continue
            dog = (g[1:] - g[:-1]).astype(F)
            for layer0 in range(1, L + 1):
                v = dog[layer0, BORDER:h - BORDER, BORDER:w - BORDER]
                is_max, is_min = v > 0, v < 0
                for dl in (-1, 0, 1):
                    for dr in (-1, 0, 1):
                        for dc in (-1, 0, 1):
                            nb = dog[layer0 + dl, BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                            is_max &= v >= nb
                            is_min &= v <= nb
                hit = (np.abs(v) > threshold) & (is_max | is_min)
                for r0, c0 in zip(*np.nonzero(hit)):
                    layer, r, c = layer0, int(r0) + BORDER, int(c0) + BORDER
                    Dv = lambda l, y, x: dog[l, y, x]
                    ok = False
                    _tally(census, "extrema")
                    for moves in range(STEPS):
                        v2 = Dv(layer, r, c) * F(2.0)
                        dxx = (Dv(layer, r, c + 1) + Dv(layer, r, c - 1) - v2) * s
                        dyy = (Dv(layer, r + 1, c) + Dv(layer, r - 1, c) - v2) * s
                        dss = (Dv(layer + 1, r, c) + Dv(layer - 1, r, c) - v2) * s
                        dxy = (Dv(layer, r + 1, c + 1) - Dv(layer, r + 1, c - 1) - Dv(layer, r - 1, c + 1) + Dv(layer, r - 1, c - 1)) * cs
                        dxs = (Dv(layer + 1, r, c + 1) - Dv(layer + 1, r, c - 1) - Dv(layer - 1, r, c + 1) + Dv(layer - 1, r, c - 1)) * cs
                        dys = (Dv(layer + 1, r + 1, c) - Dv(layer + 1, r - 1, c) - Dv(layer - 1, r + 1, c) + Dv(layer - 1, r - 1, c)) * cs
                        X = _solve3([[dxx, dxy, dxs, (Dv(layer, r, c + 1) - Dv(layer, r, c - 1)) * ds],
                                     [dxy, dyy, dys, (Dv(layer, r + 1, c) - Dv(layer, r - 1, c)) * ds],
                                     [dxs, dys, dss, (Dv(layer + 1, r, c) - Dv(layer - 1, r, c)) * ds]])
                        if X is None:
                            _tally(census, "out_zero_pivot")
                            break
                        xc, xr, xi = -X[0], -X[1], -X[2]
                        if abs(xi) < 0.5 and abs(xr) < 0.5 and abs(xc) < 0.5:
                            ok = True
                            _tally(census, f"moves_{moves}")
                            break
                        big = F(536870912.0)
                        if not (abs(xi) <= big and abs(xr) <= big and abs(xc) <= big):
                            _tally(census, "out_guard")
                            break
                        c, r, layer = c + int(np.rint(xc)), r + int(np.rint(xr)), layer + int(np.rint(xi))
                        _tally(census, "layer_moves", int(np.rint(xi)) != 0)
                        if layer < 1 or layer > L or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
                            _tally(census, "out_left")
                            break
                    else:
                        _tally(census, "out_overrun")
                    if not ok:
                        continue
                    d0 = (Dv(layer, r, c + 1) - Dv(layer, r, c - 1)) * ds
                    d1 = (Dv(layer, r + 1, c) - Dv(layer, r - 1, c)) * ds
                    d2 = (Dv(layer + 1, r, c) - Dv(layer - 1, r, c)) * ds
                    tdot = d0 * xc + d1 * xr + d2 * xi
                    contr = Dv(layer, r, c) * s + tdot * F(0.5)
                    if abs(contr) * F(L) < ct:
                        _tally(census, "out_contrast")
                        continue
                    v2 = Dv(layer, r, c) * F(2.0)
                    dxx = (Dv(layer, r, c + 1) + Dv(layer, r, c - 1) - v2) * s
                    dyy = (Dv(layer, r + 1, c) + Dv(layer, r - 1, c) - v2) * s
                    dxy = (Dv(layer, r + 1, c + 1) - Dv(layer, r + 1, c - 1) - Dv(layer, r - 1, c + 1) + Dv(layer, r - 1, c - 1)) * cs
                    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
                    if det <= 0 or tr * tr * et >= (et + F(1.0)) * (et + F(1.0)) * det:
                        _tally(census, "out_edge")
                        continue
                    scale = F(1 << o)
                    x, y = (F(c) + xc) * scale, (F(r) + xr) * scale
                    packed = o + (layer << 8) + (int(np.rint((xi + F(0.5)) * F(255.0))) << 16)
                    size = sg * sift_exp(((F(layer) + xi) / F(L)) * F(0.6931471805599453)) * scale * F(2.0)
                    if mask is not None:
                        H, W = picture_shape
                        mx = min(max(int(x * F(0.5) + F(0.5)), 0), W - 1)
                        my = min(max(int(y * F(0.5) + F(0.5)), 0), H - 1)
                        if mask[my, mx] == 0:
                            _tally(census, "out_mask")
                            continue
                    out.append((x, y, size, abs(contr), packed, layer, r, c))
    return np.array(out, dtype=CAND_DTYPE)


def retain_best(cand, nfeatures):
    if nfeatures <= 0 or len(cand) == 0:
        return cand
    resp = cand["response"]
    greater = (resp[None, :] > resp[:, None]).sum(axis=1)
    return cand[greater < nfeatures]


def _lane_sum(values, bins, n_bins, p):
    """values[k] added to bins[k] by lane p[k] % 64 in ascending p, then the lanes added in order to 0: float32 (n_bins,).  A sample may name several bins
    (2-D values / bins, the columns added in order); entries with bin < 0 take nothing."""
    part = np.zeros((64, n_bins), dtype=F)
    if values.ndim == 1:
        values, bins = values[:, None], bins[:, None]
    rounds = p // 64
    lanes = p % 64
    order = np.argsort(p, kind="stable")
    values, bins, rounds, lanes = values[order], bins[order], rounds[order], lanes[order]
    starts = np.flatnonzero(np.r_[True, rounds[1:] != rounds[:-1]])
    ends = np.r_[starts[1:], len(rounds)]
    for a, b in zip(starts, ends):  # within one round every lane holds at most one sample
        for q in range(values.shape[1]):
            sel = bins[a:b, q] >= 0
            la, bi = lanes[a:b][sel], bins[a:b, q][sel]
            part[la, bi] = part[la, bi] + values[a:b, q][sel]
    acc = np.zeros(n_bins, dtype=F)
    for lane in range(64):
        acc = acc + part[lane]
    return acc


def _window(radius):
    length = 2 * radius + 1
    p = np.arange(length * length)
    return p, p // length - radius, p % length - radius


def orientations(pyr, cand, n_octave_layers=3, census=None):
    """float32 (K, 6): the keypoints of every candidate, unsorted.  ``census`` counts ``ori_multi_peak`` (candidates with more than one peak), ``ori_window_cut``
    (candidates whose window loses samples to the layer's border) and ``ori_angle_folded`` (angles within FLT_EPSILON of 360 set to 0)."""
    out = []
    with np.errstate(all="ignore"):
        for k in cand:
            o, layer, r, c = int(k["octave"]) & 255, int(k["layer"]), int(k["r"]), int(k["c"])
            img = pyr[o][layer]
            h, w = img.shape
            scl = k["size"] * F(0.5) / F(1 << o)
            radius = int(np.rint(F(4.5) * scl))
            sigma = F(1.5) * scl
            exp_scale = F(-1.0) / (F(2.0) * sigma * sigma)
            p, i, j = _window(radius)
            y, x = r + i, c + j
            ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
            _tally(census, "ori_window_cut", not ok.all())
            p, i, j, y, x = p[ok], i[ok], j[ok], y[ok], x[ok]
            dx = img[y, x + 1] - img[y, x - 1]
            dy = img[y - 1, x] - img[y + 1, x]
            wgt = sift_exp((i * i + j * j).astype(F) * exp_scale)
            ori = sift_atan2_deg(dy, dx)
            mag = np.sqrt(dx * dx + dy * dy)
            b = np.rint(F(36.0 / 360.0) * ori).astype(np.int64)
            b = np.where(b >= ORI_BINS, b - ORI_BINS, b)
            b = np.where(b < 0, b + ORI_BINS, b)
            t = _lane_sum(wgt * mag, b, ORI_BINS, p)
            hist = (np.roll(t, 2) + np.roll(t, -2)) * F(1.0 / 16.0) + (np.roll(t, 1) + np.roll(t, -1)) * F(4.0 / 16.0) + t * F(6.0 / 16.0)
            thr = hist.max() * F(0.8)
            peaks = 0
            for jb in range(ORI_BINS):
                l, r2 = (jb - 1) % ORI_BINS, (jb + 1) % ORI_BINS
                if not (hist[jb] > hist[l] and hist[jb] > hist[r2] and hist[jb] >= thr):
                    continue
                b_ = F(jb) + F(0.5) * (hist[l] - hist[r2]) / (hist[l] - F(2.0) * hist[jb] + hist[r2])
                b_ = F(ORI_BINS) + b_ if b_ < 0 else b_ - F(ORI_BINS) if b_ >= ORI_BINS else b_
                angle = F(360.0) - F(360.0 / ORI_BINS) * b_
                if abs(angle - F(360.0)) < FLT_EPSILON:
                    angle = F(0.0)
                    _tally(census, "ori_angle_folded")
                peaks += 1
                packed = int(k["octave"])
                out.append((k["x"] * F(0.5), k["y"] * F(0.5), k["size"] * F(0.5), angle, k["response"], F((packed & ~255) | ((packed - 1) & 255))))
            _tally(census, "ori_multi_peak", peaks > 1)
    return np.array(out, dtype=F).reshape(-1, 6)


def sort_unique(kps):
    """Sorted by (x, y, size, angle, response, octave), exact duplicates removed."""
    if len(kps) == 0:
        return kps
    kps = kps[np.lexsort(kps.T[::-1])]
    keep = np.r_[True, (kps[1:] != kps[:-1]).any(axis=1)]
    return kps[keep]


def descriptors(pyr, kps, census=None):
    """uint8 (K, 128).  ``census`` counts ``desc_window_cut`` (keypoints whose window loses samples of its 4 x 4 cells to the layer's border),
    ``desc_radius_clamp`` (radius cut to the layer's diagonal), ``desc_clipped`` (values cut at 0.2 of the norm) and ``desc_saturated`` (bytes at 255)."""
    out = np.zeros((len(kps), D * D * NB), dtype=np.uint8)
    with np.errstate(all="ignore"):
        for n, kp in enumerate(kps):
            packed = int(kp[5])
            ob, layer = packed & 255, (packed >> 8) & 255
            octave = ob if ob < 128 else ob - 256
            img = pyr[octave + 1][layer]
            h, w = img.shape
            scale = np.ldexp(F(1.0), -octave).astype(F)
            px, py, scl = kp[0] * scale, kp[1] * scale, kp[2] * scale * F(0.5)
            ori = F(360.0) - kp[3]
            if abs(ori - F(360.0)) < FLT_EPSILON:
                ori = F(0.0)
            ptx, pty = int(np.rint(px)), int(np.rint(py))
            cos_t, sin_t = sift_sincos_deg(ori)
            bins_per_deg, exp_scale, hist_width = F(NB / 360.0), F(-1.0) / (F(D * D) * F(0.5)), F(3.0) * scl
            radius = int(np.rint(hist_width * F(1.4142135623730951) * F(D + 1) * F(0.5)))
            _tally(census, "desc_radius_clamp", radius > int(np.sqrt(float(h) * h + float(w) * w)))
            radius = min(radius, int(np.sqrt(float(h) * h + float(w) * w)))
            cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
            p, i, j = _window(radius)
            fi, fj = i.astype(F), j.astype(F)
            c_rot, r_rot = fj * cos_t - fi * sin_t, fj * sin_t + fi * cos_t
            rbin, cbin = r_rot + F(D // 2) - F(0.5), c_rot + F(D // 2) - F(0.5)
            r, c = pty + i, ptx + j
            cells = (rbin > -1) & (rbin < D) & (cbin > -1) & (cbin < D)
            ok = cells & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
            _tally(census, "desc_window_cut", (cells & ~ok).any())
            p, c_rot, r_rot, rbin, cbin, r, c = p[ok], c_rot[ok], r_rot[ok], rbin[ok], cbin[ok], r[ok], c[ok]
            dx = img[r, c + 1] - img[r, c - 1]
            dy = img[r - 1, c] - img[r + 1, c]
            wgt = sift_exp((c_rot * c_rot + r_rot * r_rot) * exp_scale)
            obin = (sift_atan2_deg(dy, dx) - ori) * bins_per_deg
            mag = np.sqrt(dx * dx + dy * dy) * wgt
            r0f, c0f, o0f = np.floor(rbin), np.floor(cbin), np.floor(obin)
            rbin, cbin, obin = rbin - r0f, cbin - c0f, obin - o0f
            r0, c0, o0 = r0f.astype(np.int64), c0f.astype(np.int64), o0f.astype(np.int64)
            o0 = np.where(o0 < 0, o0 + NB, o0)
            o0 = np.where(o0 >= NB, o0 - NB, o0)
            v_r1 = mag * rbin
            v_r0 = mag - v_r1
            v_rc11 = v_r1 * cbin
            v_rc10 = v_r1 - v_rc11
            v_rc01 = v_r0 * cbin
            v_rc00 = v_r0 - v_rc01
            v111 = v_rc11 * obin
            v110 = v_rc11 - v111
            v101 = v_rc10 * obin
            v100 = v_rc10 - v101
            v011 = v_rc01 * obin
            v010 = v_rc01 - v011
            v001 = v_rc00 * obin
            v000 = v_rc00 - v001
            o1 = (o0 + 1) & (NB - 1)
            values = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], axis=1).astype(F)
            bins = np.empty(values.shape, dtype=np.int64)
            for q in range(8):
                rr, cc, oo = r0 + (q >> 2), c0 + ((q >> 1) & 1), (o1 if q & 1 else o0)
                inside = (rr >= 0) & (rr < D) & (cc >= 0) & (cc < D)
                bins[:, q] = np.where(inside, (rr * D + cc) * NB + oo, -1)
            dst = _lane_sum(values, bins, D * D * NB, p)
            nrm2 = F(0.0)
            for v in dst:
                nrm2 = nrm2 + v * v
            thr = np.sqrt(nrm2) * F(0.2)
            _tally(census, "desc_clipped", (dst > thr).sum())
            dst = np.minimum(dst, thr)
            nrm2 = F(0.0)
            for v in dst:
                nrm2 = nrm2 + v * v
            s = F(512.0) / max(np.sqrt(nrm2), FLT_EPSILON)
            out[n] = np.clip(np.rint(dst * s), 0, 255).astype(np.uint8)
            _tally(census, "desc_saturated", (out[n] == 255).sum())
    return out


def detect_and_compute(gray, mask=None, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, stages=False, census=None):
    """(keypoints float32 (K, 6), descriptors uint8 (K, 128)); with ``stages`` a dict that also holds the pyramid, the candidates and the number of keypoints
    before the duplicates left (``raw``).  ``census``: a dict that receives the branch counts of ``candidates``, ``orientations`` and ``descriptors``."""
    gray = np.asarray(gray)
    assert gray.dtype == np.uint8 and gray.ndim == 2
    pyr = pyramid(gray, nOctaveLayers, sigma)
    cand = candidates(pyr, mask, gray.shape, nOctaveLayers, contrastThreshold, edgeThreshold, sigma, census)
    kept = retain_best(cand, nfeatures)
    raw = orientations(pyr, kept, nOctaveLayers, census)
    kps = sort_unique(raw)
    desc = descriptors(pyr, kps, census)
    if stages:
        return dict(pyramid=pyr, candidates=cand, keypoints=kps, descriptors=desc, raw=len(raw))
    return kps, desc


# ---- matcher and score ----
def knn(query, train):
    """(indices int32 (Q, 2), distances float32 (Q, 2)): the two nearest by exact integer squared distance, ties to the lower index; -1 / inf past the train set."""
    q, t = np.asarray(query, dtype=np.int64), np.asarray(train, dtype=np.int64)
    d2 = (q * q).sum(axis=1)[:, None] + (t * t).sum(axis=1)[None, :] - 2 * (q @ t.T)  # exact integers
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    idx = np.full((len(q), 2), -1, dtype=np.int32)
    dist = np.full((len(q), 2), np.inf, dtype=F)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.sqrt(np.take_along_axis(d2, order, axis=1).astype(F))
    return idx, dist


def mifd_from_features(kp1, desc1, kp2, desc2, ratio_threshold=0.7, k=2, min_matches=1, log_residual=False):
    """(score, survivors) of compare_image_pair.py:63-97 from two pictures' keypoints and descriptors."""
    if k != 2:
        raise ValueError("k = 2 only")
    if len(desc1) == 0 or len(desc2) == 0:
        warnings.warn("Could not extract any features for at least one image in the pair.")
        return NAN, 0
    if len(desc1) < k or len(desc2) < k:
        warnings.warn(f"Not enough descriptors for k={k:d}, only got {len(desc1):,d} and {len(desc2):,d}.")
        return NAN, 0
    idx, dist = knn(desc1, desc2)
    keep = dist[:, 0] < F(ratio_threshold) * dist[:, 1]
    kept = int(keep.sum())
    if kept < min_matches or kept == 0:
        warnings.warn(f"Not enough matches for `min_matches={min_matches}`, only got {kept}.")
        return NAN, kept
    p1, p2 = kp1[keep][:, :2].astype(F), kp2[idx[keep, 0]][:, :2].astype(F)
    with np.errstate(all="ignore"):
        res = (np.log10(p1) - np.log10(p2) if log_residual else p1 - p2).astype(np.float64)
    total = 0.0
    for dx, dy in res:
        total = total + np.sqrt(dx * dx + dy * dy)
    return float(total / kept), kept


def mifd(label, output, ratio_threshold=0.7, k=2, min_matches=1, log_residual=False, mask=None, with_matches=False, **sift):
    """``mifd`` of compare_image_pair.py:44-97 on two gray uint8 pictures."""
    kp1, d1 = detect_and_compute(label, mask, **sift)
    kp2, d2 = detect_and_compute(output, mask, **sift)
    score, kept = mifd_from_features(kp1, d1, kp2, d2, ratio_threshold, k, min_matches, log_residual)
    return (score, kept) if with_matches else score
