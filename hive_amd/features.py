"""SIFT keypoints and descriptors, the exact 2-nearest-neighbour matcher and MIFD on the MI355X (csrc/sift.hip): ``mifd`` of the reference's
scripts/compare_image_pair.py:44-97, and the detector / matcher that hive/pose_optimisation.py:294, :426, :452 call through cv2.

The rules are stated in include/hive_mi355x.h above ``hive_sift_create`` and restated in numpy float32 in tests/sift_restatement.py.  They are Lowe's SIFT with
cv2.SIFT.create()'s parameters as recalled from OpenCV 4.x; cv2 cannot be run beside this code, so keypoints and descriptors are not pinned against cv2.  The
reference matches with FLANN (an approximate randomised KD-tree search); the matcher here returns the exact nearest neighbours and is not pinned against FLANN.

``match_pairs``, ``ransac_homography`` / ``find_homography`` and ``compact_pairs`` (csrc/pairs.hip) are the stages of the reference's ``FeatureExtractor`` behind the
detector (hive/pose_optimisation.py:437-578); the homography RANSAC is a stated rule of its own, not pinned against cv2's randomised USAC_MAGSAC.
``ransac_rigid`` / ``estimate_rigid_transform`` (csrc/register.hip) fit a rigid or similarity transform to the same rows back-projected with their depth: the
start of ``hive_amd.registration``, where the reference calls COLMAP or BundleFusion (absent; not pinned against either)."""
import ctypes
import warnings

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr
from hive_amd._pictures import device_of, is_torch, on_device

NAN = float("nan")
SIFT_MIN_SIDE = 6  # the doubled picture must reach past the 5-pixel border on both sides
KEYPOINT_FIELDS = ("x", "y", "size", "angle", "response", "octave")


def blur_sigmas(n_octave_layers=3, sigma=1.6):
    """[0] the blur of the doubled base picture, [i] the blur from layer i - 1 to layer i of an octave (float64)."""
    sig = [np.sqrt(max(sigma * sigma - 4 * 0.5 * 0.5, 0.01))]
    k = 2.0 ** (1.0 / n_octave_layers)
    for i in range(1, n_octave_layers + 3):
        prev = sigma * k ** (i - 1)
        total = prev * k
        sig.append(np.sqrt(total * total - prev * prev))
    return sig


def gaussian_taps(sig):
    """round(8 sig + 1) | 1 taps: exp(-(i - R)^2 / (2 sig^2)) in float64 over their sum, rounded to float32."""
    n = int(np.rint(8 * sig + 1)) | 1
    g = np.exp(-(np.arange(n, dtype=np.float64) - n // 2) ** 2 / (2 * sig * sig))
    return np.ascontiguousarray((g / g.sum()).astype(np.float32))


def octave_sizes(h, w):
    """[(rows, cols)] of the octaves of an h x w picture (octave 0 is the doubled picture)."""
    count = int(np.rint(np.log(float(2 * min(h, w))) / np.log(2.0) - 2.0)) + 1
    sizes, rows, cols = [], 2 * h, 2 * w
    for _ in range(max(count, 1)):
        if rows < 1 or cols < 1:
            break
        sizes.append((rows, cols))
        rows, cols = rows // 2, cols // 2
    return sizes


class SIFT:
    """``cv2.SIFT.create(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma)`` on the GPU.  ``capacity``: the most refined candidates and the most
    keypoints one picture may have; a picture with more fails the call with an error that names the count (it is never cut).  One object serves any picture
    size and batch: a native detector per (context, H, W) is made on first use and holds at most ``workspace_bytes`` of pyramids (larger batches run in chunks)."""

    def __init__(self, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, capacity=4096, ctx=None, workspace_bytes=4 << 30):
        if not 1 <= int(nOctaveLayers) <= 5:
            raise ValueError(f"nOctaveLayers: 1 .. 5, got {nOctaveLayers}")
        if not 1 <= int(capacity) <= 65535:
            raise ValueError(f"capacity: 1 .. 65535, got {capacity}")
        if nfeatures < 0 or contrastThreshold < 0 or edgeThreshold <= 0 or sigma <= 0:
            raise ValueError("nfeatures and contrastThreshold must not be negative, edgeThreshold and sigma must be positive")
        self.nfeatures, self.nOctaveLayers, self.capacity = int(nfeatures), int(nOctaveLayers), int(capacity)
        self.contrastThreshold, self.edgeThreshold, self.sigma = float(contrastThreshold), float(edgeThreshold), float(sigma)
        self.ctx, self.workspace_bytes = ctx, int(workspace_bytes)
        self.taps = [gaussian_taps(s) for s in blur_sigmas(self.nOctaveLayers, self.sigma)]
        if max(len(t) for t in self.taps) > 33:
            raise ValueError(f"sigma = {sigma} with {nOctaveLayers} layers needs a blur of {max(len(t) for t in self.taps)} taps; the kernel holds 33")
        self._native = {}  # (id(ctx), H, W) -> [ctx, handle, max_images]
        self._last = None  # (ctx, handle, pictures) of the most recent launch, for the stage readers

    # ---- the native detector ----
    def _chunk(self, h, w, n):
        # float32: the doubled base, nOctaveLayers + 3 layers of octaves that sum to at most 4 / 3 of it, 20 words a candidate / keypoint slot
        per_image = 4 * (4 * h * w) * (1 + -(-(self.nOctaveLayers + 3) * 4 // 3)) + self.capacity * 20 * 4
        return int(max(1, min(n, self.workspace_bytes // per_image, 8192)))

    def _handle(self, ctx, h, w, images):
        key = (id(ctx), h, w)
        entry = self._native.get(key)
        if entry is not None and entry[2] < images:
            ctx.check(ctx.lib.hive_sift_destroy(entry[1]))
            entry = None
        if entry is None:
            count = len(self.taps)
            taps = (ctypes.c_void_p * count)(*(t.ctypes.data for t in self.taps))
            counts = (ctypes.c_int * count)(*(len(t) for t in self.taps))
            handle = ctypes.c_void_p()
            ctx.check(ctx.lib.hive_sift_create(ctx.handle, h, w, images, self.nfeatures, self.nOctaveLayers, self.contrastThreshold, self.edgeThreshold, self.sigma,
                                               taps, counts, self.capacity, ctypes.byref(handle)))
            entry = self._native[key] = [ctx, handle, images]
        return entry[1]

    def close(self):
        for ctx, handle, _ in self._native.values():
            if _lib.alive() and getattr(ctx, "handle", None):
                ctx.lib.hive_sift_destroy(handle)
        self._native, self._last = {}, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _context(self, dev):
        return _lib.context_for(self.ctx, dev)

    def detect_device(self, gray, mask=None, ctx=None, out=None, first=0):
        """The launches alone, nothing synchronises: ``gray`` (and ``mask``) contiguous uint8 device tensors (N, H, W) -> device tensors ``(keypoints float32
        (N, capacity, 6), descriptors uint8 (N, capacity, 128), counts int32 (N, 3))``; rows past a picture's count are undefined.  ``out``: such a triple of a
        larger batch, filled from picture ``first`` on.  Hand the counts to ``check_counts`` once they are on the host."""
        import torch
        n, h, w = (int(v) for v in gray.shape)
        if min(h, w) < SIFT_MIN_SIDE:
            raise ValueError(f"{h} x {w} is smaller than {SIFT_MIN_SIDE} x {SIFT_MIN_SIDE}, the smallest picture SIFT can handle")
        ctx = ctx or self._context(gray.device)
        if out is None:
            out = (torch.empty((n, self.capacity, 6), dtype=torch.float32, device=gray.device),
                   torch.empty((n, self.capacity, 128), dtype=torch.uint8, device=gray.device), torch.empty((n, 3), dtype=torch.int32, device=gray.device))
        kps, desc, counts = out
        chunk = self._chunk(h, w, n)
        handle = self._handle(ctx, h, w, chunk)
        for at in range(0, n, chunk):
            m = min(chunk, n - at)
            ctx.check(ctx.lib.hive_sift_detect(handle, ptr(gray[at:at + m]), ptr(mask[at:at + m]) if mask is not None else None, m, ptr(kps[first + at:]),
                                               ptr(desc[first + at:]), ptr(counts[first + at:])))
            self._last = (ctx, handle, m, h, w, gray.device)
        return out

    def check_counts(self, counts):
        """``counts``: host (N, 3).  Raises when a picture had more candidates or keypoints than the capacity."""
        counts = np.asarray(counts)
        for i, (cand, raw, _) in enumerate(counts):
            if max(cand, raw) > self.capacity:
                what, count = ("refined candidates", cand) if cand > self.capacity else ("keypoints", raw)
                raise _lib.HiveError(_lib.ERR_INVALID, f"SIFT: picture {i} has {int(count)} {what}, more than the capacity {self.capacity}; make the SIFT with a larger capacity")

    def _pictures(self, gray, mask):
        batched = len(gray.shape) == 3
        if len(gray.shape) not in (2, 3):
            raise ValueError(f"gray pictures are (H, W) or (N, H, W), got {tuple(gray.shape)}")
        dev = device_of(gray, mask)
        device = lambda a, name: on_device(a, dev, check=lambda dtype, _: dtype == "uint8", error=lambda a: f"{name}: uint8, got {a.dtype}",
                                           shape=(-1,) + tuple(gray.shape[-2:]))
        g = device(gray, "gray")
        m = None
        if mask is not None:
            if tuple(mask.shape) != tuple(gray.shape):
                raise ValueError(f"mask: shape {tuple(mask.shape)}, the pictures have {tuple(gray.shape)}")
            m = device(mask, "mask")
        return g, m, batched

    def detect_and_compute(self, gray, mask=None):
        """``gray``: one uint8 (H, W) picture or a batch (N, H, W), a numpy array or a device tensor; ``mask`` likewise (a keypoint whose rounded position has
        mask 0 is dropped).  Returns ``(keypoints, descriptors)``, float32 (K, 6) in the order of ``KEYPOINT_FIELDS`` and uint8 (K, 128), numpy arrays; for a batch
        a list of such pairs.  The float32 view of the descriptor bytes is what cv2 returns."""
        g, m, batched = self._pictures(gray, mask)
        kps, desc, counts = self.detect_device(g, m)
        counts_h = counts.cpu().numpy()
        self.check_counts(counts_h)
        kps_h, desc_h = kps.cpu().numpy(), desc.cpu().numpy()
        out = [(kps_h[i, :k].copy(), desc_h[i, :k].copy()) for i, k in enumerate(counts_h[:, 2])]
        return out if batched else out[0]

    # ---- stages of the most recent launch (tests) ----
    def read_layer(self, octave, layer):
        """Gaussian layer ``layer`` of octave ``octave`` of the pictures of the most recent launch: a float32 device tensor (N, rows, cols)."""
        import torch
        ctx, handle, n, h, w, dev = self._last
        rows, cols = octave_sizes(h, w)[octave]
        out = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
        ctx.check(ctx.lib.hive_sift_read_layer(handle, octave, layer, n, ptr(out)))
        return out

    def read_candidates(self):
        """The refined candidates of the most recent launch in append order: a device tensor (N, capacity, 8) of 32-bit words (int32 view; the first four are
        float32 bits): x, y, size, response, packed octave, layer, r, c."""
        import torch
        ctx, handle, n, _, _, dev = self._last
        out = torch.empty((n, self.capacity, 8), dtype=torch.int32, device=dev)
        ctx.check(ctx.lib.hive_sift_read_candidates(handle, n, ptr(out)))
        return out


def knn_match(query, train, ctx=None):
    """The two nearest ``train`` descriptors of every ``query`` descriptor (uint8 (Q, 128) and (T, 128), numpy arrays or device tensors) by exact squared L2
    distance, ties to the lower train index: ``(indices int32 (Q, 2), distances float32 (Q, 2))``, of the kind ``query`` is.  With fewer than two train descriptors
    the missing entries are -1 and inf.  This is the exact answer: not pinned against the reference's approximate FLANN search."""
    import torch
    as_numpy = not is_torch(query)
    dev = device_of(query, train)
    device = lambda a, name: on_device(a, dev, check=lambda dtype, shape: dtype == "uint8" and len(shape) == 2 and shape[1] == 128,
                                       error=lambda a: f"{name}: uint8 (K, 128) descriptors, got {a.dtype} {tuple(a.shape)}")
    q, t = device(query, "query"), device(train, "train")
    nq, nt = int(q.shape[0]), int(t.shape[0])
    idx = torch.full((nq, 2), -1, dtype=torch.int32, device=dev)
    dist = torch.full((nq, 2), float("inf"), dtype=torch.float32, device=dev)
    if nq and nt:
        ctx = _lib.context_for(ctx, dev)
        ctx.check(ctx.lib.hive_knn_match(ctx.handle, ptr(q), nq, ptr(t), nt, ptr(idx), ptr(dist)))
    return (idx.cpu().numpy(), dist.cpu().numpy()) if as_numpy else (idx, dist)


def warn_no_score(n_query, n_train, matches, k=2, min_matches=1):
    """The reference's warnings (compare_image_pair.py:63-87) for a pair without a score; True when one was given."""
    if n_query == 0 or n_train == 0:
        warnings.warn("Could not extract any features for at least one image in the pair.")
    elif n_query < k or n_train < k:
        warnings.warn(f"Not enough descriptors for k={k:d}, only got {n_query:,d} and {n_train:,d}.")
    elif matches < min_matches or matches == 0:
        warnings.warn(f"Not enough matches for `min_matches={min_matches}`, only got {matches}.")
    else:
        return False
    return True


def score_pairs(sift, features, query_first, train_first, pairs, ctx, ratio_threshold=0.7, min_matches=1):
    """MIFD of ``pairs`` pairs of pictures of one ``SIFT.detect_device`` result, picture ``query_first + p`` against ``train_first + p``: device tensors
    ``(scores float64 (pairs,), matches int32 (pairs,), indices int32 (pairs, capacity, 2), distances float32 (pairs, capacity, 2))``.  Nothing synchronises."""
    import torch
    kps, desc, counts = features
    dev, cap = kps.device, sift.capacity
    scores = torch.empty(pairs, dtype=torch.float64, device=dev)
    matches = torch.empty(pairs, dtype=torch.int32, device=dev)
    idx = torch.empty((pairs, cap, 2), dtype=torch.int32, device=dev)
    dist = torch.empty((pairs, cap, 2), dtype=torch.float32, device=dev)
    ctx.check(ctx.lib.hive_mifd(ctx.handle, ptr(kps), ptr(desc), ptr(counts), cap, query_first, train_first, pairs, float(ratio_threshold), int(min_matches), ptr(idx),
                                ptr(dist), ptr(scores), ptr(matches)))
    return scores, matches, idx, dist


def mifd(label, output, ratio_threshold=0.7, k=2, min_matches=1, log_residual=False, sift=None, return_matches=False):
    """``mifd`` of compare_image_pair.py:44-97 on two gray uint8 pictures (numpy arrays or device tensors): SIFT on both, the two nearest ``output`` descriptors
    of every ``label`` descriptor, Lowe's ratio test, the mean distance between the matched positions; nan, with the reference's warnings, with fewer than ``k``
    descriptors on a side or fewer than ``min_matches`` matches.  ``k`` must be 2 (ValueError otherwise).  ``sift``: a ``SIFT`` to use (default parameters
    otherwise).  ``log_residual``: the distances are taken between the float32 log10 of the positions; that variant is finished on the host from the device's
    matches.  ``return_matches``: ``(score, matches)``."""
    import torch
    if k != 2:
        raise ValueError(f"mifd: k = 2 only (the ratio test needs exactly the two nearest), got {k}")
    own = sift is None
    sift = sift or SIFT()
    try:
        a, _, _ = sift._pictures(label, None)
        b, _, _ = sift._pictures(output, None)
        if a.shape[0] != 1 or b.shape[0] != 1:
            raise ValueError("mifd: one (H, W) picture on each side")
        dev, cap = a.device, sift.capacity
        ctx = sift._context(dev)
        if min(a.shape[1:]) < SIFT_MIN_SIDE or min(b.shape[1:]) < SIFT_MIN_SIDE:
            warnings.warn("Could not extract any features for at least one image in the pair.")
            return (NAN, 0) if return_matches else NAN
        features = (torch.empty((2, cap, 6), dtype=torch.float32, device=dev), torch.empty((2, cap, 128), dtype=torch.uint8, device=dev),
                    torch.empty((2, 3), dtype=torch.int32, device=dev))
        if a.shape == b.shape:
            sift.detect_device(torch.cat([a, b]), None, ctx, out=features)
        else:
            sift.detect_device(a, None, ctx, out=features, first=0)
            sift.detect_device(b, None, ctx, out=features, first=1)
        scores, matches, idx, dist = score_pairs(sift, features, 0, 1, 1, ctx, ratio_threshold, min_matches)
        counts = features[2].cpu().numpy()
        sift.check_counts(counts)
        nq, nt = int(counts[0, 2]), int(counts[1, 2])
        kept = int(matches.cpu().numpy()[0]) if nq >= k and nt >= k else 0
        if warn_no_score(nq, nt, kept, k, min_matches):
            score = NAN
        elif log_residual:
            kps = features[0].cpu().numpy()
            idx_h, dist_h = idx[0, :nq].cpu().numpy(), dist[0, :nq].cpu().numpy()
            keep = dist_h[:, 0] < np.float32(ratio_threshold) * dist_h[:, 1]
            with np.errstate(all="ignore"):
                res = (np.log10(kps[0, :nq][keep][:, :2]) - np.log10(kps[1][idx_h[keep, 0]][:, :2])).astype(np.float64)
            total = 0.0
            for dx, dy in res:
                total = total + np.sqrt(dx * dx + dy * dy)
            score = float(total / kept)
        else:
            score = float(scores.cpu().numpy()[0])
        return (score, kept) if return_matches else score
    finally:
        if own:
            sift.close()


# ---- feature pairs for pose optimisation: the pair matcher, its filter and the homography RANSAC (csrc/pairs.hip) ----
ROW_WORDS = 8  # a survivor: x_i, y_i, x_j, y_j, depth_i, depth_j (float32), query index, train index (int32 bits)


def match_pairs(features, pairs, depth, ratio=0.7, min_features=2, return_table=False, ctx=None):
    """The stage before the RANSAC of the reference's ``FeatureExtractor`` (hive/pose_optimisation.py:449-455, :518-539) for a list of picture pairs of one
    ``SIFT.detect_device`` result: the exact two nearest ``pairs[p][1]`` descriptors of every ``pairs[p][0]`` descriptor, then the filter -- both pictures have
    ``max(min_features, 2)`` keypoints, ``not float(d0) > ratio * float(d1)`` in float64, and the depth at both rounded keypoint positions is not 0 -- with the
    survivors kept in query order.  ``features``: the device triple; ``pairs``: (P, 2) picture indices, a list, an array or an int32 device tensor; ``depth``:
    float32 device tensor (N, H, W).  Returns device tensors ``(rows float32 (P, capacity, 8), counts int32 (P, 2))``: a row is x_i, y_i, x_j, y_j, depth_i,
    depth_j and, as int32 bits, the query and the train index; ``counts[p]`` the ratio survivors and the survivors (rows past them are undefined).  With
    ``return_table`` also ``(indices int32, distances float32)`` (P, capacity, 2), the raw 2-NN table.  Nothing synchronises.  The matcher is the exact answer:
    not pinned against the reference's approximate FLANN search."""
    import torch
    kps, desc, counts = features
    dev, cap, n = kps.device, int(kps.shape[1]), int(kps.shape[0])
    if not is_torch(pairs):
        host = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        if len(host) and (host.min() < 0 or host.max() >= n):
            raise ValueError(f"pairs name pictures {int(host.min())} .. {int(host.max())}; the features hold {n}")
        pairs = torch.from_numpy(host.astype(np.int32)).to(dev)
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"pairs: int32 (P, 2), got {pairs.dtype} {tuple(pairs.shape)}")
    if depth.dtype != torch.float32 or depth.dim() != 3 or int(depth.shape[0]) != n:
        raise ValueError(f"depth: float32 (N, H, W) with N = {n}, got {depth.dtype} {tuple(depth.shape)}")
    pairs, depth, p = pairs.contiguous(), depth.contiguous(), int(pairs.shape[0])
    rows = torch.empty((p, cap, ROW_WORDS), dtype=torch.float32, device=dev)
    pair_counts = torch.zeros((p, 2), dtype=torch.int32, device=dev)
    idx = torch.empty((p, cap, 2), dtype=torch.int32, device=dev) if return_table else None
    dist = torch.empty((p, cap, 2), dtype=torch.float32, device=dev) if return_table else None
    if p:
        ctx = _lib.context_for(ctx, dev)
        ctx.check(ctx.lib.hive_pairs_match(ctx.handle, ptr(kps), ptr(desc), ptr(counts), cap, n, ptr(pairs), p, ptr(depth), int(depth.shape[1]), int(depth.shape[2]),
                                           float(ratio), int(min_features), ptr(rows), ptr(pair_counts), ptr(idx), ptr(dist)))
    return (rows, pair_counts, idx, dist) if return_table else (rows, pair_counts)


def ransac_homography(rows, counts, keys, threshold=3.0, trials=2000, seed=0, min_count=0, ctx=None):
    """The homography RANSAC of include/hive_mi355x.h (rules ``normalise`` .. ``H``) for P pairs at once.  ``rows``: float32 device tensor (P, stride, W >= 4)
    whose first four words are x_i, y_i, x_j, y_j (``match_pairs``'s rows, or plain (P, stride, 4) points); ``counts``: int32 device tensor (P,), or a column
    such as ``match_pairs``'s ``counts[:, 1]``; ``keys``: (P, 2) the frame pairs that seed the draws.  Returns device tensors ``(H float64 (P, 3, 3), mask uint8
    (P, stride), result int32 (P, 3))``: per pair the winning trial (-1 without a model, -2 for a count outside 0 .. stride), the winner's count and the final
    count; a pair with fewer than ``max(min_count, 4)`` correspondences has no model.  A function of its inputs alone: all ``trials`` trials run.  It stands where the reference calls ``cv2.findHomography(..., cv2.USAC_MAGSAC)``
    (:562) and is not pinned against cv2.  Nothing synchronises."""
    import torch
    if rows.dtype != torch.float32 or rows.dim() != 3 or int(rows.shape[2]) < 4 or not rows.is_contiguous():
        raise ValueError(f"rows: contiguous float32 (P, stride, >= 4), got {rows.dtype} {tuple(rows.shape)}")
    dev, p, stride, words = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(rows.shape[2])
    if counts.dtype != torch.int32 or counts.dim() != 1 or int(counts.shape[0]) != p:
        raise ValueError(f"counts: int32 (P,) with P = {p}, got {counts.dtype} {tuple(counts.shape)}")
    if not is_torch(keys):
        keys = torch.from_numpy(np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1, 2).astype(np.int32))).to(dev)
    if keys.dtype != torch.int32 or tuple(keys.shape) != (p, 2):
        raise ValueError(f"keys: int32 (P, 2) with P = {p}, got {keys.dtype} {tuple(keys.shape)}")
    keys = keys.contiguous()
    H = torch.empty((p, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((p, max(stride, 1)), dtype=torch.uint8, device=dev)[:, :stride]
    result = torch.empty((p, 3), dtype=torch.int32, device=dev)
    if p and stride:
        ctx = _lib.context_for(ctx, dev)
        ctx.check(ctx.lib.hive_ransac_homography(ctx.handle, ptr(rows), words, ptr(counts), int(counts.stride(0)), ptr(keys), p, stride, float(threshold), int(trials),
                                                 int(seed) & 0xFFFFFFFF, int(min_count), ptr(H), ptr(mask), ptr(result)))
    elif p:
        H.fill_(NAN)
        result.copy_(torch.tensor([-1, 0, 0], dtype=torch.int32, device=dev))
    return H, mask, result


def find_homography(points_i, points_j, threshold=3.0, trials=2000, seed=0, pair_key=(0, 0), return_stats=False, ctx=None):
    """The part of ``cv2.findHomography(points_i, points_j, cv2.USAC_MAGSAC)`` (hive/pose_optimisation.py:562) for one pair: (M, 2) points, numpy arrays or
    device tensors -> ``(H, mask)``, H float64 (3, 3) with h33 = 1 mapping ``points_i`` onto ``points_j`` (None without a model: fewer than four points, all
    points of a side equal, or every sample degenerate) and the inlier mask uint8 (M,), of the kind ``points_i`` is.  ``threshold`` in pixels of ``points_j`` and
    ``trials`` are cv2's defaults (ransacReprojThreshold 3, maxIters 2000, from recall).  The draws depend on ``seed`` and ``pair_key`` alone, so the result is a
    function of the arguments.  ``return_stats``: also ``(winning trial, the winner's count, the final count)``.  Not pinned against cv2: USAC_MAGSAC is randomised."""
    import torch
    as_numpy = not is_torch(points_i)
    dev = device_of(points_i, points_j)
    device = lambda a, name: on_device(a if is_torch(a) else np.asarray(a, dtype=np.float32).reshape(-1, 2), dev, dtype=torch.float32,
                                       check=lambda _, shape: len(shape) == 2 and shape[1] == 2, error=lambda a: f"{name}: (M, 2) points, got {tuple(a.shape)}")
    a, b = device(points_i, "points_i"), device(points_j, "points_j")
    if a.shape != b.shape:
        raise ValueError(f"points_i {tuple(a.shape)} and points_j {tuple(b.shape)} differ")
    m = int(a.shape[0])
    rows = torch.cat([a, b], dim=1).reshape(1, m, 4).contiguous()
    H, mask, result = ransac_homography(rows, torch.tensor([m], dtype=torch.int32, device=dev), [pair_key], threshold, trials, seed, ctx=ctx)
    stats = tuple(int(v) for v in result[0].cpu().numpy())
    found = stats[0] >= 0
    if as_numpy:
        out = (H[0].cpu().numpy() if found else None, mask[0].cpu().numpy())
    else:
        out = (H[0] if found else None, mask[0])
    return out + (stats,) if return_stats else out


def ransac_rigid(rows, counts, keys, camera_matrix=None, threshold=0.05, trials=2000, seed=0, min_count=0, with_scale=False, ctx=None):
    """The rigid (``with_scale``: similarity) RANSAC of include/hive_mi355x.h (rules ``points`` .. ``outputs`` above ``hive_ransac_rigid``; csrc/register.hip) for
    P pairs at once.  ``rows``: float32 device tensor (P, stride, W >= 6).  With ``camera_matrix`` (3 x 3, fx, fy, cx, cy are read) a row is ``match_pairs``'s
    x_i, y_i, x_j, y_j, depth_i, depth_j and both sides are back-projected; with ``camera_matrix=None`` a row is X_i Y_i Z_i X_j Y_j Z_j.  ``counts``: int32
    device tensor (P,), or a column such as ``match_pairs``'s ``counts[:, 1]``; ``keys``: (P, 2) the frame pairs that seed the draws.  Returns device tensors
    ``(T float64 (P, 4, 4), scale float64 (P,), rms float64 (P,), mask uint8 (P, stride), result int32 (P, 3))``: T maps camera-i points onto camera-j points
    and holds scale * R and t; rms is over the final inliers; per pair the winning trial (-1 without a model, -2 for a count outside 0 .. stride), the winner's
    count and the final count.  A pair with fewer than ``max(min_count, 3)`` correspondences has no model: T, scale and rms are NaN and the mask is 0.
    ``threshold`` is in the depth's unit; its default 0.05 is a parameter default (5 cm for depth in metres), not a measured quantity.  A function of its inputs
    alone: all ``trials`` trials run.  Not pinned against cv2's estimateAffine3D, Open3D, BundleFusion or COLMAP (all absent).  Nothing synchronises."""
    import torch
    if rows.dtype != torch.float32 or rows.dim() != 3 or int(rows.shape[2]) < 6 or not rows.is_contiguous():
        raise ValueError(f"rows: contiguous float32 (P, stride, >= 6), got {rows.dtype} {tuple(rows.shape)}")
    dev, p, stride, words = rows.device, int(rows.shape[0]), int(rows.shape[1]), int(rows.shape[2])
    if counts.dtype != torch.int32 or counts.dim() != 1 or int(counts.shape[0]) != p:
        raise ValueError(f"counts: int32 (P,) with P = {p}, got {counts.dtype} {tuple(counts.shape)}")
    if not is_torch(keys):
        keys = torch.from_numpy(np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1, 2).astype(np.int32))).to(dev)
    if keys.dtype != torch.int32 or tuple(keys.shape) != (p, 2):
        raise ValueError(f"keys: int32 (P, 2) with P = {p}, got {keys.dtype} {tuple(keys.shape)}")
    keys = keys.contiguous()
    camera = None
    if camera_matrix is not None:
        K = np.asarray(camera_matrix.detach().cpu().numpy() if is_torch(camera_matrix) else camera_matrix, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError(f"camera_matrix: (3, 3), got {K.shape}")
        camera = (ctypes.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    T = torch.empty((p, 4, 4), dtype=torch.float64, device=dev)
    scale = torch.empty(p, dtype=torch.float64, device=dev)
    rms = torch.empty(p, dtype=torch.float64, device=dev)
    mask = torch.empty((p, max(stride, 1)), dtype=torch.uint8, device=dev)[:, :stride]
    result = torch.empty((p, 3), dtype=torch.int32, device=dev)
    if p and stride:
        ctx = _lib.context_for(ctx, dev)
        ctx.check(ctx.lib.hive_ransac_rigid(ctx.handle, ptr(rows), words, ptr(counts), int(counts.stride(0)), ptr(keys), p, stride, camera, float(threshold), int(trials),
                                            int(seed) & 0xFFFFFFFF, int(min_count), int(bool(with_scale)), ptr(T), ptr(scale), ptr(rms), ptr(mask), ptr(result)))
    elif p:
        T.fill_(NAN), scale.fill_(NAN), rms.fill_(NAN)
        result.copy_(torch.tensor([-1, 0, 0], dtype=torch.int32, device=dev))
    return T, scale, rms, mask, result


def estimate_rigid_transform(points_i, points_j, threshold=0.05, trials=2000, seed=0, pair_key=(0, 0), with_scale=False, return_stats=False, ctx=None):
    """``ransac_rigid`` for one pair of (M, 3) point sets, numpy arrays or device tensors -> ``(T, mask)``: T float64 (4, 4) mapping ``points_i`` onto
    ``points_j`` (scale * R and t; None without a model: fewer than three points, or every sample degenerate) and the inlier mask uint8 (M,), of the kind
    ``points_i`` is.  ``threshold`` is in the points' unit; 0.05 is a parameter default (5 cm for metres), not a measured quantity.  The draws depend on ``seed``
    and ``pair_key`` alone, so the result is a function of the arguments.  ``return_stats``: also ``(winning trial, the winner's count, the final count, scale,
    rms)``.  Not pinned against cv2's estimateAffine3D or Open3D (absent)."""
    import torch
    as_numpy = not is_torch(points_i)
    dev = device_of(points_i, points_j)
    host = lambda a: a if a.ndim == 2 else a.reshape(-1, 3)  # an empty list is (0, 3)
    device = lambda a, name: on_device(a if is_torch(a) else host(np.asarray(a, dtype=np.float32)), dev, dtype=torch.float32,
                                       check=lambda _, shape: len(shape) == 2 and shape[1] == 3, error=lambda a: f"{name}: (M, 3) points, got {tuple(a.shape)}")
    a, b = device(points_i, "points_i"), device(points_j, "points_j")
    if a.shape != b.shape:
        raise ValueError(f"points_i {tuple(a.shape)} and points_j {tuple(b.shape)} differ")
    m = int(a.shape[0])
    rows = torch.cat([a, b], dim=1).reshape(1, m, 6).contiguous()
    T, scale, rms, mask, result = ransac_rigid(rows, torch.tensor([m], dtype=torch.int32, device=dev), [pair_key], None, threshold, trials, seed, 0, with_scale, ctx=ctx)
    host = torch.cat([result[0].double(), scale, rms]).cpu().numpy()  # the one synchronisation
    stats = (int(host[0]), int(host[1]), int(host[2]), float(host[3]), float(host[4]))
    found = stats[0] >= 0
    if as_numpy:
        out = (T[0].cpu().numpy() if found else None, mask[0].cpu().numpy())
    else:
        out = (T[0] if found else None, mask[0])
    return out + (stats,) if return_stats else out


def compact_pairs(rows, counts, mask, result, min_features, ctx=None):
    """The second compaction (:465-468): the inlier rows of every pair with ``min_features`` survivors and ``min_features`` inliers, pair after pair, inliers in
    row order.  Device tensors ``(out float32 (P * stride, 8), kept int32 (P,), offsets int64 (P + 1,))``: ``out[offsets[p]:offsets[p + 1]]`` are pair p's rows,
    ``kept[p]`` their number (0: the pair is dropped), ``offsets[P]`` all rows.  Nothing synchronises."""
    import torch
    dev, p, stride = rows.device, int(rows.shape[0]), int(rows.shape[1])
    out = torch.empty((p * stride, ROW_WORDS), dtype=torch.float32, device=dev)
    kept = torch.zeros(p, dtype=torch.int32, device=dev)
    offsets = torch.zeros(p + 1, dtype=torch.int64, device=dev)
    if p:
        ctx = _lib.context_for(ctx, dev)
        ctx.check(ctx.lib.hive_pairs_compact(ctx.handle, ptr(rows), ptr(counts), ptr(mask), ptr(result), p, stride, int(min_features), ptr(out), ptr(kept), ptr(offsets)))
    return out, kept, offsets
