"""Feature pairs for pose optimisation (``FeatureExtractor`` of hive/pose_optimisation.py:224-656, at the end of this file) and foreground trajectory smoothing
(``--fts_num_epochs N``): ``ForegroundPoseOptimiser`` of hive/pose_optimisation.py:1618-1711 on the MI355X.

An Adam loop over the camera poses that damps the jitter of the dynamic objects: the centroid of every frame's object pixels is put into world space with the
initial poses, and the poses are then moved so that those world-space centroids stay where they were while the camera path gets smoother.

  ``centroids``                 per-frame mean of ``point_cloud_from_depth(depth, mask > 0, K)`` and its point count (``hive_fg_centroids``)
  ``dataset_centroids``         the same for every frame of a dataset, uploaded in chunks
  ``find_chunks``               maximal runs of frames with object pixels, at least three long (:1650-1663)
  ``fts_optimise``              the loss, its gradient and the Adam loop in one launch (``hive_fts_optimise``)
  ``ForegroundPoseOptimiser``   the reference's class: ``ForegroundPoseOptimiser(dataset, learning_rate, num_epochs).run() -> Trajectory``

Deviation from the reference, on purpose: the parameters are float64 here (the reference keeps them in float32 and promotes inside the loss); the start values
are the reference's float32 ``dataset.camera_trajectory.tensor()``, widened.  tests/test_fts_gpu.py bounds the difference by the reference's own rounding.
"""
import enum
import logging

import numpy as np

from hive_amd import _lib
from hive_amd._lib import ptr
from hive_amd.geometric import Trajectory

MIN_CHUNK_SIZE = 3  # pose_optimisation.py:1648
UPLOAD_CHUNK_FRAMES = 64


def centroids(depth, masks, camera_matrix, ctx=None):
    """For every frame of a device-resident batch -- ``depth`` float32 (n, H, W), ``masks`` uint8 (n, H, W) instance ids -- the mean, in camera space, of the points
    ``point_cloud_from_depth(depth[i], masks[i] > 0, camera_matrix)`` and their number, without materialising the point cloud.  Returns (float64 (n, 3), int64 (n,))
    numpy arrays; a frame without a valid object pixel has count 0 and centroid 0.  Bit-identical from run to run (fixed float64 reduction tree)."""
    import torch
    from hive_amd.geometric import _kinv
    assert depth.dtype == torch.float32 and masks.dtype == torch.uint8 and depth.dim() == 3 and tuple(depth.shape) == tuple(masks.shape), \
        "depth float32 (n, H, W) and masks uint8 (n, H, W) device tensors"
    ctx = ctx or _lib.default_context(depth.device.index or 0)
    ctx.follow_torch_stream()
    depth, masks = depth.contiguous(), masks.contiguous()
    n, h, w = (int(v) for v in depth.shape)
    Kinv = _kinv(np.asarray(camera_matrix).reshape(3, 3))
    out, counts = np.zeros((n, 3), np.float64), np.zeros(n, np.int64)
    ctx.check(ctx.lib.hive_fg_centroids(ctx.handle, ptr(depth), ptr(masks), n, h, w, ptr(Kinv), ptr(out), ptr(counts)))
    return out, counts


def dataset_centroids(dataset, num_frames=None, chunk_frames=UPLOAD_CHUNK_FRAMES, ctx=None):
    """``centroids`` for frames 0 .. num_frames - 1 of ``dataset.depth_dataset`` / ``dataset.mask_dataset`` (the reference's ``get_point_cloud``, :1626-1634), through
    one reused set of pinned and device buffers of ``chunk_frames`` frames (``fusion._Staging``)."""
    from hive_amd.fusion import _Staging
    n = dataset.num_frames if num_frames is None else int(num_frames)
    out, counts = np.zeros((n, 3), np.float64), np.zeros(n, np.int64)
    staging = None
    for a in range(0, n, chunk_frames):
        b = min(n, a + chunk_frames)
        first = np.asarray(dataset.depth_dataset[a])
        if staging is None:
            staging = _Staging(min(chunk_frames, n), *first.shape[:2])
        _, depth_h, masks_h = staging.host(b - a, False, True)
        for j, i in enumerate(range(a, b)):
            depth_h.numpy()[j] = first if j == 0 else dataset.depth_dataset[i]
            masks_h.numpy()[j] = dataset.mask_dataset[i]
        _, depth, masks = staging.upload(b - a, False, True)
        out[a:b], counts[a:b] = centroids(depth, masks, dataset.camera_matrix, ctx=ctx)
    return out, counts


def find_chunks(counts, min_chunk_size=MIN_CHUNK_SIZE):
    """Maximal runs of consecutive frames with a non-empty point cloud, runs shorter than ``min_chunk_size`` dropped (:1650-1663): a list of (first frame, length)."""
    chunks, start = [], None
    for i, c in enumerate(list(counts) + [0]):
        if c > 0:
            start = i if start is None else start
        else:
            if start is not None and i - start >= min_chunk_size:
                chunks.append((start, i - start))
            start = None
    return chunks


def fts_optimise(params, centroids_camera_space, chunks, learning_rate=1e-5, num_epochs=100, gt_params=None, return_gradient=False, ctx=None):
    """The Adam loop of ``ForegroundPoseOptimiser.run`` (:1669-1709), all epochs in one launch (``hive_fts_optimise``; loss, gradients and update rule in
    include/hive_mi355x.h).  ``params`` (N, 7) rows [scalar-last quaternion, translation]; ``centroids_camera_space`` (N, 3); ``chunks`` a list of (first frame, length >= 3);
    ``gt_params``: the parameters the fixed world-space centroids are taken at (default: ``params``, as in the reference).  Returns (parameters float64 (N, 7), NOT
    normalised, losses float64 (num_epochs + 1,): before every step and at the returned parameters) and, with ``return_gradient``, dL/dparams at the returned
    parameters (with ``num_epochs=0``: at ``params``).  Without chunks the loss is 0 and only the weight decay acts."""
    ctx = ctx or _lib.default_context()
    p = np.array(params, dtype=np.float64, order="C")
    assert p.ndim == 2 and p.shape[1] == 7, "params (N, 7)"
    n = p.shape[0]
    c = np.ascontiguousarray(centroids_camera_space, dtype=np.float64)
    assert c.shape == (n, 3), "centroids (N, 3)"
    g = None if gt_params is None else np.ascontiguousarray(gt_params, dtype=np.float64)
    assert g is None or g.shape == (n, 7), "gt_params (N, 7)"
    start = np.ascontiguousarray([s for s, _ in chunks], dtype=np.int32)
    length = np.ascontiguousarray([m for _, m in chunks], dtype=np.int32)
    losses = np.zeros(int(num_epochs) + 1, np.float64)
    grad = np.zeros((n, 7), np.float64) if return_gradient else None
    ctx.check(ctx.lib.hive_fts_optimise(ctx.handle, ptr(p), ptr(g), ptr(c), n, ptr(start) if len(chunks) else None, ptr(length) if len(chunks) else None,
                                        len(chunks), float(learning_rate), int(num_epochs), ptr(losses), ptr(grad)))
    return (p, losses, grad) if return_gradient else (p, losses)


class ForegroundPoseOptimiser:
    """The reference's ``ForegroundPoseOptimiser`` (:1618-1711).  ``run()`` returns the smoothed ``Trajectory`` = rows [q / |q|, t] (``get_trajectory``, float64); the
    dataset and its stored trajectory are not touched.  Without a single chunk (no run of three frames with object pixels) the reference calls ``backward()`` on a
    constant and raises; here ``run()`` logs a line and returns the input trajectory (widened to float64, quaternions normalised), no epoch applied."""

    def __init__(self, dataset, learning_rate=1e-5, num_epochs=100):
        self.dataset = dataset
        self.learning_rate = learning_rate
        self.num_epochs = num_epochs
        self.losses = None  # after run(): the loss before every epoch's step and at the returned poses

    def run(self) -> Trajectory:
        centroids_camera_space, counts = dataset_centroids(self.dataset)
        start = self.dataset.camera_trajectory.tensor().numpy().astype(np.float64)  # the reference's float32 start values, widened
        chunks = find_chunks(counts)
        if not chunks:
            logging.info("Foreground trajectory smoothing: no run of %d consecutive frames with dynamic objects, trajectory left as it is.", MIN_CHUNK_SIZE)
            self.losses = np.zeros(1)
            params = start
        else:
            params, self.losses = fts_optimise(start, centroids_camera_space, chunks, self.learning_rate, self.num_epochs)
        out = params.copy()
        out[:, :4] = params[:, :4] / np.linalg.norm(params[:, :4], ord=2, axis=1).reshape((-1, 1))
        return Trajectory(out)


# ---- feature pairs: FrameSamplingMode, FeatureData / FeatureSet and the FeatureExtractor of hive/pose_optimisation.py:61-656 ----
class FrameSamplingMode(enum.Enum):
    """How frame pairs are sampled from a sequence (:61-74)."""
    Exhaustive = enum.auto()                  # every (i, j), i < j
    Consecutive = enum.auto()                 # (0, 1), (1, 2), (2, 3), ...
    ConsecutiveNoOverlap = enum.auto()        # (0, 1), (2, 3), (4, 5), ...
    ConsecutiveNoOverlapOffset = enum.auto()  # (1, 2), (3, 4), (5, 6), ...
    Hierarchical = enum.auto()                # consecutive pairs, then pairs 2, 4, 8, ... frames apart


def sample_frame_pairs(mode, num_frames):
    """The pair lists of ``PoseOptimiser._sample_frame_pairs`` (:1042-1092).  Hierarchical: for level 0 .. floor(log2(num_frames - 1)), step = 1 << level, every
    (start, start + step) with start a multiple of the step and start + step < num_frames, the levels in ascending order.  Fewer than two frames give []."""
    n = int(num_frames)
    if not isinstance(mode, FrameSamplingMode):
        raise RuntimeError(f"Unsupported frame sampling mode: {mode}.")
    if n < 2:
        return []
    if mode == FrameSamplingMode.Exhaustive:
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    if mode == FrameSamplingMode.Hierarchical:
        pairs = []
        for level in range((n - 1).bit_length()):  # bit_length(n - 1) - 1 = floor(log2(n - 1))
            step = 1 << level
            pairs += [(start, start + step) for start in range(0, n, step) if start + step < n]
        return pairs
    start = 1 if mode == FrameSamplingMode.ConsecutiveNoOverlapOffset else 0
    step = 1 if mode == FrameSamplingMode.Consecutive else 2
    return [(i, i + 1) for i in range(start, n - 1, step)]


class FeatureData:
    """The frame index, the image coordinates and the depth of one side of the correspondences (:84-113): int64 (N,), float32 (N, 2), float32 (N,), plain tensors
    on one device."""

    def __init__(self, index=None, points=None, depth=None):
        import torch
        self.index = (torch.empty(0, dtype=torch.long) if index is None else torch.as_tensor(index)).to(torch.long)
        self.points = (torch.empty((0, 2), dtype=torch.float32) if points is None else torch.as_tensor(points)).to(torch.float32).reshape(-1, 2)
        self.depth = (torch.empty(0, dtype=torch.float32) if depth is None else torch.as_tensor(depth)).to(torch.float32)
        if not len(self.index) == len(self.points) == len(self.depth):
            raise ValueError(f"index, points and depth have {len(self.index)}, {len(self.points)} and {len(self.depth)} rows")

    def __len__(self):
        return len(self.index)

    def to(self, device):
        return FeatureData(self.index.to(device), self.points.to(device), self.depth.to(device))

    def sample_at(self, frame_indices):
        """A copy of the rows ``frame_indices`` names: a tensor of row numbers or a boolean mask."""
        return FeatureData(self.index[frame_indices].clone(), self.points[frame_indices].clone(), self.depth[frame_indices].clone())


class FeatureSet:
    """What a pose refinement starts from (:116-221): the camera matrix and the two sides of the matched, depth-carrying correspondences of all frame pairs."""

    KEYS = ("frame_i.index", "frame_i.points", "frame_i.depth", "frame_j.index", "frame_j.points", "frame_j.depth")

    def __init__(self, camera_matrix=None, frame_i=None, frame_j=None):
        import torch
        self.camera_matrix = torch.eye(3, dtype=torch.float32) if camera_matrix is None else torch.as_tensor(camera_matrix)
        self.frame_i = FeatureData() if frame_i is None else frame_i
        self.frame_j = FeatureData() if frame_j is None else frame_j
        if len(self.frame_i) != len(self.frame_j):
            raise ValueError(f"frame_i has {len(self.frame_i)} rows, frame_j {len(self.frame_j)}")

    @property
    def device(self):
        return self.camera_matrix.device

    def __len__(self):
        return len(self.frame_i)

    def to(self, device):
        return FeatureSet(self.camera_matrix.to(device), self.frame_i.to(device), self.frame_j.to(device))

    def state_dict(self):
        """The reference's keys: ``camera_matrix`` and ``frame_{i,j}.{index,points,depth}``."""
        out = {"camera_matrix": self.camera_matrix}
        for side, data in (("frame_i", self.frame_i), ("frame_j", self.frame_j)):
            out.update({f"{side}.index": data.index, f"{side}.points": data.points, f"{side}.depth": data.depth})
        return out

    def save(self, f):
        """``torch.save`` of the plain dict of ``state_dict()``, on the CPU: what the reference's ``FeatureSet.load`` reads."""
        import torch
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, f)

    @classmethod
    def load(cls, f, device=None):
        """From a file written by ``save`` or by the reference's ``FeatureSet.save`` (its module's state_dict has the same keys)."""
        import torch
        state = torch.load(f, map_location="cpu")
        side = lambda name: FeatureData(state[f"{name}.index"], state[f"{name}.points"], state[f"{name}.depth"])
        out = cls(state["camera_matrix"], side("frame_i"), side("frame_j"))
        return out if device is None else out.to(device)

    def sample_at(self, frame_indices):
        """The correspondences whose two frames are both among ``frame_indices`` (:174-201)."""
        import torch
        frames = torch.as_tensor(sorted(set(int(i) for i in frame_indices)), dtype=torch.long, device=self.frame_i.index.device)
        mask = torch.isin(self.frame_i.index, frames) & torch.isin(self.frame_j.index, frames)
        return FeatureSet(self.camera_matrix.clone(), self.frame_i.sample_at(mask), self.frame_j.sample_at(mask))

    def subset_from(self, frame_pairs):
        """The correspondences of the given frame pairs (:203-221)."""
        import torch
        mask = torch.zeros(len(self), dtype=torch.bool, device=self.frame_i.index.device)
        for i, j in frame_pairs:
            mask |= (self.frame_i.index == int(i)) & (self.frame_j.index == int(j))
        return FeatureSet(self.camera_matrix.clone(), self.frame_i.sample_at(mask), self.frame_j.sample_at(mask))


class FeatureExtractionOptions:
    """Options of the ``FeatureExtractor`` (:224-264), with the reference's checks and warnings."""

    def __init__(self, ignore_dynamic_objects=True, min_features=20, max_features=2048):
        if not isinstance(min_features, int) or min_features < 5:
            raise ValueError(f"`min_features` must be a positive integer that is at least 5, but got {min_features}.")
        if max_features is not None and (not isinstance(max_features, int) or max_features <= min_features):
            raise ValueError(f"`max_features` must be a positive integer greater than `min_features` ({min_features}), but got {max_features}.")
        if min_features < 20:
            logging.warning(f"`min_features` was set to {min_features}, however it is recommended to set `min_features` to at least 20. "
                            f"Anything lower than 20 generally leads to a low SNR and bad results.")
        if max_features is not None and max_features < 2 * min_features:
            logging.warning(f"`max_features` was set to {max_features}, however it is recommended to set `max_features` to at least 2 * `min_features` "
                            f"({2 * min_features}). This is to increase the likelihood that enough features will remain after filtering to meet the requirement "
                            f"of having at least `min_features` features.")
        self.ignore_dynamic_objects = ignore_dynamic_objects
        self.min_features = min_features
        self.max_features = max_features

    def __repr__(self):
        return f"{self.__class__.__name__}(ignore_dynamic_objects={self.ignore_dynamic_objects}, min_features={self.min_features}, max_features={self.max_features})"


class FeatureExtractor:
    """The reference's ``FeatureExtractor`` (:267-656) on the MI355X: for every frame pair the matched SIFT keypoints that pass Lowe's ratio test, have depth on
    both sides and agree with one homography, as a ``FeatureSet`` whose rows follow ``frame_pairs`` and, inside a pair, the query keypoints.

    One ``extract_feature_points`` call runs on the device and synchronises once, at the end, to fetch the counts: gray planes of the frames that occur in a
    pair (cv2's 8-bit COLOR_RGB2GRAY rule, see ``hive_similarity_ssim_psnr``), with ``ignore_dynamic_objects`` the SIFT mask ``mask == 0``, SIFT ONCE per frame
    (the reference detects a frame again for every pair it stands in) with ``nfeatures = max_features``, the pair matcher and its filter
    (``features.match_pairs``), the homography RANSAC (``features.ransac_homography``) on pairs with ``min_features`` survivors, and the compaction by its inlier
    mask, which drops pairs with fewer than ``min_features`` inliers.

    Not pinned against cv2: the keypoints (cv2's SIFT), the matches (the reference's FLANN search is approximate; this one is exact) and the inlier set
    (``cv2.USAC_MAGSAC`` is randomised; the RANSAC here is the rule stated in include/hive_mi355x.h, a function of the inputs, ``seed`` and the frame pair).
    ``ransac_threshold`` and ``ransac_trials`` are cv2.findHomography's defaults.  With ``debug_path``, ``frame_pairs.txt`` and ``feature_set.pth`` are written
    there and the feature set is reused while the pair list stays the same (:367-402); the reference's match pictures (``cv2.drawMatchesKnn``) are NOT written.
    ``sift``: a ``features.SIFT`` to use (one with ``nfeatures = max_features`` and room for 8192 candidates a frame otherwise)."""

    UPLOAD_CHUNK_FRAMES = 64
    OWN_SIFT_CAPACITY = 8192

    def __init__(self, dataset, frame_pairs, feature_extraction_options=None, debug_path=None, sift=None, ransac_threshold=3.0, ransac_trials=2000, seed=0,
                 device=None):
        self.dataset = dataset
        self.frame_pairs = [(int(i), int(j)) for i, j in frame_pairs]
        self.options = feature_extraction_options or FeatureExtractionOptions()
        self.debug_path = debug_path
        self.frame_pairs_path = self.feature_set_path = None
        self.sift, self.ransac_threshold, self.ransac_trials, self.seed, self.device = sift, float(ransac_threshold), int(ransac_trials), int(seed), device
        self.pair_stats = None  # after a run on the device: int (P, 5) per pair -- ratio survivors, survivors, winning trial, the winner's count, rows kept

    @property
    def min_features(self):
        return self.options.min_features

    @property
    def max_features(self):
        return self.options.max_features

    @property
    def ignore_dynamic_objects(self):
        return self.options.ignore_dynamic_objects

    def _setup_folders(self):
        """The cache rule of :367-402: the stored feature set is kept only while ``frame_pairs.txt`` holds this pair list."""
        if self.debug_path is None:
            return
        import os
        self.frame_pairs_path = os.path.join(self.debug_path, "frame_pairs.txt")
        self.feature_set_path = os.path.join(self.debug_path, "feature_set.pth")
        os.makedirs(self.debug_path, exist_ok=True)
        wanted = np.asarray(self.frame_pairs, dtype=np.float64).reshape(-1, 2)
        if os.path.isfile(self.frame_pairs_path):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)  # an empty list
                cached = np.loadtxt(self.frame_pairs_path, ndmin=2).reshape(-1, 2)
            if cached.shape == wanted.shape and bool(np.all(cached == wanted)):
                return
        for path in (self.frame_pairs_path, self.feature_set_path):
            if os.path.isfile(path):
                os.remove(path)
        np.savetxt(self.frame_pairs_path, wanted)

    def _upload(self, frames, device):
        """Gray planes, SIFT masks (or None) and depth maps of ``frames`` as device tensors (n, H, W)."""
        import torch
        first = np.asarray(self.dataset.rgb_dataset[frames[0]])
        n, (h, w) = len(frames), first.shape[:2]
        gray = torch.empty((n, h, w), dtype=torch.uint8, device=device)
        depth = torch.empty((n, h, w), dtype=torch.float32, device=device)
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=device) if self.ignore_dynamic_objects else None
        for a in range(0, n, self.UPLOAD_CHUNK_FRAMES):
            part = frames[a:a + self.UPLOAD_CHUNK_FRAMES]
            rgb = torch.from_numpy(np.stack([np.asarray(self.dataset.rgb_dataset[i])[..., :3] for i in part])).to(device).to(torch.int32)
            # cv2's 8-bit COLOR_RGB2GRAY: exact integers
            gray[a:a + len(part)] = ((4899 * rgb[..., 0] + 9617 * rgb[..., 1] + 1868 * rgb[..., 2] + 8192) >> 14).to(torch.uint8)
            depth[a:a + len(part)] = torch.from_numpy(np.stack([np.asarray(self.dataset.depth_dataset[i], dtype=np.float32) for i in part])).to(device)
            if mask is not None:  # dynamic objects are 0: SIFT ignores them (:422-429)
                mask[a:a + len(part)] = (torch.from_numpy(np.stack([np.asarray(self.dataset.mask_dataset[i]) for i in part])).to(device) == 0).to(torch.uint8)
        return gray, mask, depth

    def extract_feature_points(self):
        import os

        import torch
        from hive_amd import features as F
        logging.info("Extracting image feature matches...")
        self._setup_folders()
        device = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.feature_set_path and os.path.isfile(self.feature_set_path):
            logging.info(f"Found cached feature set at: {self.feature_set_path}")
            return FeatureSet.load(self.feature_set_path, device=device)
        camera_matrix = torch.from_numpy(np.array(self.dataset.camera_matrix, copy=True)).to(device)
        pairs = np.asarray(self.frame_pairs, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.dataset.num_frames):
            raise ValueError(f"frame pairs name frames {int(pairs.min())} .. {int(pairs.max())}; the dataset has {self.dataset.num_frames}")
        if len(pairs) == 0:
            out = FeatureSet(camera_matrix, FeatureData().to(device), FeatureData().to(device))
            self.pair_stats = np.zeros((0, 5), dtype=np.int64)
        else:
            logging.info("Extracting matching image feature info...")
            frames = sorted(set(pairs.flatten().tolist()))  # only frames that occur in a pair
            picture = {f: k for k, f in enumerate(frames)}
            gray, mask, depth = self._upload(frames, device)
            sift = self.sift or F.SIFT(nfeatures=self.max_features or 0, capacity=self.OWN_SIFT_CAPACITY)
            try:
                feats = sift.detect_device(gray, mask)
                pictures = np.vectorize(picture.get)(pairs)
                rows, counts = F.match_pairs(feats, pictures, depth, ratio=0.7, min_features=self.min_features)
                _, inlier_mask, result = F.ransac_homography(rows, counts[:, 1], pairs, self.ransac_threshold, self.ransac_trials, self.seed, min_count=self.min_features)
                data, kept, offsets = F.compact_pairs(rows, counts, inlier_mask, result, self.min_features)
                # the one synchronisation: every count in one copy
                host = torch.cat([feats[2].flatten().long(), counts.flatten().long(), result.flatten().long(), kept.long(), offsets]).cpu().numpy()
            finally:
                if self.sift is None:
                    sift.close()
            n, p = len(frames), len(pairs)
            sift.check_counts(host[:3 * n].reshape(n, 3))
            counts_h, result_h = host[3 * n:3 * n + 2 * p].reshape(p, 2), host[3 * n + 2 * p:3 * n + 5 * p].reshape(p, 3)
            kept_h, total = host[3 * n + 5 * p:3 * n + 6 * p], int(host[-1])
            self.pair_stats = np.concatenate([counts_h, result_h[:, :2], kept_h[:, None]], axis=1)
            data = data[:total]
            kept_d = kept.long()
            index_i = torch.repeat_interleave(torch.from_numpy(pairs[:, 0].copy()).to(device), kept_d, output_size=total)
            index_j = torch.repeat_interleave(torch.from_numpy(pairs[:, 1].copy()).to(device), kept_d, output_size=total)
            out = FeatureSet(camera_matrix, FeatureData(index_i, data[:, 0:2].clone(), data[:, 4].clone()), FeatureData(index_j, data[:, 2:4].clone(), data[:, 5].clone()))
        self._print_results_stats(out.frame_i.index, out.frame_j.index, int((self.pair_stats[:, 4] > 0).sum()))
        if self.feature_set_path:
            out.save(self.feature_set_path)
        return out

    def _print_results_stats(self, index_i, index_j, num_good_frame_pairs):
        """The log lines of :630-655."""
        import torch
        covered = set(torch.unique(torch.cat([index_i, index_j])).tolist())
        coverage = len(covered) / max(self.dataset.num_frames, 1)
        logging.info(f"Found {num_good_frame_pairs} good frame pairs ({num_good_frame_pairs}/{len(self.frame_pairs)})")
        logging.info(f"Frame pairs cover {100 * coverage:.2f}% of the frames.")
        chunks, inside = 0, False
        for frame_index in range(self.dataset.num_frames):
            chunks += 1 if frame_index in covered and not inside else 0
            inside = frame_index in covered
        logging.info(f"Found {chunks} group(s) of consecutive frames.")
