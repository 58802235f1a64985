"""Pose optimisation on the MI355X: the feature pairs (``FeatureExtractor`` of hive/pose_optimisation.py:224-656), the ``PoseOptimiser`` that consumes them
(:659-1615) and the foreground trajectory smoothing (``--fts_num_epochs N``: ``ForegroundPoseOptimiser``, :1618-1711).

``PoseOptimiser`` / ``optimise_poses``: the reference's Adam loop over the camera poses as ONE native loop (``hive_pose_optimise``, csrc/poseopt.hip): hand-derived
gradients gathered per frame without floating-point atomics, the learning-rate scheduler and the early stop on the device, two launches an epoch and one
read-back per ``check_every`` epochs.  Deliberate deviations from the reference, none of them pinned against the reference's run:

  * PROJECTED ADAM.  The reference assigns a new ``torch.nn.Parameter`` for the normalised quaternions (and, with ``clip_distance``, the clipped positions) every
    epoch while its optimiser keeps the old objects, whose ``.grad`` stays None: its ``step()`` moves nothing, the loss never changes and early stopping ends the
    run after 76 epochs.  Built here is the intent: every epoch normalises the quaternions and clips the positions IN PLACE, as projections of the live
    parameters, and Adam steps those same parameters with its moments and step count carried through.
  * float64 parameters (the reference: float32); the start values are the reference's float32 values, widened; ``scale`` and ``shift`` come back as float64 numpy.
  * ``OptimisationOptions.copy()`` carries ``clip_distance``; ``OptimisationOptions`` validates ``steps``.
  * ``AlignmentType.Deformable`` raises NotImplementedError.

Foreground trajectory smoothing: an Adam loop over the camera poses that damps the jitter of the dynamic objects: the centroid of every frame's object pixels is
put into world space with the initial poses, and the poses are then moved so that those world-space centroids stay where they were while the camera path gets
smoother.

  ``centroids``                 per-frame mean of ``point_cloud_from_depth(depth, mask > 0, K)`` and its point count (``hive_fg_centroids``)
  ``dataset_centroids``         the same for every frame of a dataset, uploaded in chunks
  ``find_chunks``               maximal runs of frames with object pixels, at least three long (:1650-1663)
  ``fts_optimise``              the loss, its gradient and the Adam loop in one launch (``hive_fts_optimise``)
  ``ForegroundPoseOptimiser``   the reference's class: ``ForegroundPoseOptimiser(dataset, learning_rate, num_epochs).run() -> Trajectory``

Deviation from the reference, on purpose: the parameters are float64 here (the reference keeps them in float32 and promotes inside the loss); the start values
are the reference's float32 ``dataset.camera_trajectory.tensor()``, widened.  tests/test_fts_gpu.py bounds the difference by the reference's own rounding.
"""
import ctypes
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
    ctx = _lib.context_for(ctx, depth.device)
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
    ``sift``: a ``features.SIFT`` to use (one with ``nfeatures = max_features`` and room for 8192 candidates a frame otherwise).

    ``model="rigid"``: the inlier mask comes from ``features.ransac_rigid`` (csrc/register.hip) on the same rows, back-projected with the dataset's camera
    matrix, in the place of the homography, which is exact only for a plane or a pure rotation; ``rigid_threshold`` is in the depth's unit (0.05 is a parameter
    default, 5 cm for metres, not a measured quantity) and ``with_scale`` fits a similarity.  The compaction and the ``FeatureSet`` are as before, and
    ``pair_transforms = (T, scale, rms, result)`` holds the relative transforms as host arrays after the run (``registration.chain_pairs`` makes a trajectory
    and per-frame depth scales of them; the hand-off to the Affine alignment is ``scale_parameters = 1 / depth_scale``).  A cached feature set under
    ``debug_path`` carries no transforms: ``pair_transforms`` stays None when it is reused."""

    UPLOAD_CHUNK_FRAMES = 64
    OWN_SIFT_CAPACITY = 8192

    def __init__(self, dataset, frame_pairs, feature_extraction_options=None, debug_path=None, sift=None, ransac_threshold=3.0, ransac_trials=2000, seed=0,
                 device=None, model="homography", rigid_threshold=0.05, with_scale=False):
        if model not in ("homography", "rigid"):
            raise ValueError(f"model = {model!r}; 'homography' or 'rigid'")
        self.model, self.rigid_threshold, self.with_scale = model, float(rigid_threshold), bool(with_scale)
        self.pair_transforms = None  # after a run with model="rigid": host arrays (T (P, 4, 4), scale (P,), rms (P,), result (P, 3)) of features.ransac_rigid
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
            if self.model == "rigid":
                self.pair_transforms = (np.zeros((0, 4, 4)), np.zeros(0), np.zeros(0), np.zeros((0, 3), dtype=np.int64))
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
                rigid = None
                if self.model == "rigid":
                    *rigid, inlier_mask, result = F.ransac_rigid(rows, counts[:, 1], pairs, self.dataset.camera_matrix, self.rigid_threshold, self.ransac_trials, self.seed,
                                                                 min_count=self.min_features, with_scale=self.with_scale)
                else:
                    _, inlier_mask, result = F.ransac_homography(rows, counts[:, 1], pairs, self.ransac_threshold, self.ransac_trials, self.seed, min_count=self.min_features)
                data, kept, offsets = F.compact_pairs(rows, counts, inlier_mask, result, self.min_features)
                # the one synchronisation: every count in one copy
                host = torch.cat([feats[2].flatten().long(), counts.flatten().long(), result.flatten().long(), kept.long(), offsets])
                if rigid is None:
                    host = host.cpu().numpy()
                else:  # the transforms ride in the same copy: every count is far below 2^53
                    both = torch.cat([host.double()] + [t.flatten() for t in rigid]).cpu().numpy()
                    host, rigid = both[:len(host)].astype(np.int64), both[len(host):]
            finally:
                if self.sift is None:
                    sift.close()
            n, p = len(frames), len(pairs)
            sift.check_counts(host[:3 * n].reshape(n, 3))
            counts_h, result_h = host[3 * n:3 * n + 2 * p].reshape(p, 2), host[3 * n + 2 * p:3 * n + 5 * p].reshape(p, 3)
            kept_h, total = host[3 * n + 5 * p:3 * n + 6 * p], int(host[-1])
            self.pair_stats = np.concatenate([counts_h, result_h[:, :2], kept_h[:, None]], axis=1)
            if rigid is not None:
                self.pair_transforms = (rigid[:16 * p].reshape(p, 4, 4), rigid[16 * p:17 * p], rigid[17 * p:], result_h.copy())
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


# ---- the pose optimiser: AlignmentType .. PoseOptimiser of hive/pose_optimisation.py:659-1615, its Adam loop as hive_pose_optimise (csrc/poseopt.hip) ----
class AlignmentType(enum.Enum):
    """How depth maps are scaled and shifted (if at all) during pose optimisation (:659-669)."""
    Rigid = enum.auto()       # the camera pose alone
    Affine = enum.auto()      # the camera pose and one scale and shift per depth map
    Deformable = enum.auto()  # a 3 x 3 field of scales and shifts per depth map: NOT built here (``optimise_poses`` raises NotImplementedError)


class ResidualType(enum.Enum):
    """How residuals are calculated (:829-842)."""
    World3D = enum.auto()  # both sides of a correspondence in world space: the distance in 3-D
    Image2D = enum.auto()  # side i projected into frame j: the distance in pixels


class OptimisationStep(enum.Enum):
    """Steps of the pose optimisation pipeline (:846-868)."""
    PairWise3D = enum.auto()
    Global3D = enum.auto()
    PairWise2D = enum.auto()
    Global2D = enum.auto()


class EarlyStopping:
    """Whether training has stagnated (:790-825): ``step(loss)`` sets ``should_stop`` once more than ``patience`` calls in a row failed to lower the best loss by
    more than ``min_difference``.  hive_pose_optimise runs the same rule on the device."""

    def __init__(self, patience=10, min_difference=0.0):
        self.patience = patience
        self.min_difference = min_difference
        self.best_loss = float('inf')
        self.calls_since_last_best = 0
        self.should_stop = False

    def step(self, loss) -> bool:
        loss = float(loss)
        if loss < self.best_loss and abs(loss - self.best_loss) > self.min_difference:
            self.best_loss = loss
            self.calls_since_last_best = 0
        else:
            self.calls_since_last_best += 1
        if self.calls_since_last_best > self.patience:
            self.should_stop = True
        return self.should_stop


def _check_number(value, name, kind, positive, nullable=False):
    """The reference's ``check_domain``: ``kind`` int or float (a float option takes an int too), positive or non-negative, None where ``nullable``."""
    if value is None and nullable:
        return
    ok = isinstance(value, kind if kind is int else (int, float)) and not isinstance(value, bool)
    if not ok or not (value > 0 if positive else value >= 0) or value != value:
        raise ValueError(f"`{name}` must be a {'positive' if positive else 'non-negative'} {kind.__name__}{' or None' if nullable else ''}, but got {value!r}.")


class OptimisationOptions:
    """Configuration of the ``PoseOptimiser`` (:871-964), the reference's names and defaults.  Two deliberate deviations: ``copy()`` carries ``clip_distance``
    (the reference drops it, harmlessly there), and ``steps`` is validated -- a non-empty tuple or list of ``OptimisationStep`` (the reference's check can never
    reject a wrong element)."""

    default_pipeline = (OptimisationStep.PairWise3D, OptimisationStep.Global3D)

    def __init__(self, num_epochs=4000, learning_rate=1e-2, l2_regularisation=0.5, min_loss_delta=1e-4, lr_scheduler_patience=50, early_stopping_patience=75,
                 alignment_type=AlignmentType.Rigid, steps=default_pipeline, position_only=False, fine_tune=True, pose_t_reg=0.5, pose_r_reg=1.0,
                 trajectory_smoothing=None, clip_distance=1.0):
        _check_number(num_epochs, 'num_epochs', int, True)
        _check_number(learning_rate, 'learning_rate', float, True)
        _check_number(l2_regularisation, 'l2_regularisation', float, False)
        _check_number(min_loss_delta, 'min_loss_delta', float, True)
        _check_number(lr_scheduler_patience, 'lr_scheduler_patience', int, True)
        _check_number(early_stopping_patience, 'early_stopping_patience', int, True)
        _check_number(pose_t_reg, 'pose_t_reg', float, False)
        _check_number(pose_r_reg, 'pose_r_reg', float, False)
        _check_number(trajectory_smoothing, 'trajectory_smoothing', float, False, nullable=True)
        _check_number(clip_distance, 'clip_distance', float, False, nullable=True)
        if not isinstance(alignment_type, AlignmentType):
            raise ValueError(f"alignment_type must be an {AlignmentType}, but got {alignment_type!r}.")
        if not isinstance(steps, (tuple, list)) or len(steps) == 0:
            raise ValueError(f"steps must a tuple or list with at least one element, got {type(steps)} instead.")
        for step in steps:
            if not isinstance(step, OptimisationStep):
                raise ValueError(f"steps must only contain values of type {OptimisationStep}, but found a value of type {type(step)}")
        self.num_epochs = num_epochs
        self.learning_rate = learning_rate
        self.l2_regularisation = l2_regularisation
        self.min_loss_delta = min_loss_delta
        self.lr_scheduler_patience = lr_scheduler_patience
        self.early_stopping_patience = early_stopping_patience
        self.alignment_type = alignment_type
        self.steps = steps
        self.position_only = position_only
        self.pose_t_reg = pose_t_reg
        self.pose_r_reg = pose_r_reg
        self.fine_tune = fine_tune
        self.trajectory_smoothing = trajectory_smoothing
        self.clip_distance = clip_distance

    _FIELDS = ("num_epochs", "learning_rate", "l2_regularisation", "min_loss_delta", "lr_scheduler_patience", "early_stopping_patience", "alignment_type", "steps",
               "position_only", "pose_t_reg", "pose_r_reg", "fine_tune", "trajectory_smoothing", "clip_distance")

    def __repr__(self):
        return f"{self.__class__.__name__}(" + ", ".join(f"{name}={getattr(self, name)}" for name in self._FIELDS) + ")"

    def copy(self) -> 'OptimisationOptions':
        return OptimisationOptions(**{name: getattr(self, name) for name in self._FIELDS})


class OptimisationParameters:
    """The parameters subject to optimisation (:672-787): a plain holder of float64 arrays -- ``rotation_quaternions`` (N, 4) scalar last, ``translation_vectors``
    (N, 3), and per frame ``scale`` / ``shift`` (N,), empty for Rigid alignment.  The reference's is a torch.nn.Module of float32 Parameters."""

    def __init__(self, initial_camera_poses, alignment_type, scale_parameters=None, shift_parameters=None, dtype=np.float64):
        poses = np.asarray(initial_camera_poses.values if isinstance(initial_camera_poses, Trajectory) else initial_camera_poses)
        if poses.ndim != 2 or poses.shape[1] != 7:
            raise ValueError(f"initial_camera_poses must be (N, 7), but got {poses.shape}")
        self.rotation_quaternions = np.array(poses[:, :4], dtype=dtype)
        self.translation_vectors = np.array(poses[:, 4:], dtype=dtype)
        self.alignment_type = alignment_type
        n = len(poses)
        if alignment_type == AlignmentType.Rigid:
            scale_parameters, shift_parameters = np.empty(0), np.empty(0)
        elif alignment_type == AlignmentType.Affine:
            scale_parameters = np.ones(n) if scale_parameters is None or np.size(scale_parameters) == 0 else scale_parameters
            shift_parameters = np.zeros(n) if shift_parameters is None or np.size(shift_parameters) == 0 else shift_parameters
        elif alignment_type == AlignmentType.Deformable:
            raise NotImplementedError("AlignmentType.Deformable (a 3 x 3 field of scales and shifts per frame) is not built; Rigid and Affine are.")
        else:
            raise RuntimeError(f"Unsupported alignment type {alignment_type}.")
        self.scale = np.array(scale_parameters, dtype=dtype)
        self.shift = np.array(shift_parameters, dtype=dtype)

    @property
    def dtype(self):
        return self.rotation_quaternions.dtype

    @property
    def num_frames(self):
        return len(self.rotation_quaternions)

    def __len__(self) -> int:
        """The number of optimisation parameters."""
        return int(self.rotation_quaternions.size + self.translation_vectors.size + self.scale.size + self.shift.size)

    def poses(self):
        """(N, 7) rows [raw quaternion, translation]."""
        return np.hstack((self.rotation_quaternions, self.translation_vectors))

    def normalise_rotations(self):
        """Scale the rotation quaternions to unit vectors, in place."""
        self.rotation_quaternions /= np.linalg.norm(self.rotation_quaternions, ord=2, axis=1).reshape((-1, 1))

    def get_trajectory(self) -> Trajectory:
        r = self.rotation_quaternions / np.linalg.norm(self.rotation_quaternions, ord=2, axis=1).reshape((-1, 1))
        return Trajectory(np.hstack((r, self.translation_vectors)))

    def sample_at(self, frame_indices) -> 'OptimisationParameters':
        frame_indices = list(frame_indices)
        has = self.scale.size > 0
        return OptimisationParameters(self.poses()[frame_indices], self.alignment_type, self.scale[frame_indices] if has else None,
                                      self.shift[frame_indices] if has else None, self.dtype)

    def clone(self) -> 'OptimisationParameters':
        return OptimisationParameters(self.poses(), self.alignment_type, self.scale.copy(), self.shift.copy(), self.dtype)


class _PoseOptions(ctypes.Structure):
    """``hive_pose_options`` of include/hive_mi355x.h."""
    _fields_ = [("num_epochs", ctypes.c_int32), ("lr_scheduler_patience", ctypes.c_int32), ("early_stopping_patience", ctypes.c_int32),
                ("alignment_type", ctypes.c_int32), ("residual_type", ctypes.c_int32), ("smooth_trajectory", ctypes.c_int32), ("position_only", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("learning_rate", ctypes.c_double), ("l2_regularisation", ctypes.c_double), ("min_loss_delta", ctypes.c_double),
                ("pose_t_reg", ctypes.c_double), ("pose_r_reg", ctypes.c_double)]


DEFAULT_CHECK_EVERY = 64  # epochs enqueued between two reads of the device-side stop flag: ~1 ms of queued launches, one read in 64 epochs


def project_poses(poses, max_frame_distance=None, ctx=None):
    """One epoch's projection alone (``hive_pose_project``): quaternions normalised, positions clipped to ``max_frame_distance`` between adjacent frames (None: no
    clip), in the order include/hive_mi355x.h states.  ``poses`` (N, 7); returns a float64 copy."""
    ctx = ctx or _lib.default_context()
    p = np.array(poses, dtype=np.float64, order="C")
    assert p.ndim == 2 and p.shape[1] == 7, "poses (N, 7)"
    ctx.check(ctx.lib.hive_pose_project(ctx.handle, ptr(p), len(p), -1.0 if max_frame_distance is None else float(max_frame_distance)))
    return p


def optimise_poses(feature_set, parameters, options=None, residual_type=ResidualType.World3D, smooth_trajectory=True, fps=None, check_every=DEFAULT_CHECK_EVERY,
                   return_gradient=False, num_epochs=None, ctx=None):
    """The loop of ``PoseOptimiser._optimisation_loop`` (:1256-1338) as ``hive_pose_optimise``: projected Adam with hand-derived gradients, the scheduler and the
    early stop on the device (rule and deviations: module docstring, include/hive_mi355x.h).  ``feature_set``: a ``FeatureSet`` on the device; ``parameters``: an
    ``OptimisationParameters`` (left untouched); ``options``: ``OptimisationOptions`` -- its ``clip_distance`` (metres a second) needs ``fps``; ``num_epochs``
    overrides the options' (0: evaluate only).  Returns (parameters, losses (epochs_run,), learning rates (epochs_run,), epochs_run): the RAW parameters after the
    last step, the loss of every epoch before its step, the learning rate after the scheduler saw it.  With ``return_gradient`` also the loss at the returned
    parameters and its gradient (N, 9) = d/d(quaternion, translation, scale, shift), pins applied."""
    import torch
    options = options or OptimisationOptions()
    alignment = parameters.alignment_type
    if alignment == AlignmentType.Deformable or options.alignment_type == AlignmentType.Deformable:
        raise NotImplementedError("AlignmentType.Deformable (a 3 x 3 field of scales and shifts per frame) is not built; Rigid and Affine are.")
    if not isinstance(residual_type, ResidualType):
        raise RuntimeError(f"optimise_poses got given an unsupported residuals type {residual_type}.")
    if options.clip_distance is not None and fps is None:
        raise ValueError("options.clip_distance is metres a second: pass the dataset's fps (or clip_distance=None)")
    if len(feature_set) == 0:
        raise ValueError("the feature set holds no correspondence")
    if feature_set.frame_i.index.device.type != "cuda":
        raise ValueError("the feature set must be on the device (FeatureSet.to('cuda')): hive_amd has no CPU fallback")
    ctx = _lib.context_for(ctx, feature_set.frame_i.index.device)
    epochs = int(options.num_epochs if num_epochs is None else num_epochs)
    affine = alignment == AlignmentType.Affine
    K = feature_set.camera_matrix.detach().cpu().numpy().astype(np.float64)
    sides = [(s.index.contiguous(), s.points.contiguous(), s.depth.contiguous()) for s in (feature_set.frame_i, feature_set.frame_j)]
    assert all(i.dtype == torch.long and p.dtype == torch.float32 and d.dtype == torch.float32 for i, p, d in sides)
    n = parameters.num_frames
    p = np.array(parameters.poses(), dtype=np.float64, order="C")
    scale = np.array(parameters.scale, dtype=np.float64) if affine else None
    shift = np.array(parameters.shift, dtype=np.float64) if affine else None
    o = _PoseOptions(num_epochs=epochs, lr_scheduler_patience=int(options.lr_scheduler_patience), early_stopping_patience=int(options.early_stopping_patience),
                     alignment_type=1 if affine else 0, residual_type=0 if residual_type == ResidualType.World3D else 1, smooth_trajectory=int(bool(smooth_trajectory)),
                     position_only=int(bool(options.position_only)), reserved=0, learning_rate=float(options.learning_rate),
                     l2_regularisation=float(options.l2_regularisation), min_loss_delta=float(options.min_loss_delta), pose_t_reg=float(options.pose_t_reg),
                     pose_r_reg=float(options.pose_r_reg))
    losses, rates = np.zeros(max(epochs, 1), np.float64), np.zeros(max(epochs, 1), np.float64)
    ran, final = ctypes.c_int(0), np.zeros(1, np.float64)
    grad = np.zeros((n, 9), np.float64) if return_gradient else None
    max_distance = -1.0 if options.clip_distance is None else float(options.clip_distance) * (1.0 / float(fps))
    ctx.check(ctx.lib.hive_pose_optimise(ctx.handle, ptr(p), ptr(scale), ptr(shift), n, K[0, 0], K[1, 1], K[0, 2], K[1, 2], ptr(sides[0][0]), ptr(sides[0][1]),
                                         ptr(sides[0][2]), ptr(sides[1][0]), ptr(sides[1][1]), ptr(sides[1][2]), len(feature_set), ctypes.addressof(o), max_distance,
                                         int(check_every), ptr(losses), ptr(rates), ctypes.byref(ran), ptr(final) if return_gradient else None, ptr(grad)))
    out = OptimisationParameters(p, alignment, scale, shift)
    result = (out, losses[:ran.value].copy(), rates[:ran.value].copy(), int(ran.value))
    return result + (float(final[0]), grad) if return_gradient else result


class PoseOptimiser:
    """The reference's ``PoseOptimiser`` (:967-1615): ``PoseOptimiser(dataset, frame_sampling, feature_extraction_options, optimisation_options, debug)
    .run(num_frames) -> (Trajectory, scale, shift)``; ``scale`` / ``shift`` float64 numpy.  Features by ``FeatureExtractor``, every optimisation loop by
    ``optimise_poses`` (projected Adam -- the deliberate deviation the module docstring states), the host-side steps in numpy / scipy as the reference has
    them.  The dataset's stored trajectory is not touched.  A loop over a feature set without a single correspondence (the offset run of a two-frame sequence)
    returns its parameters as they are, with a log line; the reference takes a mean over nothing there.  The match visualisations are not written."""

    DEBUG_FOLDER = 'pose_optim'

    def __init__(self, dataset, frame_sampling=FrameSamplingMode.Hierarchical, feature_extraction_options=None, optimisation_options=None, debug=True,
                 check_every=DEFAULT_CHECK_EVERY):
        self.dataset = dataset
        self.frame_sampling = frame_sampling
        self.feature_extraction_options = feature_extraction_options or FeatureExtractionOptions()
        self.optimisation_options = optimisation_options or OptimisationOptions()
        self.debug = debug
        self.debug_path = None
        self.check_every = check_every
        self.history = []  # after run(): per loop (label, losses, learning rates, epochs run)

    def run(self, num_frames=-1):
        if num_frames == -1:
            num_frames = self.dataset.num_frames
        # the reference's float32 start values, widened
        start = np.asarray(self.dataset.camera_trajectory[:num_frames]).astype(np.float32).astype(np.float64)
        self.history = []
        self._setup_debug_folder()
        frame_pairs = self._sample_frame_pairs(self.frame_sampling)
        fixed_parameters = self._extract_feature_points(frame_pairs, self.feature_extraction_options)
        optimisation_parameters = OptimisationParameters(start, alignment_type=self.optimisation_options.alignment_type)
        optimised_parameters = self._optimise_pose(fixed_parameters, optimisation_parameters, optimisation_options=self.optimisation_options, num_frames=num_frames)
        trajectory = self._interpolate_poses_without_matches(fixed_parameters, optimised_parameters.get_trajectory())
        if self.optimisation_options.trajectory_smoothing:
            trajectory = self._smooth_trajectory(trajectory=trajectory, weight=self.optimisation_options.trajectory_smoothing)
        scale, shift = optimised_parameters.scale.copy(), optimised_parameters.shift.copy()
        if self.debug:
            import os
            trajectory.save(os.path.join(self.debug_path, 'optimised_camera_trajectory.txt'))
            np.savetxt(os.path.join(self.debug_path, 'scale.txt'), scale)
            np.savetxt(os.path.join(self.debug_path, 'shift.txt'), shift)
        return trajectory, scale, shift

    def _setup_debug_folder(self):
        if self.debug:
            import os
            self.debug_path = os.path.join(self.dataset.base_path, self.DEBUG_FOLDER)
            os.makedirs(self.debug_path, exist_ok=True)

    def _sample_frame_pairs(self, frame_sampling_mode, num_frames=-1):
        return sample_frame_pairs(frame_sampling_mode, self.dataset.num_frames if num_frames == -1 else num_frames)

    def _extract_feature_points(self, frame_pairs, feature_extraction_options=None) -> FeatureSet:
        extractor = FeatureExtractor(self.dataset, frame_pairs, feature_extraction_options or FeatureExtractionOptions(), debug_path=self.debug_path)
        return extractor.extract_feature_points().subset_from(frame_pairs)

    def _optimise_pose(self, fixed_parameters, optimisation_parameters, optimisation_options=None, num_frames=-1) -> OptimisationParameters:
        """The step pipeline plus the fine-tune step (:1110-1183)."""
        options = optimisation_options or self.optimisation_options
        if num_frames == -1:
            num_frames = self.dataset.num_frames
        if num_frames != self.dataset.num_frames:
            fixed_parameters = fixed_parameters.sample_at(range(num_frames))
            optimisation_parameters = optimisation_parameters.sample_at(list(range(num_frames)))
        if fixed_parameters.frame_i.index.device.type != "cuda":
            fixed_parameters = fixed_parameters.to("cuda")
        num_steps = len(self.optimisation_options.steps) + (1 if self.optimisation_options.fine_tune else 0)
        if self.debug:
            self.visualise_solution(optimisation_parameters, label="initial_trajectory")
        for i, step in enumerate(self.optimisation_options.steps):
            logging.info(f"Step {i + 1}/{num_steps}: {step.name} Alignment...")
            if step in (OptimisationStep.PairWise2D, OptimisationStep.PairWise3D):
                residual_type = ResidualType.Image2D if step == OptimisationStep.PairWise2D else ResidualType.World3D
                optimisation_parameters = self._optimise_pairwise(fixed_parameters, optimisation_parameters, options, residual_type, num_frames)
            elif step in (OptimisationStep.Global2D, OptimisationStep.Global3D):
                residual_type = ResidualType.Image2D if step == OptimisationStep.Global2D else ResidualType.World3D
                optimisation_parameters = self._optimisation_loop(fixed_parameters, optimisation_parameters, options, residual_type, label=step.name)
            else:
                raise RuntimeError(f"Unsupported optimisation step: {step}.")
            if self.debug:
                self.visualise_solution(optimisation_parameters, f"{i}_{step.name}")
        if self.optimisation_options.fine_tune:
            logging.info(f"Step {num_steps}/{num_steps}: Fine tuning...")
            optimisation_parameters = self._optimisation_loop(fixed_parameters, optimisation_parameters, options, ResidualType.World3D, smooth_trajectory=False,
                                                              label="FineTune")
            if self.debug:
                self.visualise_solution(optimisation_parameters, f"{num_steps}_FineTune")
        return optimisation_parameters

    def _optimise_pairwise(self, fixed_parameters, optimisation_parameters, optimisation_options=None, residual_type=ResidualType.World3D, num_frames=-1):
        """Poses over the consecutive pairs (0, 1), (2, 3), .. and then (1, 2), (3, 4), .. in isolation, Rigid whatever the options say, chained from the
        identity pose by the relative pose of every pair (:1185-1254)."""
        from hive_amd.geometric import add_pose, get_identity_pose, subtract_pose
        if num_frames == -1:
            num_frames = self.dataset.num_frames
        options = (optimisation_options or self.optimisation_options).copy()
        options.alignment_type = AlignmentType.Rigid
        rigid = OptimisationParameters(optimisation_parameters.poses(), AlignmentType.Rigid)
        pose_data = dict()
        for mode in (FrameSamplingMode.ConsecutiveNoOverlap, FrameSamplingMode.ConsecutiveNoOverlapOffset):
            frame_pairs = self._sample_frame_pairs(mode, num_frames)
            feature_set = fixed_parameters.subset_from(frame_pairs)
            trajectory = self._optimisation_loop(feature_set, rigid, options, residual_type=residual_type, label=f"PairWise/{mode.name}").get_trajectory()
            for i, j in frame_pairs:
                pose_data[(i, j)] = trajectory[[i, j]]
        merged = [get_identity_pose()]
        for i, j in sorted(pose_data.keys()):
            pose_i, pose_j = pose_data[i, j]
            merged.append(add_pose(merged[-1], subtract_pose(pose_i, pose_j)))
        return OptimisationParameters(np.asarray(merged), optimisation_parameters.alignment_type, optimisation_parameters.scale, optimisation_parameters.shift,
                                      optimisation_parameters.dtype)

    def _optimisation_loop(self, fixed_parameters, optimisation_parameters, optimisation_options=None, residual_type=ResidualType.World3D, smooth_trajectory=True,
                           label=None) -> OptimisationParameters:
        options = optimisation_options or self.optimisation_options
        if len(fixed_parameters) == 0:
            logging.info("Pose optimisation: no correspondence for this step, parameters left as they are.")
            return optimisation_parameters.clone()
        if options.alignment_type != optimisation_parameters.alignment_type:  # the pair-wise runs force Rigid
            optimisation_parameters = OptimisationParameters(optimisation_parameters.poses(), options.alignment_type)
        out, losses, rates, ran = optimise_poses(fixed_parameters, optimisation_parameters, options, residual_type, smooth_trajectory,
                                                 fps=self.dataset.fps if options.clip_distance is not None else None, check_every=self.check_every)
        self.history.append((label, losses, rates, ran))
        if ran:
            logging.info(f"{label or 'Optimisation'}: {ran} epochs, loss {losses[0]:.4f} -> {losses[-1]:.4f}, LR {rates[-1]:,.2e}")
        return out

    @staticmethod
    def _interpolate_poses_without_matches(feature_set, optimised_camera_trajectory) -> Trajectory:
        """Poses of the frames in no matched pair, by Slerp / linear interpolation between the nearest frames that are (:1521-1569)."""
        import torch
        from scipy.interpolate import interp1d
        from scipy.spatial.transform import Rotation, Slerp
        num_frames = len(optimised_camera_trajectory)
        matched = set(i for i in torch.unique(torch.cat((feature_set.frame_i.index, feature_set.frame_j.index))).tolist() if i < num_frames)
        chunks, chunk = [], []
        for frame_index in range(num_frames):
            if frame_index not in matched:
                chunk.append(frame_index)
            elif chunk:
                chunks.append(chunk)
                chunk = []
        if chunk:
            chunks.append(chunk)
        out = optimised_camera_trajectory.copy()
        for chunk in chunks:
            start, end = max(0, chunk[0] - 1), min(chunk[-1] + 1, num_frames - 1)
            if end == start:
                continue
            times = np.linspace(0, 1, num=end - start + 1)
            slerp = Slerp([0, 1], Rotation.from_quat([optimised_camera_trajectory[start, :4], optimised_camera_trajectory[end, :4]]))
            lerp = interp1d([0, 1], [optimised_camera_trajectory[start, 4:], optimised_camera_trajectory[end, 4:]], axis=0)
            out[start:end + 1, 4:] = lerp(times)
            out[start:end + 1, :4] = slerp(times).as_quat()
        return out

    @staticmethod
    def _smooth_trajectory(trajectory, weight=0.9) -> Trajectory:
        """Exponential moving average of the positions (:1571-1588)."""
        out = trajectory.copy()
        for i in range(1, len(out)):
            out.positions[i] = weight * trajectory.positions[i] + (1 - weight) * out.positions[i - 1]
        return out

    def visualise_solution(self, solution, label):
        """The trajectory on the XY and XZ planes as ``<label>.png`` in the debug folder (:1590-1615), when matplotlib imports."""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            return
        import os
        positions = solution.get_trajectory().positions
        figure, axes = plt.subplots(1, 2, figsize=(12.8, 4.8))
        for axis, (name, column) in zip(axes, (("y", 1), ("z", 2))):
            axis.plot(positions[:, 0], positions[:, column], '-', color="black", label="trajectory")
            axis.legend()
            axis.set_xlabel("x [m]")
            axis.set_ylabel(f"{name} [m]")
            axis.set_title(f"Trajectory on X{name.upper()} Plane")
        plt.tight_layout()
        plt.savefig(os.path.join(self.debug_path, f"{label}.png"), dpi=90)
        plt.close(figure)


def main(argv=None):
    """The reference's command line (:1714-1763): optimise a dataset's poses and, in debug mode, fuse a mesh before and after."""
    import argparse
    import os

    from hive_amd.io import HiveDataset
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset_path', type=str, help='Path to the VTM formatted dataset.')
    parser.add_argument('--num_frames', type=int, default=-1, help='Number of frames to optimise. If set to -1 (default), use all frames.')
    parser.add_argument('--fine_tune', action='store_true', help='Whether to perform an additional fine tuning step.')
    parser.add_argument('--params_init', type=str, choices=['gt', 'random'], default='gt', help='How to initialise the camera trajectory.')
    parser.add_argument('--random_seed', type=int, default=None, help='Random seed to use when initialising camera trajectory with random data.')
    args = parser.parse_args(argv)
    if not HiveDataset.is_valid_folder_structure(args.dataset_path):
        raise RuntimeError(f"The path {args.dataset_path} does not point to a valid dataset.")
    dataset = HiveDataset(args.dataset_path)
    num_frames = args.num_frames
    if num_frames == -1:
        num_frames = dataset.num_frames
    elif num_frames < 2:
        raise RuntimeError(f"--num_frames must at least 2, but got {num_frames}.")
    if args.params_init == 'random':
        from scipy.spatial.transform import Rotation
        rng = np.random.default_rng(args.random_seed)
        dataset.camera_trajectory[:, :4] = Rotation.random(len(dataset), random_state=args.random_seed).as_quat()
        dataset.camera_trajectory[:, 4:] = rng.normal(loc=0., scale=.1, size=(len(dataset), 3))
    optimiser = PoseOptimiser(dataset, feature_extraction_options=FeatureExtractionOptions(min_features=40, max_features=2048),
                              optimisation_options=OptimisationOptions(num_epochs=20000, learning_rate=1e-2, lr_scheduler_patience=50))
    camera_trajectory, _, _ = optimiser.run(num_frames)
    if optimiser.debug_path:
        from hive_amd.fusion import tsdf_fusion
        from hive_amd.options import BackgroundMeshOptions, MeshReconstructionMethod
        reconstruction_options = BackgroundMeshOptions(reconstruction_method=MeshReconstructionMethod.TSDFFusion, sdf_max_voxels=80000000)
        logging.info("Running TSDFFusion on initial pose data...")
        tsdf_fusion(dataset, options=reconstruction_options, num_frames=num_frames).export(os.path.join(optimiser.debug_path, 'before.ply'))
        dataset.camera_trajectory = camera_trajectory
        logging.info("Running TSDFFusion on final pose data..")
        tsdf_fusion(dataset, options=reconstruction_options, num_frames=num_frames).export(os.path.join(optimiser.debug_path, 'after.ply'))


if __name__ == '__main__':
    main()
