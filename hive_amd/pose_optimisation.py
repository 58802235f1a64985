"""Foreground trajectory smoothing (``--fts_num_epochs N``): ``ForegroundPoseOptimiser`` of hive/pose_optimisation.py:1618-1711 on the MI355X.

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
