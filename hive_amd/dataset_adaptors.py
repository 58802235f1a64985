"""Dataset adaptors: the API surface of /root/reference/hive/dataset_adaptors.py for the inputs of the hot
path.  ``TUMAdaptor`` (RGB-D + ground-truth poses, BASELINE.json config 1) is implemented; ``UnrealAdaptor``,
``VideoAdaptor`` and ``StrayScannerAdaptor`` (dataset_adaptors.py:769, 1023, 1158) need COLMAP / ffmpeg / capture
formats that are outside the dense-compute scope ("KEEP API, no logic"): their names, folder
checks and constructor signatures are here so that ``from hive.dataset_adaptors import ...`` lines and ``get_dataset``'s
dispatch keep working, and ``convert`` says what is missing instead of doing the work.
``estimate_depth_dpt`` is re-exported from ``hive_amd.depth``.
"""
import enum
import logging
import os
import shutil
import warnings
from os.path import join as pjoin

import numpy as np
from PIL import Image
from scipy.spatial.transform import Rotation

from hive_amd.depth import estimate_depth_dpt  # noqa: F401  (reference location: dataset_adaptors.py:1346)
from hive_amd.geometric import Trajectory
from hive_amd.io import DatasetMetadata, HiveDataset, ImageFolderDataset
from hive_amd.options import BackgroundMeshOptions, COLMAPOptions, InpaintingMode, PipelineOptions, StorageOptions
from hive_amd.utils import timed_block


class DatasetAdaptor:
    """Base of the converters to the HIVE format (dataset_adaptors.py:57-572): ``convert()`` writes the HIVE folder."""
    required_files: list = []
    required_folders: list = []

    def __init__(self, base_path, output_path, num_frames=-1, frame_step=1, colmap_options=None):
        self.base_path, self.output_path = str(base_path), str(output_path)
        self.num_frames, self.frame_step = num_frames, frame_step
        self.colmap_options = colmap_options or COLMAPOptions()

    @classmethod
    def is_valid_folder_structure(cls, path) -> bool:
        path = str(path)
        return (os.path.isdir(path) and all(os.path.isfile(pjoin(path, f)) for f in cls.required_files)
                and all(os.path.isdir(pjoin(path, f)) for f in cls.required_folders))

    def convert(self, estimate_pose, estimate_depth, inpainting_mode=InpaintingMode.Off, static_camera=False, no_cache=False, profiling=None, png_encoder="host"):
        raise NotImplementedError(f"{type(self).__name__}.convert: this capture format needs stages outside the dense-compute path of "
                                  f"this build (COLMAP / ffmpeg / capture-specific decoding, SURVEY.md section 2 row 11); convert the "
                                  f"sequence with the reference and open the resulting HIVE folder, or use a TUM-layout folder")

    def _inpaint_frame_data(self, mode: InpaintingMode, png_encoder="host"):
        """Inpaints the RGB frames, depth maps and masks of the converted folder and writes them to disk (dataset_adaptors.py:473-571)."""
        inpaint_frame_data(self.output_path, mode, png_encoder=png_encoder)


class TUMAdaptor(DatasetAdaptor):
    """Converts a TUM RGB-D sequence (rgb.txt, depth.txt, groundtruth.txt, rgb/, depth/) to the HIVE format
    (dataset_adaptors.py:573-760): frames are associated by nearest timestamp per depth map, the cam-to-world
    ground-truth poses are re-based (``normalise_position``), inverted to world-to-camera and rotated -90 degrees
    about x; depth PNGs (1/5000 m units) are rewritten in millimetres."""
    fx, fy, cx, cy = 580.0, 580.0, 319.5, 239.5
    width, height = 640, 480
    intrinsic_matrix = np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])
    fps = 30.0
    pose_path, rgb_files_path, depth_map_files_path = "groundtruth.txt", "rgb.txt", "depth.txt"
    required_files = [pose_path, rgb_files_path, depth_map_files_path]
    rgb_folder, depth_folder = "rgb", "depth"
    required_folders = [rgb_folder, depth_folder]

    def __init__(self, base_path, output_path, num_frames=-1, frame_step=1, is_16_bit=True, colmap_options=None):
        self.base_path, self.output_path = str(base_path), str(output_path)
        self.colmap_options = colmap_options or COLMAPOptions()
        for name in self.required_files:
            if not os.path.isfile(pjoin(self.base_path, name)):
                raise RuntimeError(f"The TUM dataset {self.base_path} is missing the file {name}.")
        for name in self.required_folders:
            if not os.path.isdir(pjoin(self.base_path, name)):
                raise RuntimeError(f"The TUM dataset {self.base_path} is missing the folder {name}.")
        self.frame_step = frame_step
        self.depth_scale_factor = 1.0 / 5000.0 if is_16_bit else 1.0
        self.image_filenames, self.depth_filenames, trajectory = self._get_synced_frame_data()
        full = len(self.image_filenames)
        self.num_frames = full if num_frames == -1 or num_frames > full else num_frames
        trajectory = trajectory.normalise_position().inverse()
        rotation = np.eye(4)
        rotation[:3, :3] = Rotation.from_euler('xyz', [-90, 0, 0], degrees=True).as_matrix()
        self.camera_trajectory = trajectory.apply(rotation)

    @staticmethod
    def _load_list(path):
        stamps, data = [], []
        with open(path, 'r') as f:
            for line in f:
                line = line.strip()
                if not line or line.startswith('#'):
                    continue
                parts = line.split(' ')
                stamps.append(float(parts[0]))
                data.append(parts[1:])
        return np.array(stamps), data

    def _get_synced_frame_data(self):
        image_t, image_paths = self._load_list(pjoin(self.base_path, self.rgb_files_path))
        depth_t, depth_paths = self._load_list(pjoin(self.base_path, self.depth_map_files_path))
        pose_t, poses = self._load_list(pjoin(self.base_path, self.pose_path))

        def closest(query, target):  # index of the closest query timestamp for every target timestamp
            return np.abs(query.reshape(-1, 1) - target.reshape(1, -1)).argmin(axis=0)

        images = [image_paths[i][0][len("rgb/"):] for i in closest(image_t, depth_t)]
        depths = [p[0][len("depth/"):] for p in depth_paths]
        rows = []
        for i in closest(pose_t, depth_t):
            tx, ty, tz, qx, qy, qz, qw = map(float, poses[i])
            rows.append((qx, qy, qz, qw, tx, ty, tz))
        return images, depths, Trajectory(np.array(rows))

    def get_metadata(self, estimate_pose=False, estimate_depth=False) -> DatasetMetadata:
        return DatasetMetadata(num_frames=self.num_frames, frame_step=self.frame_step, fps=self.fps, width=self.width, height=self.height,
                               estimate_pose=estimate_pose, estimate_depth=estimate_depth,
                               depth_mask_dilation_iterations=BackgroundMeshOptions().depth_mask_dilation_iterations,
                               depth_scale=HiveDataset.depth_scaling_factor)

    def depth_to_mm(self, raw):
        """TUM depth PNG values -> uint16 millimetres, in the reference's operation order (dataset_adaptors.py:762-764:
        metres first, then x 1000, then truncation) -- dividing by the two scale factors in one step rounds differently
        and is off by one millimetre for 41 of the 65536 raw values."""
        depth_map = np.asarray(raw) * self.depth_scale_factor  # convert to metres from non-standard scale & units.
        return (1000 * depth_map).astype(np.uint16)  # convert to mm from metres.

    def convert(self, estimate_pose=False, estimate_depth=False, inpainting_mode=InpaintingMode.Off, static_camera=False, no_cache=False,
                profiling=None, png_encoder="host", segment_motion=False) -> HiveDataset:
        """Write the HIVE-format folder and return it as a ``HiveDataset`` (dataset_adaptors.py:176-266).
        The reference's instance masks come from detectron2 (out of scope).  By default empty masks are written, i.e. a static scene.  ``segment_motion=True``
        (or a ``segmentation.MotionSegmentationOptions``) replaces them, once the trajectory is final and before any inpainting, by
        ``segmentation.segment_dataset``'s: what moved against the fused static model -- a rule of this project, not Mask R-CNN; it needs the sensor depth.
        ``estimate_depth=True`` replaces the sensor depth by DPT-Hybrid estimates (needs the weights file).  ``png_encoder`` ("host" | "gpu") goes to
        ``estimate_depth_dpt`` and ``inpaint_frame_data``; the frames copied here are always written by the host encoder.
        ``estimate_pose=True`` (with the sensor depth): the reference runs COLMAP, which is absent; here the folder is written as usual and
        ``registration.estimate_trajectory`` (SIFT matches back-projected with the depth, a rigid RANSAC per hierarchical frame pair, the transforms chained) on
        it replaces the ground-truth file's trajectory, anchored at that file's first pose; frames that no chain of pairs reached are warned about.  Together
        with ``estimate_depth=True`` it raises: per-frame depth scales would have to be applied before fusion."""
        if estimate_pose and estimate_depth:
            raise NotImplementedError("pose estimation on estimated depth: the per-frame depth scales of the registration would have to be applied before fusion; "
                                      "COLMAP, which the reference runs here, is outside the dense-compute scope")
        if static_camera:
            raise NotImplementedError("the static-camera override is outside the dense-compute scope")
        if segment_motion and estimate_depth:
            raise NotImplementedError("motion segmentation on estimated depth: the per-frame scale of an estimated depth map makes its difference to the model "
                                      "meaningless; use the sensor depth")
        _check_inpainting_mode(inpainting_mode)
        out = self.output_path
        if no_cache and os.path.isdir(out):
            shutil.rmtree(out)
        os.makedirs(out, exist_ok=True)
        for folder in HiveDataset.required_folders:
            os.makedirs(pjoin(out, folder), exist_ok=True)
        self.get_metadata(estimate_pose, estimate_depth).save(pjoin(out, HiveDataset.metadata_filename))
        logging.info("Copying frames...")
        for i in range(self.num_frames):
            name = HiveDataset.index_to_filename(i)
            Image.open(pjoin(self.base_path, self.rgb_folder, self.image_filenames[i])).convert('RGB').save(pjoin(out, "rgb", name))
            Image.fromarray(np.zeros((self.height, self.width), np.uint8)).save(pjoin(out, "mask", name))
            if not estimate_depth:
                raw = np.asarray(Image.open(pjoin(self.base_path, self.depth_folder, self.depth_filenames[i])))
                depth_mm = self.depth_to_mm(raw)
                Image.fromarray(depth_mm).save(pjoin(out, "depth", name))  # uint16 -> 16-bit PNG
        if estimate_depth:
            estimate_depth_dpt(ImageFolderDataset(pjoin(out, "rgb")), pjoin(out, "depth"), png_encoder=png_encoder)
        np.savetxt(pjoin(out, HiveDataset.camera_matrix_filename), self.intrinsic_matrix)
        Trajectory(self.camera_trajectory.values[:self.num_frames]).save(pjoin(out, HiveDataset.camera_trajectory_filename))
        if estimate_pose:
            from hive_amd import registration
            logging.info("Estimating the camera trajectory from the frames...")
            estimate = registration.estimate_trajectory(HiveDataset(out))
            if estimate.lost:
                warnings.warn(f"pose estimation: no chain of frame pairs reached the frames {estimate.lost}; each copies the pose of a neighbour")
            estimate.trajectory.save(pjoin(out, HiveDataset.camera_trajectory_filename))
        if segment_motion:
            from hive_amd import segmentation
            logging.info("Segmenting what moved against the static model...")
            options = segment_motion if isinstance(segment_motion, segmentation.MotionSegmentationOptions) else None
            segmentation.segment_dataset(HiveDataset(out), options, png_encoder=png_encoder)
        with timed_block("Inpainted the frame data in", profiling, ('timing', 'load_dataset', 'inpainting')):  # (dataset_adaptors.py:261-262)
            self._inpaint_frame_data(mode=inpainting_mode, png_encoder=png_encoder)
        return HiveDataset(out)


class UnrealAdaptor(DatasetAdaptor):
    """Unreal Engine captures (dataset_adaptors.py:769-851): API only."""
    metadata_filename, camera_matrix_filename, camera_trajectory_filename = "info.json", "camera.txt", "trajectory.txt"
    required_files = [metadata_filename, camera_matrix_filename, camera_trajectory_filename]
    rgb_folder, depth_folder = "colour", "depth"
    required_folders = [rgb_folder, depth_folder]


class VideoAdaptorBase(DatasetAdaptor):
    """Common part of the adaptors that read frames from a video file (dataset_adaptors.py:854-1020): API only."""

    def __init__(self, base_path, output_path, video_path, num_frames=-1, frame_step=1, colmap_options=None, resize_to=640):
        super().__init__(base_path, output_path, num_frames=num_frames, frame_step=frame_step, colmap_options=colmap_options)
        self.video_path, self.resize_to = str(video_path), resize_to


class VideoAdaptor(VideoAdaptorBase):
    """A plain video file (poses from COLMAP, depth from DPT; dataset_adaptors.py:1023-1091): API only."""

    def __init__(self, base_path, output_path, num_frames=-1, frame_step=1, colmap_options=None, resize_to=640):
        path = str(base_path)
        super().__init__(os.path.dirname(path), output_path, video_path=path, num_frames=num_frames, frame_step=frame_step, colmap_options=colmap_options,
                         resize_to=resize_to)

    @classmethod
    def is_valid_folder_structure(cls, path) -> bool:
        path = str(path)
        return os.path.isfile(path) and os.path.splitext(path)[1] == ".mp4"  # (dataset_adaptors.py:1059)


class DeviceOrientation(enum.Enum):
    """How a StrayScanner capture was held (dataset_adaptors.py:1094-1155)."""
    Landscape = enum.auto()
    Portrait = enum.auto()
    LandscapeReverse = enum.auto()
    PortraitReverse = enum.auto()


class StrayScannerAdaptor(VideoAdaptorBase):
    """iOS StrayScanner captures (LiDAR depth + ARKit odometry; dataset_adaptors.py:1158-1335): API only."""
    video_filename, camera_matrix_filename, camera_trajectory_filename = "rgb.mp4", "camera_matrix.csv", "odometry.csv"
    required_files = [video_filename, camera_matrix_filename, camera_trajectory_filename]
    depth_folder, confidence_map_folder = "depth", "confidence"
    required_folders = [depth_folder, confidence_map_folder]

    def __init__(self, base_path, output_path, num_frames=-1, frame_step=1, colmap_options=None, resize_to=640, depth_confidence_filter_level=0,
                 fix_orientation=True):
        super().__init__(base_path, output_path, video_path=pjoin(str(base_path), self.video_filename), num_frames=num_frames, frame_step=frame_step,
                         colmap_options=colmap_options, resize_to=resize_to)
        self.depth_confidence_filter_level, self.fix_orientation = depth_confidence_filter_level, fix_orientation


INPAINTING_MASK_DILATION = (5, 5, 5)  # `cv2.dilate(mask, np.ones((5, 5)), iterations=5)` (dataset_adaptors.py:501-503)
INPAINTING_RADIUS = 30                # `cv2.inpaint(image, mask, 30, cv2.INPAINT_TELEA)` (:510)


def _check_inpainting_mode(mode: InpaintingMode):
    if mode & (InpaintingMode.Lama_Image | InpaintingMode.Lama_Depth):
        raise NotImplementedError(f"inpainting mode {mode.name}: LaMa is a third-party network outside this build; use CV2_Image_Depth "
                                  f"(--inpainting_mode 1), or inpaint the frames with the reference and open the resulting HIVE folder")
    if mode != InpaintingMode.Off and mode != InpaintingMode.CV2_Image_Depth:
        raise RuntimeError(f"The inpainting mode must either be {InpaintingMode.Off} or specify an image and a depth inpainting method, got {mode}.")


def _write_png(path, array):
    Image.fromarray(array).save(path)  # uint8 [H][W] / [H][W][3] -> 8-bit PNG, uint16 [H][W] -> 16-bit PNG


def inpaint_frame_data(dataset_path, mode: InpaintingMode, ctx=None, batch_size=32, png_encoder="host"):
    """``DatasetAdaptor._inpaint_frame_data`` (dataset_adaptors.py:473-571) on a HIVE-format folder: the instance masks are dilated with a 5 x 5
    element five times, colour and depth are filled under them (radius 30) and written to ``rgb_inpainted/`` and ``depth_inpainted/`` under the
    file names and bit depths of ``rgb/`` and ``depth/``; ``mask_inpainted/`` gets an all-zero mask per frame (the background then has no
    dynamic object left to mask, :536-539, :570-571).

    ``Off`` does nothing; ``CV2_Image_Depth`` runs Telea's method on the GPU, ``batch_size`` frames per call, in the level order that
    ``hive_inpaint_telea`` states (not cv2's heap order: INTEGRATION.md); the three modes with LaMa raise ``NotImplementedError``.  The PNG
    files of a batch are written by a thread pool while the GPU fills the next one.  ``png_encoder="gpu"``: the three files of every frame of a batch are
    compressed on the device in one ``hive_amd.png.encode`` call (same pixels, the device encoder's bytes) and the pool only writes them; the default
    ``"host"`` is Pillow, as before."""
    from hive_amd import png
    png.check_encoder(png_encoder)
    mode = InpaintingMode(mode)
    if mode == InpaintingMode.Off:
        return
    _check_inpainting_mode(mode)
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from hive_amd.image_processing import inpaint_frames
    from hive_amd.utils import usable_cores
    logging.info("Creating inpainted frame data.")
    dataset_path = str(dataset_path)
    folders = {}
    for name in (HiveDataset.rgb_folder, HiveDataset.depth_folder, HiveDataset.mask_folder):
        folders[name] = ImageFolderDataset(pjoin(dataset_path, name))
    rgb_set, depth_set, mask_set = (folders[name] for name in (HiveDataset.rgb_folder, HiveDataset.depth_folder, HiveDataset.mask_folder))
    if not len(rgb_set) == len(depth_set) == len(mask_set):
        raise RuntimeError(f"{dataset_path}: {len(rgb_set)} colour frames, {len(depth_set)} depth maps and {len(mask_set)} masks")
    out_rgb, out_depth, out_mask = (pjoin(dataset_path, name) for name in (HiveDataset.inpainted_rgb_folder, HiveDataset.inpainted_depth_folder,
                                                                           HiveDataset.inpainted_mask_folder))
    for folder in (out_rgb, out_depth, out_mask):
        os.makedirs(folder, exist_ok=True)
    n = len(rgb_set)
    device = torch.device("cuda", ctx.device if ctx is not None else torch.cuda.current_device())
    writers = ThreadPoolExecutor(max_workers=max(1, min(32, usable_cores() - 1)))
    pending = []
    try:
        for start in range(0, n, batch_size):
            index = range(start, min(n, start + batch_size))
            rgb = np.stack([np.asarray(rgb_set[i]) for i in index])
            depth = np.stack([np.asarray(depth_set[i]) for i in index])
            mask = np.stack([np.asarray(mask_set[i]) for i in index])
            if mask.ndim == 4:  # a mask stored as a colour image: any channel marks the object
                mask = mask.max(axis=3)
            if depth.dtype != np.uint16 or rgb.dtype != np.uint8 or rgb.ndim != 4:
                raise RuntimeError(f"{dataset_path}: expected 8-bit colour frames and 16-bit depth maps, got {rgb.dtype} {rgb.shape} and {depth.dtype}")
            filled_rgb, filled_depth = inpaint_frames(torch.from_numpy(rgb).to(device), torch.from_numpy(depth).to(device),
                                                      torch.from_numpy(np.ascontiguousarray(mask != 0, dtype=np.uint8)).to(device),
                                                      dilation=INPAINTING_MASK_DILATION, radius=INPAINTING_RADIUS, ctx=ctx)
            if png_encoder == "gpu":
                black = torch.zeros(mask.shape[1:], dtype=torch.uint8, device=device)
                files = png.encode([picture for j in range(len(index)) for picture in (filled_rgb[j], filled_depth[j].view(torch.uint16), black)], ctx=ctx)
                names = [pjoin(folder, names.image_filenames[i]) for i in index for folder, names in ((out_rgb, rgb_set), (out_depth, depth_set), (out_mask, mask_set))]
                for done in pending:
                    done.result()
                pending = [writers.submit(png.write_file, name, data) for name, data in zip(names, files)]
                continue
            filled_rgb, filled_depth = filled_rgb.cpu().numpy(), filled_depth.cpu().numpy()
            for done in pending:  # at most two batches of files in flight
                done.result()
            pending = []
            black = np.zeros(mask.shape[1:], np.uint8)
            for j, i in enumerate(index):
                pending.append(writers.submit(_write_png, pjoin(out_rgb, rgb_set.image_filenames[i]), filled_rgb[j]))
                pending.append(writers.submit(_write_png, pjoin(out_depth, depth_set.image_filenames[i]), filled_depth[j]))
                pending.append(writers.submit(_write_png, pjoin(out_mask, mask_set.image_filenames[i]), black))
        for done in pending:
            done.result()
    finally:
        writers.shutdown(wait=True)


def _open_hive_folder(path, inpainting_mode, profiling=None, png_encoder="host") -> HiveDataset:
    """A HIVE folder as it is; with an inpainting mode and no inpainted frames yet, those are made first (the masks come with the folder)."""
    dataset = HiveDataset(path)
    if inpainting_mode != InpaintingMode.Off and not dataset.has_inpainted_frame_data:
        with timed_block("Inpainted the frame data in", profiling, ('timing', 'load_dataset', 'inpainting')):
            inpaint_frame_data(path, inpainting_mode, png_encoder=png_encoder)
        dataset = HiveDataset(path)
    return dataset


def get_dataset(storage_options, colmap_options=None, pipeline_options=None, resize_to=640, depth_confidence_filter_level=0, profiling=None,
                **legacy) -> HiveDataset:
    """Open a HIVE dataset, converting it first if it is in another format (dataset_adaptors.py:1438-1498).

    Reference form: ``get_dataset(storage_options: StorageOptions, colmap_options, pipeline_options, resize_to, ...)``.  The
    shorthand of this build's earlier rounds still works: ``get_dataset(dataset_path, output_path, num_frames=-1, frame_step=1,
    estimate_depth=False, no_cache=False)``."""
    if not isinstance(storage_options, StorageOptions):  # shorthand: (dataset_path, output_path, ...)
        output_path = legacy.pop("output_path", colmap_options)
        pipeline_options = PipelineOptions(num_frames=legacy.pop("num_frames", -1), frame_step=legacy.pop("frame_step", 1),
                                           estimate_depth=legacy.pop("estimate_depth", False))
        storage_options = StorageOptions(dataset_path=storage_options, output_path=output_path, no_cache=legacy.pop("no_cache", False))
        colmap_options = None
        if HiveDataset.is_valid_folder_structure(storage_options.dataset_path):  # (the shorthand opens a HIVE folder in place)
            return HiveDataset(storage_options.dataset_path)
    assert not legacy, f"get_dataset: unexpected arguments {sorted(legacy)}"
    colmap_options = colmap_options or COLMAPOptions()
    pipeline_options = pipeline_options or PipelineOptions()
    dataset_path, output_path = str(storage_options.dataset_path), str(storage_options.output_path)
    if not storage_options.no_cache and HiveDataset.is_valid_folder_structure(output_path):
        return _open_hive_folder(output_path, pipeline_options.inpainting_mode, profiling, pipeline_options.png_encoder)
    base = dict(base_path=dataset_path, output_path=output_path, num_frames=pipeline_options.num_frames, frame_step=pipeline_options.frame_step,
                colmap_options=colmap_options)
    if HiveDataset.is_valid_folder_structure(dataset_path):
        return _open_hive_folder(dataset_path, pipeline_options.inpainting_mode, profiling, pipeline_options.png_encoder)
    if TUMAdaptor.is_valid_folder_structure(dataset_path):
        converter = TUMAdaptor(**base)
    elif UnrealAdaptor.is_valid_folder_structure(dataset_path):
        converter = UnrealAdaptor(**base)
    elif StrayScannerAdaptor.is_valid_folder_structure(dataset_path):
        converter = StrayScannerAdaptor(**base, resize_to=resize_to, depth_confidence_filter_level=depth_confidence_filter_level,
                                        fix_orientation=not pipeline_options.estimate_pose)
    elif VideoAdaptor.is_valid_folder_structure(dataset_path):
        converter = VideoAdaptor(resize_to=resize_to, **base)
    elif not os.path.isdir(dataset_path):
        raise RuntimeError(f"Could not open the path {dataset_path} or it is not a folder.")
    else:
        raise RuntimeError(f"Could not recognise the dataset format for the dataset at {dataset_path}.")
    return converter.convert(estimate_pose=pipeline_options.estimate_pose, estimate_depth=pipeline_options.estimate_depth,
                             inpainting_mode=pipeline_options.inpainting_mode, static_camera=pipeline_options.static_camera,
                             no_cache=storage_options.no_cache, profiling=profiling, png_encoder=pipeline_options.png_encoder)
