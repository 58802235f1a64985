"""HIVE's pipeline for the part the dense-compute path serves: dataset -> key frames -> TSDF fusion -> background mesh
(/root/reference/hive/pipeline.py:258-286, 871-901), then the per-frame foreground meshes (``_create_scene``, :309-497) with the
connected-component clean-up and, on request, decimation, billboards and trajectory smoothing.

Meshes are written as PLY.  On request (``run(export_gltf=True)`` / ``--export_gltf``) the reference's last stages follow (:213-237, :902-1158): the two
scenes are centred (``_center_scenes``), written as ``mesh/fg.glb`` and ``mesh/bg.glb`` (hive_amd/gltf.py: packed on the device, csrc/gltf.hip) with
``mesh/metadata.json``, and copied to the player's folder (``_export_video_webxr``).  Where the reference compresses with draco_transcoder the files are
written quantised (KHR_mesh_quantization).  Draco itself and the WebXR server of the reference's ``Pipeline`` stay outside the scope of this build
(SURVEY.md §2 row 10), as do the oriented bounds of ``align_scene`` (trimesh's).
"""
import argparse
import json
import logging
import os
import shutil
from pathlib import Path
from typing import Optional

import numpy as np

from hive_amd import foreground, fusion, gltf
from hive_amd.dataset_adaptors import get_dataset
from hive_amd.io import HiveDataset
from hive_amd.options import (BackgroundMeshOptions, COLMAPOptions, ForegroundTrajectorySmoothingOptions, MaskDilationOptions, MeshDecimationOptions,
                              MeshFilteringOptions, MeshReconstructionMethod, PipelineOptions, StorageOptions, WebXROptions)
from hive_amd.utils import set_key_path, timed_block


def write_ply(path, vertices, faces, vertex_colors=None, vertex_normals=None, *, vertex_uv=None, texture_file=None):
    """Binary little-endian PLY (trimesh, which the reference exports glb with, is not a dependency here).  ``vertex_uv`` (V, 2) adds float
    ``texture_u`` / ``texture_v`` vertex properties and ``texture_file`` a ``comment TextureFile <name>`` header line (the form MeshLab reads)."""
    vertices = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int32)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if vertex_normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if vertex_colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if vertex_uv is not None:
        fields += [("texture_u", "<f4"), ("texture_v", "<f4")]
    v = np.empty(len(vertices), dtype=fields)
    v["x"], v["y"], v["z"] = vertices.T
    if vertex_normals is not None:
        v["nx"], v["ny"], v["nz"] = np.asarray(vertex_normals, np.float32).T
    if vertex_colors is not None:
        c = np.asarray(vertex_colors)
        v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
    if vertex_uv is not None:
        uv = np.asarray(vertex_uv, np.float32)
        v["texture_u"], v["texture_v"] = uv[:, 0], uv[:, 1]
    f = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    f["n"], f["i"] = 3, faces
    names = {"<f4": "float", "u1": "uchar"}
    with open(path, "wb") as out:
        header = ["ply", "format binary_little_endian 1.0"]
        if texture_file is not None:
            header += [f"comment TextureFile {texture_file}"]
        header += [f"element vertex {len(v)}"]
        header += [f"property {names[t]} {n}" for n, t in fields]
        header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
        out.write(("\n".join(header) + "\n").encode())
        out.write(v.tobytes())
        out.write(f.tobytes())


class Pipeline:
    """The reference's ``Pipeline`` (/root/reference/hive/pipeline.py:59-262) for the part this build serves: dataset -> key frames
    -> TSDF fusion -> background mesh -> per-frame foreground meshes.  Constructor, ``from_command_line`` and ``run`` take the reference's
    arguments; the foreground path does what the reference's does, and with ``export_gltf`` the scenes are centred, written as glTF and exported to the player's
    folder (``_center_scenes`` .. ``_export_video_webxr`` below); draco and the WebXR server are outside this build's scope."""
    mesh_folder = "mesh"
    bundle_fusion_folder = "bundle_fusion"

    def __init__(self, options: Optional[PipelineOptions] = None, storage_options: Optional[StorageOptions] = None, decimation_options=None,
                 dilation_options=None, filtering_options=None, colmap_options=None, static_mesh_options: Optional[BackgroundMeshOptions] = None,
                 webxr_options=None, fts_options=None, *, background_mesh_options: Optional[BackgroundMeshOptions] = None, num_frames=None):
        """Reference form (pipeline.py:67-99): ``Pipeline(options, storage_options, decimation_options, dilation_options,
        filtering_options, colmap_options, static_mesh_options, webxr_options, fts_options)``.  The keyword shorthand of this
        build's earlier rounds -- ``Pipeline(background_mesh_options=..., num_frames=...)`` -- still works."""
        self.options = options or PipelineOptions()
        if num_frames is not None:
            self.options.num_frames = num_frames
        self.storage_options = storage_options
        self.decimation_options = decimation_options or MeshDecimationOptions()
        self.dilation_options = dilation_options or MaskDilationOptions()
        self.filtering_options = filtering_options or MeshFilteringOptions()
        self.colmap_options = colmap_options or COLMAPOptions()
        self.background_mesh_options = static_mesh_options or background_mesh_options or BackgroundMeshOptions()
        self.webxr_options = webxr_options or WebXROptions()
        self.fts_options = fts_options or ForegroundTrajectorySmoothingOptions()
        self.profiling = {}

    @staticmethod
    def from_command_line(argv=None) -> 'Pipeline':
        """pipeline.py:100-141: every option group registers its flags on one parser; ``argv=None`` reads ``sys.argv``.  (The reference leaves the trajectory
        smoothing group out of its parser, so its ``--fts_*`` flags can only be set from code; here they are registered like the others.)"""
        parser = argparse.ArgumentParser("HIVE", description="Create 3D mesh videos from a RGB-D sequence with camera trajectory annotations.")
        groups = (PipelineOptions, StorageOptions, MaskDilationOptions, MeshFilteringOptions, MeshDecimationOptions, COLMAPOptions, BackgroundMeshOptions,
                  WebXROptions, ForegroundTrajectorySmoothingOptions)
        for group in groups:
            group.add_args(parser)
        args = parser.parse_args(argv)
        logging.debug(args)
        return Pipeline(options=PipelineOptions.from_args(args), storage_options=StorageOptions.from_args(args),
                        decimation_options=MeshDecimationOptions.from_args(args), dilation_options=MaskDilationOptions.from_args(args),
                        filtering_options=MeshFilteringOptions.from_args(args), colmap_options=COLMAPOptions.from_args(args),
                        static_mesh_options=BackgroundMeshOptions.from_args(args), webxr_options=WebXROptions.from_args(args),
                        fts_options=ForegroundTrajectorySmoothingOptions.from_args(args))

    @property
    def num_frames(self) -> int:
        return self.options.num_frames

    @property
    def estimate_pose(self) -> bool:
        return self.options.estimate_pose

    @property
    def estimate_depth(self) -> bool:
        return self.options.estimate_depth

    @property
    def mesh_path(self) -> str:
        return os.path.join(self.storage_options.output_path, self.mesh_folder)

    @staticmethod
    def create_static_mesh(dataset: HiveDataset, num_frames=-1, options: Optional[BackgroundMeshOptions] = None, frame_set=None):
        """pipeline.py:871-901: key frames (unless a frame set is given), then TSDF fusion."""
        options = options or BackgroundMeshOptions()
        if num_frames < 1:
            num_frames = dataset.num_frames
        if options.reconstruction_method != MeshReconstructionMethod.TSDFFusion:
            raise NotImplementedError(f"{options.reconstruction_method.name}: only TSDFFusion is part of the dense-compute path")
        if frame_set is None:
            frame_set = dataset.select_key_frames(threshold=options.key_frame_threshold, frame_step=options.key_frame_step)
            frame_set = [f for f in frame_set if f < num_frames]
        logging.info(f"Creating background mesh from {len(frame_set)} key frames...")
        return fusion.tsdf_fusion(dataset, options, num_frames=num_frames, frame_set=frame_set)

    def create_foreground_meshes(self, dataset: HiveDataset, num_frames: int, folder: str, scene: Optional[gltf.Scene] = None):
        """``_create_foreground_scene`` / ``_create_scene`` (pipeline.py:288-497) for the dynamic objects of frames 0 .. num_frames - 1: every frame through
        ``foreground.process_frame`` with the connected-component clean-up on; a frame with a surviving object gives ``<folder>/%06d.ply`` (vertices in the frame of
        bg.ply, atlas uv) and ``<folder>/%06d.png`` (its texture atlas).  With ``decimation_options.enabled`` (``--enable_decimation``; off by default) every object is
        decimated before the clean-up and ``mesh_decimation`` profiling counts are recorded; with ``options.billboard`` (``--billboard``) every object is flattened to
        its median depth before texturing; with ``fts_options.num_epochs > 0`` (``--fts_num_epochs``) the meshes are built with the poses ``ForegroundPoseOptimiser``
        returns (:297-303) -- the dataset's stored trajectory, and with it bg.ply, stay as they are (the reference's ``temporary_trajectory``).  With a ``scene`` every
        frame's mesh joins it as it is made, on the device, under the node name ``%06d`` (:487)."""
        from PIL import Image
        not_applied = []
        decimation = self.decimation_options if self.decimation_options.enabled else None
        if self.decimation_options.num_faces_object > 0 and decimation is None:
            not_applied.append("decimation")
        self.profiling.setdefault("foreground_reconstruction", {})["not_applied"] = not_applied
        if not_applied:
            logging.info(f"Foreground meshes: {', '.join(not_applied)} requested without --enable_decimation, not applied.")
        os.makedirs(folder, exist_ok=True)
        trajectory = dataset.camera_trajectory
        if self.fts_options.num_epochs > 0:
            from hive_amd.pose_optimisation import ForegroundPoseOptimiser
            with timed_block("Smoothed the foreground trajectory in", self.profiling, ("timing", "foreground_reconstruction", "trajectory_smoothing")):
                trajectory = ForegroundPoseOptimiser(dataset, learning_rate=self.fts_options.learning_rate, num_epochs=self.fts_options.num_epochs).run()
        poses = trajectory.to_homogenous_transforms()
        buffers = None
        for i in range(num_frames):
            depth = dataset.depth_dataset[i]
            if buffers is None:
                buffers = foreground.FrameMeshBuffers(*depth.shape[:2])
            mesh = foreground.process_frame(dataset.rgb_dataset[i], depth, dataset.mask_dataset[i], dataset.camera_matrix, poses[i], self.dilation_options,
                                            self.filtering_options, disable_coverage_constraint=self.options.disable_coverage_constraint, buffers=buffers,
                                            enable_cc_analysis=True, decimation_options=decimation, billboard=bool(self.options.billboard))
            if mesh is None:
                continue
            for object_id, ((v0, f0), (v1, f1)) in mesh.get("decimation", {}).items():  # pipeline.py:418-427
                set_key_path(self.profiling, ["mesh_decimation", "vertex_count", "before", i, object_id], v0)
                set_key_path(self.profiling, ["mesh_decimation", "face_count", "before", i, object_id], f0)
                set_key_path(self.profiling, ["mesh_decimation", "vertex_count", "after", i, object_id], v1)
                set_key_path(self.profiling, ["mesh_decimation", "face_count", "after", i, object_id], f1)
            name = f"{i:06d}.png"
            Image.fromarray(mesh["texture"].cpu().numpy()).save(os.path.join(folder, name))
            write_ply(os.path.join(folder, f"{i:06d}.ply"), mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy(),
                      vertex_uv=mesh["uv"].cpu().numpy(), texture_file=name)
            if scene is not None:
                scene.add_geometry({key: mesh[key] for key in ("vertices", "faces", "uv", "texture")}, node_name=f"{i:06d}")

    # ------------------------------------------------------------------------------------------------ glTF export (pipeline.py:213-237, 902-1158)
    @staticmethod
    def _create_empty_scene(dataset: HiveDataset) -> gltf.Scene:
        """pipeline.py:636-648: an empty scene with the dataset's camera (resolution and focal lengths)."""
        K = np.asarray(dataset.camera_matrix)
        return gltf.Scene(camera=dict(resolution=(dataset.frame_width, dataset.frame_height), focal=(float(K[0, 0]), float(K[1, 1]))))

    def _create_background_scene(self, dataset: HiveDataset, static_mesh=None, num_frames: Optional[int] = None):
        """pipeline.py:258-286 for TSDFFusion: the static mesh under the node ``000000``.  Where the reference rewrites the vertex colours with
        ``(255 * (c / 255) ** 2.2).astype(int)`` (:281-282) the mesh stays as it is and the same table is returned as the ``lut`` the packer applies on the
        device.  Returns (scene, lut).  With ``options.texture_background`` the node is the mesh textured from the key frames (``_texture_background``) and
        there is no ``lut``: the 2.2-power table is for vertex colours, frames go in as they are, as the foreground's do."""
        if self.background_mesh_options.reconstruction_method != MeshReconstructionMethod.TSDFFusion:
            raise NotImplementedError(f"{self.background_mesh_options.reconstruction_method.name}: only TSDFFusion is part of the dense-compute path")
        scene = self._create_empty_scene(dataset)
        n = self.num_frames if num_frames is None else num_frames
        if static_mesh is None:
            static_mesh = self.create_static_mesh(dataset, num_frames=n, options=self.background_mesh_options)
        if self.options.texture_background:
            scene.add_geometry(self._texture_background(dataset, static_mesh, n), node_name="000000")
            return scene, None
        lut = (255 * np.power(np.arange(256) / 255, 2.2)).astype(np.uint8)
        scene.add_geometry(static_mesh, node_name="000000")
        return scene, lut

    def _texture_background(self, dataset: HiveDataset, static_mesh, num_frames: int) -> dict:
        """The static mesh with an atlas (``texturing.texture_mesh``) from the key frames the fusion used (``create_static_mesh``'s set; beyond
        ``options.texture_max_views`` every ceil(k / max)-th of them): the stored frames as they are (not the inpainted ones), without the pixels of the stored
        instance masks (non-zero), dilated with the run's ``MaskDilationOptions`` as the foreground's are.  ``profiling['background_texturing']`` gets the
        counts.  ``options.texture_smoothness`` and ``options.texture_cull_back_faces`` are passed on; when either is set the record gains ``smoothing``, the
        stats of the label smoothing.  ``options.texture_exposure``, ``options.texture_levelling`` and ``options.texture_levelling_sweeps`` are passed on too
        (``_texturing_record``); with all of them off the call and the export are what they were."""
        from hive_amd import texturing
        from hive_amd.image_processing import dilate_mask
        if num_frames is None or num_frames < 1:
            num_frames = dataset.num_frames
        options = self.background_mesh_options
        frame_set = [f for f in dataset.select_key_frames(threshold=options.key_frame_threshold, frame_step=options.key_frame_step) if f < num_frames]
        step = -(-len(frame_set) // max(1, int(self.options.texture_max_views)))
        frame_set = frame_set[::max(1, step)]
        with timed_block("Textured the background mesh in", self.profiling, ("timing", "background_reconstruction", "texturing")):
            frames = np.stack([np.asarray(dataset.rgb_dataset[i])[:, :, :3] for i in frame_set])
            masks = np.stack([dilate_mask(np.asarray(dataset.mask_dataset[i]) != 0, self.dilation_options) for i in frame_set])
            poses = np.asarray(dataset.camera_trajectory.to_homogenous_transforms(), np.float64)[frame_set]
            mesh = texturing.texture_mesh(static_mesh, frames, np.asarray(dataset.camera_matrix), poses, masks=masks, cell=self.options.texture_cell,
                                          return_views=True, smoothness=float(self.options.texture_smoothness),
                                          cull_back_faces=bool(self.options.texture_cull_back_faces), return_stats=True,
                                          exposure=bool(self.options.texture_exposure), levelling=bool(self.options.texture_levelling),
                                          levelling_sweeps=int(self.options.texture_levelling_sweeps))
        views, stats = mesh.pop("views"), mesh.pop("stats")
        self.profiling["background_texturing"] = self._texturing_record(frame_set, int(views.shape[0]), int((views >= 0).sum()), mesh["texture"].shape, stats,
                                                                        float(self.options.texture_smoothness) > 0 or bool(self.options.texture_cull_back_faces))
        return mesh

    @staticmethod
    def _texturing_record(frame_set, faces, faces_with_a_view, atlas_shape, stats, smoothing) -> dict:
        """``profiling['background_texturing']``: the counts; ``smoothing`` (the five label-smoothing stats) when ``--texture_smoothness`` or
        ``--texture_cull_back_faces`` is set; ``exposure`` (gains and pair counts as lists, fallback channels) with ``--texture_exposure``; ``levelling`` (seam
        vertices, sweeps, largest offset) with ``--texture_levelling``.  With every switch off: the four counts alone."""
        record = {"key_frames": [int(f) for f in frame_set], "faces": int(faces), "faces_with_a_view": int(faces_with_a_view),
                  "atlas": [int(atlas_shape[1]), int(atlas_shape[0])]}
        stats = dict(stats or {})
        exposure, levelling = stats.pop("exposure", None), stats.pop("levelling", None)
        if smoothing and stats:
            record["smoothing"] = stats
        if exposure is not None:
            record["exposure"] = {"gains": np.asarray(exposure["gains"]).tolist(), "pair_counts": np.asarray(exposure["pair_counts"]).tolist(),
                                  "fallback_channels": [int(c) for c in exposure["fallback_channels"]]}
        if levelling is not None:
            record["levelling"] = dict(levelling)
        return record

    def _create_foreground_scene(self, dataset: HiveDataset, num_frames: Optional[int] = None, folder: Optional[str] = None) -> gltf.Scene:
        """pipeline.py:288-307: an empty scene for ``background_only``, else every frame's mesh (``create_foreground_meshes``, which smooths the trajectory
        first when asked to); the PLY and PNG files go to ``folder`` (default ``<mesh_path>/fg``) as in a run without export."""
        scene = self._create_empty_scene(dataset)
        if not self.options.background_only:
            n = dataset.num_frames if num_frames is None else num_frames
            self.create_foreground_meshes(dataset, n, folder or os.path.join(self.mesh_path, "fg"), scene=scene)
        return scene

    @staticmethod
    def _get_scene_bounds(foreground_scene, background_scene):
        """pipeline.py:1084-1104: the joint (2, 3) bounds; a foreground scene without meshes has no bounds and contributes none."""
        fg_bounds, bg_bounds = foreground_scene.bounds, background_scene.bounds
        if fg_bounds is None:
            return bg_bounds
        return np.vstack([np.min(np.vstack((fg_bounds[0], bg_bounds[0])), axis=0), np.max(np.vstack((fg_bounds[1], bg_bounds[1])), axis=0)])

    def _center_scenes(self, dataset, foreground_scene, background_scene):
        """pipeline.py:982-1031 on copies of the scenes: turn them the right way up, then move them so that the joint bounds are centred in x and sit on y = 0 and
        z = 0.  Two stated choices: the turn by 180 degrees about z is exactly diag(-1, -1, 1, 1) (scipy's ``Rotation.from_euler('xyz', [0, 0, 180])`` has
        1.2e-16 where this has 0), and the offset is rounded to float32 as the reference's ``np.eye(4, dtype=np.float32)`` does.  ``align_scene`` needs trimesh's
        oriented bounds (:1006-1017) and raises."""
        if self.options.align_scene:
            raise NotImplementedError("align_scene: the oriented bounds of the background scene are trimesh's (trimesh.bounds.oriented_bounds), which this build does not have")
        foreground_scene, background_scene = foreground_scene.copy(), background_scene.copy()
        rotate_right_way_up = np.diag([-1.0, -1.0, 1.0, 1.0])
        foreground_scene.apply_transform(rotate_right_way_up)
        background_scene.apply_transform(rotate_right_way_up)
        scene_bounds = self._get_scene_bounds(foreground_scene, background_scene)
        scene_centroid = np.mean(scene_bounds, axis=0)
        translation = np.eye(4, dtype=np.float32)
        translation[:3, 3] = np.array([-scene_centroid[0], -scene_bounds[0, 1], -scene_bounds[0, 2]])
        foreground_scene.apply_transform(translation)
        background_scene.apply_transform(translation)
        return foreground_scene, background_scene

    @classmethod
    def _write_meshes_to_disk(cls, mesh_path: str, foreground_scene, background_scene, overwrite_ok=False, quantize=False, background_lut=None, texture_format="png",
                              jpeg_quality=90, png_encoder="host"):
        """pipeline.py:902-919 -> (path of fg.glb, path of bg.glb).  (The folder already holds this run's PLY files, so unlike the reference's it is made with
        ``exist_ok=True``; ``overwrite_ok`` guards the export folder, ``_export_video_webxr``.)"""
        os.makedirs(mesh_path, exist_ok=True)
        return (cls._write_mesh_to_disk(mesh_path, "fg", foreground_scene, quantize=quantize, texture_format=texture_format, jpeg_quality=jpeg_quality,
                                        png_encoder=png_encoder),
                cls._write_mesh_to_disk(mesh_path, "bg", background_scene, quantize=quantize, lut=background_lut, texture_format=texture_format, jpeg_quality=jpeg_quality,
                                        png_encoder=png_encoder))

    @classmethod
    def _write_mesh_to_disk(cls, base_folder: str, scene_name: str, scene, quantize=False, lut=None, texture_format="png", jpeg_quality=90, png_encoder="host") -> str:
        """pipeline.py:921-936: ``<base_folder>/<scene_name>.glb`` through ``gltf.write_glb``; the textures as ``options.texture_format`` says (PNG unless asked)."""
        output_path = os.path.join(base_folder, f"{scene_name}.glb")
        sizes = gltf.write_glb(output_path, scene, quantize=quantize, lut=lut, texture_format=texture_format, jpeg_quality=jpeg_quality, png_encoder=png_encoder)
        logging.info(f"Wrote mesh data to {output_path} ({sizes['total']} bytes)")
        return output_path

    def _compress_with_quantisation(self, path_to_glb: str, scene, lut=None):
        """Where the reference runs draco_transcoder over the file (:938-980): the scene is written again with KHR_mesh_quantization, the plain file is
        replaced, and ``profiling['mesh_compression'][foreground | background]`` gets the reference's four keys from the two file sizes.  The textures keep
        the plain file's format (``options.texture_format``)."""
        src_path = Path(path_to_glb)
        tmp_path = src_path.with_name(f"{src_path.stem}_tmp{src_path.suffix}")
        gltf.write_glb(str(tmp_path), scene, quantize=True, lut=lut, texture_format=self.options.texture_format, jpeg_quality=self.options.jpeg_quality,
                       png_encoder=self.options.png_encoder)
        size_before, size_after = os.path.getsize(src_path), os.path.getsize(tmp_path)
        shutil.move(str(tmp_path), str(src_path))
        name = {"fg": "foreground", "bg": "background"}.get(src_path.stem, src_path.stem)
        set_key_path(self.profiling, ["mesh_compression", name], {
            "uncompressed_file_size": size_before,
            "compressed_file_size": size_after,
            "data_saving": 1 - size_after / size_before,
            "compression_ratio": size_before / size_after,
        })

    @staticmethod
    def _get_dataset_name(dataset: HiveDataset) -> str:
        """pipeline.py:1106-1109: the dataset's folder name."""
        return Path(dataset.base_path).name

    def _get_webxr_metadata(self, dataset: HiveDataset, num_frames: Optional[int] = None) -> dict:
        """pipeline.py:1111-1125: the six keys of the player's metadata.json (a textured background, ``options.texture_background``, is not vertex-coloured)."""
        fy = float(np.asarray(dataset.camera_matrix)[1, 1])
        fov_y = float(np.rad2deg(2 * np.arctan2(dataset.frame_height, 2 * fy)))  # io.py:1025-1027
        return dict(fps=dataset.fps, fov_y=int(fov_y), num_frames=self.num_frames if num_frames is None else num_frames,
                    use_vertex_colour_for_bg=self.background_mesh_options.reconstruction_method != MeshReconstructionMethod.RGBD and
                    not self.options.texture_background,
                    add_ground_plane=self.webxr_options.webxr_add_ground_plane, add_sky_box=self.webxr_options.webxr_add_sky_box)

    def _export_video_webxr(self, mesh_path: str, fg_scene_name: str, bg_scene_name: str, metadata: dict, export_name: str) -> str:
        """pipeline.py:1127-1158: metadata.json beside the meshes, then the three files copied to ``<webxr_path>/<export_name>``; an export folder that exists
        raises FileExistsError unless ``storage_options.overwrite_ok``."""
        webxr_output_path = os.path.join(self.webxr_options.webxr_path, export_name)
        os.makedirs(webxr_output_path, exist_ok=bool(self.storage_options and self.storage_options.overwrite_ok))
        with open(os.path.join(mesh_path, "metadata.json"), "w") as f:
            json.dump(metadata, f)
        for filename in ("metadata.json", f"{fg_scene_name}.glb", f"{bg_scene_name}.glb"):
            shutil.copy(os.path.join(mesh_path, filename), os.path.join(webxr_output_path, filename))
        logging.info(f"Exported mesh data to: {webxr_output_path}")
        return webxr_output_path

    def run(self, dataset=None, adaptor=None, compress=True, *, estimate_depth=None, export_gltf=None):
        """pipeline.py:172-262: load (or convert) the dataset, fuse the static scene, write ``<output>/mesh/bg.ply`` (vertex colours in sRGB as
        pipeline.py:281-282), then -- unless ``background_only`` -- the foreground meshes of every frame (``create_foreground_meshes``: ``mesh/fg/``),
        and ``profiling.json``; returns the background mesh.

        Reference form: ``run(dataset: Optional[HiveDataset] = None, adaptor: Optional[DatasetAdaptor] = None, compress=True)`` with the
        paths in ``storage_options``.  Shorthand of earlier rounds: ``run(dataset_path, output_path, estimate_depth=False)``.

        ``export_gltf`` (default: ``options.export_gltf``, off): after the PLY files the scenes are centred and ``mesh/fg.glb``, ``mesh/bg.glb`` and
        ``mesh/metadata.json`` are written and copied to ``webxr_options.webxr_path/<dataset name>`` (:213-237); with ``compress`` the files are written
        quantised.  Off, a run writes nothing new."""
        if isinstance(dataset, (str, os.PathLike)):  # shorthand: run(dataset_path, output_path)
            self.storage_options = StorageOptions(dataset_path=str(dataset), output_path=str(adaptor))
            dataset = adaptor = None
        if estimate_depth is not None:
            self.options.estimate_depth = bool(estimate_depth)
        if self.storage_options is None and dataset is None and adaptor is None:
            raise ValueError("Pipeline.run needs storage_options (dataset_path, output_path), a dataset or an adaptor")
        with timed_block("Loaded dataset in", self.profiling, ("timing", "load_dataset", "total")):
            if adaptor is not None:
                dataset = adaptor.convert(estimate_pose=self.estimate_pose, estimate_depth=self.estimate_depth, inpainting_mode=self.options.inpainting_mode,
                                          static_camera=self.options.static_camera, no_cache=bool(self.storage_options and self.storage_options.no_cache),
                                          profiling=self.profiling, png_encoder=self.options.png_encoder)
            elif dataset is None:
                resize_to = None if self.options.disable_scaling else 640
                dataset = get_dataset(self.storage_options, self.colmap_options, self.options, resize_to=resize_to, profiling=self.profiling)
            n = dataset.num_frames if self.num_frames == -1 else min(self.num_frames, dataset.num_frames)
        with timed_block("Created background mesh in", self.profiling, ("timing", "background_reconstruction", "total")):
            mesh = self.create_static_mesh(dataset, num_frames=n, options=self.background_mesh_options)
        # vertex colours -> sRGB as pipeline.py:281-282
        colors = np.asarray(mesh.visual.vertex_colors)[:, :3]
        colors = (255 * np.power(colors / 255, 2.2)).astype(np.uint8)
        out = self.mesh_path if self.storage_options is not None else os.path.join(dataset.base_path, self.mesh_folder)
        os.makedirs(out, exist_ok=True)
        with timed_block("Wrote mesh data in", self.profiling, ("timing", "mesh_export")):
            write_ply(os.path.join(out, "bg.ply"), mesh.vertices, mesh.faces, colors, mesh.vertex_normals)
        export_gltf = bool(self.options.export_gltf if export_gltf is None else export_gltf)
        foreground_scene = self._create_empty_scene(dataset) if export_gltf else None
        if not self.options.background_only:
            with timed_block("Created foreground meshes in", self.profiling, ("timing", "foreground_reconstruction", "total")):
                self.create_foreground_meshes(dataset, n, os.path.join(out, "fg"), scene=foreground_scene)
        if export_gltf:
            self._export_gltf(dataset, n, out, mesh, foreground_scene, compress)
        with open(os.path.join(dataset.base_path, "profiling.json"), "w") as f:  # pipeline.py:251
            json.dump(self.profiling, f, indent=2)
        return mesh


    def _export_gltf(self, dataset, num_frames, mesh_path, static_mesh, foreground_scene, compress):
        """The reference's last four stages (pipeline.py:213-237) under its timing keys (``mesh_export`` is the sum of the PLY and the glTF writing)."""
        if self.storage_options is None:
            self.storage_options = StorageOptions(dataset_path=dataset.base_path, output_path=os.path.dirname(mesh_path))
        background_scene, lut = self._create_background_scene(dataset, static_mesh, num_frames)
        with timed_block("Centred the scenes in", self.profiling, ("timing", "scene_centering")):
            foreground_scene, background_scene = self._center_scenes(dataset, foreground_scene, background_scene)
        ply_seconds = self.profiling.get("timing", {}).get("mesh_export", 0.0)
        with timed_block("Wrote glTF data in", self.profiling, ("timing", "mesh_export")):
            fg_path, bg_path = self._write_meshes_to_disk(mesh_path, foreground_scene, background_scene, overwrite_ok=self.storage_options.overwrite_ok,
                                                          background_lut=lut, texture_format=self.options.texture_format, jpeg_quality=self.options.jpeg_quality,
                                                          png_encoder=self.options.png_encoder)
        self.profiling["timing"]["mesh_export"] += ply_seconds
        with timed_block("Compressed mesh data in", self.profiling, ("timing", "mesh_compression", "total")):
            with timed_block("Quantised the foreground scene in", self.profiling, ("timing", "mesh_compression", "foreground")):
                if compress:
                    self._compress_with_quantisation(fg_path, foreground_scene)
            with timed_block("Quantised the background scene in", self.profiling, ("timing", "mesh_compression", "background")):
                if compress:
                    self._compress_with_quantisation(bg_path, background_scene, lut)
        with timed_block("Exported mesh data in", self.profiling, ("timing", "webxr_export")):
            self._export_video_webxr(mesh_path, fg_scene_name="fg", bg_scene_name="bg", metadata=self._get_webxr_metadata(dataset, num_frames),
                                     export_name=self._get_dataset_name(dataset))


def main(argv=None):
    """`python -m hive_amd ...` / `python -m hive_amd.pipeline ...`: /root/reference/hive/pipeline.py:1337-1339 (and hive/__main__.py:17-20) --
    build the pipeline from the command line and run it."""
    program = Pipeline.from_command_line(argv)
    return program.run()


if __name__ == '__main__':
    main()
