"""Timings of the motion segmentation (hive_amd.segmentation; csrc/segment.hip) on the MI355X (not gated by any test; no target is fixed in advance; the README
and DESIGN.md quote the figures).  At 640 x 480, for 1 frame and for 64 frames:

  * label: ``label_components`` alone (int32 labels, connectivity 8; launches and the drain of the stream) on a random mask at density 0.5 and on a one-blob
    mask (a disc of radius 150), beside ``scipy.ndimage.label`` on the host of the same box, on the same masks, and the masks' download it would need.
  * fused: ``motion_masks`` (``hive_motion_segment``: motion rule, one opening iteration, labelling, 1 % area filter, with its one read-back) on a room with
    drifting ellipses pulled 30 % towards the camera, beside the same three steps in numpy / scipy on the host.
  * segment_dataset: seconds per frame of ``segment_dataset(write=False)`` on that sequence written as a HIVE folder (PNG decoding, fusion at 2 cm voxels, the
    ray casts and the segmentation), and of the ray casts plus the segmentation alone.
Medians of --repeats after two warm-up rounds (segment_dataset: of three after one).
What is NOT measured: a real capture; pictures larger than 640 x 480; ``convert(segment_motion=True)`` end to end; the PNG writing."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640


def timed(fn, repeats, warmup=2):
    import torch
    samples = []
    for i in range(repeats + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            samples.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(samples)


def host_timed(fn, repeats):
    samples = []
    for i in range(repeats + 1):
        t0 = time.perf_counter()
        fn()
        if i >= 1:
            samples.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(samples)


def label_rows(n, repeats):
    import torch
    from scipy import ndimage
    from hive_amd import segmentation as seg
    import segmentation_restatement as sr
    rng = np.random.default_rng(7)
    v, u = np.mgrid[0:H, 0:W]
    masks = {"random_0.5": (rng.random((n, H, W)) < 0.5).astype(np.uint8),
             "one_blob": np.repeat((((v - 240) ** 2 + (u - 320) ** 2) <= 150 ** 2).astype(np.uint8)[None], n, axis=0)}
    out = {}
    for name, m in masks.items():
        d = torch.from_numpy(m).cuda()
        labels, counts = seg.label_components(d)
        want = sr.label(m[0], 8)
        assert np.array_equal(labels[0].cpu().numpy(), want[0]) and int(counts[0]) == want[1], name
        out[name] = {"gpu_ms": timed(lambda: seg.label_components(d), repeats), "download_mask_ms": timed(lambda: d.cpu(), repeats),
                     "scipy_label_host_ms": host_timed(lambda: [ndimage.label(x, structure=sr.BOX) for x in m], max(3, repeats // 3)),
                     "components_in_frame_0": want[1]}
    return out


def moving_sequence(n):
    """A room with up to three ellipses pulled 30 % towards the camera: (sequence dict, live depth)."""
    from hive_amd import synthetic
    seq = synthetic.make_sequence(num_frames=n, height=H, width=W, yaw_step_deg=1.0, invalid_fraction=0.0)
    ids = synthetic.ellipse_masks(n, H, W, seed=5)
    live = np.where(ids > 0, seq["depth"] * np.float32(0.7), seq["depth"]).astype(np.float32)
    return seq, live


def fused_rows(n, repeats, seq, live):
    import torch
    from hive_amd import segmentation as seg
    import segmentation_restatement as sr
    d_live, d_model = torch.from_numpy(live[:n]).cuda(), torch.from_numpy(seq["depth"][:n]).cuda()
    ids, counts = seg.motion_masks(d_live, d_model)
    want = sr.motion_masks(live[:1], seq["depth"][:1])
    assert np.array_equal(ids[0].cpu().numpy(), want[0][0])
    return {"gpu_ms": timed(lambda: seg.motion_masks(d_live, d_model), repeats),
            "numpy_scipy_host_ms": host_timed(lambda: sr.motion_masks(live[:n], seq["depth"][:n]), max(3, repeats // 3)), "objects_per_frame": counts.cpu().tolist()[:8]}


def dataset_rows(n, seq, live):
    import torch
    from PIL import Image
    from hive_amd import fusion, segmentation as seg, synthetic
    from hive_amd.geometric import Trajectory
    from hive_amd.io import DatasetMetadata, HiveDataset
    from hive_amd.options import BackgroundMeshOptions
    with tempfile.TemporaryDirectory() as folder:
        for name in HiveDataset.required_folders:
            os.makedirs(os.path.join(folder, name))
        DatasetMetadata(num_frames=n, fps=30.0, width=W, height=H).save(os.path.join(folder, HiveDataset.metadata_filename))
        np.savetxt(os.path.join(folder, HiveDataset.camera_matrix_filename), seq["K"])
        Trajectory(synthetic.trajectory_rows_world_to_cam(seq["poses"][:n])).save(os.path.join(folder, HiveDataset.camera_trajectory_filename))
        for i in range(n):
            name = HiveDataset.index_to_filename(i)
            Image.fromarray(seq["color"][i]).save(os.path.join(folder, "rgb", name))
            Image.fromarray((live[i] * 1000.0).astype(np.uint16)).save(os.path.join(folder, "depth", name))
            Image.fromarray(np.zeros((H, W), np.uint8)).save(os.path.join(folder, "mask", name))
        dataset = HiveDataset(folder)
        options = BackgroundMeshOptions(sdf_voxel_size=0.02)
        walls, result = [], None
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = seg.segment_dataset(dataset, mesh_options=options, write=False)
            torch.cuda.synchronize()
            if i >= 1:
                walls.append(time.perf_counter() - t0)
        frames = fusion.DeviceFrames.from_dataset(dataset, list(range(n)), with_masks=False, with_color=False)

        def cast_and_segment():
            model = torch.stack([result.volume.raycast(dataset.camera_matrix, pose, (H, W)) for pose in frames.poses])
            seg.motion_masks(frames.depth, model)
        return {"segment_dataset_s_per_frame": statistics.median(walls) / n, "raycast_and_segment_ms_per_frame": timed(cast_and_segment, 3, 1) / n,
                "frames_with_an_object": int((result.counts > 0).sum()), "voxel_size_m": 0.02, "volume_dims": [int(v) for v in result.volume.vol_dim]}


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--repeats", type=int, default=9)
    parser.add_argument("--frames", type=int, nargs="+", default=[1, 64])
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmentation_probe.json"))
    args = parser.parse_args()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "height": H, "width": W, "repeats": args.repeats,
              "unit": "milliseconds per call (all frames of the batch), medians of the repeats after 2 warm-up rounds, unless the key says otherwise"}
    seq, live = moving_sequence(max(args.frames))
    for n in args.frames:
        row = result[f"frames_{n}"] = {}
        for key, fn in (("label", lambda: label_rows(n, args.repeats)), ("fused", lambda: fused_rows(n, args.repeats, seq, live)),
                        ("segment_dataset", lambda: dataset_rows(n, seq, live))):
            row[key] = fn()
            print(f"# {n} frame(s): {key} done", file=sys.stderr, flush=True)
    result["not_measured"] = ["a real capture", "pictures larger than 640 x 480", "convert(segment_motion=True) end to end", "the PNG writing"]
    text = json.dumps(result, indent=2)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
