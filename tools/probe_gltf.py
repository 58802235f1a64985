"""Timings of the glTF export (hive_amd.gltf.write_glb; csrc/gltf.hip) on the MI355X (not gated by any test; no ratio is fixed in advance; DESIGN.md records the
figures).  Two scenes:

  * the foreground of the tests' three-ellipse sequence: --frames frames at 480 x 640 through ``foreground.process_frame``, device-resident float64 meshes;
  * a background of about 730 k faces: a 605 x 605 height field with vertex colours, once device-resident (float64) and once as the host float32 arrays the
    pipeline's fused mesh arrives in (the upload is then part of the pack).

For each: the median over --repeats ``write_glb`` calls (the scene's packing cache cleared before each), plain and quantised, split into pack (layout, upload of
host meshes, three launches, the bounds read-back), download (the ONE copy of the buffer), png (PIL) and file write.  Beside it the BASELINE: the same geometry
bytes made on the host with numpy from host copies of the scene's tensors as they are (float64 vertices and uv, int64 faces) -- the download of those tensors
and the numpy conversion timed apart -- and checked equal to the device's bytes.  ``pack_alone`` is the pack step called back to back (no download, no file
write between the calls): inside ``write_glb`` the step that follows a file of several megabytes can stall on the host, so ``pack`` carries its minimum and
maximum.  What is NOT measured: PNG encoding and the file write are the same code on both
sides and are only reported once; nothing here opens the files in a viewer (three.js, trimesh), and draco is not run."""
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


def foreground_scene(frames):
    import torch
    from hive_amd import foreground, gltf, synthetic
    from hive_amd.options import MaskDilationOptions, MeshFilteringOptions
    H, W = 480, 640
    seq = synthetic.make_sequence(num_frames=frames, height=H, width=W, yaw_step_deg=10.0)
    masks = synthetic.ellipse_masks(frames, H, W, num_objects=3, seed=5)
    scene = gltf.Scene(camera=dict(resolution=(W, H), focal=(seq["K"][0, 0], seq["K"][1, 1])))
    buffers = foreground.FrameMeshBuffers(H, W)
    for i in range(frames):
        ids = masks[i].copy()
        ids[seq["depth"][i] == 0] = 0
        mesh = foreground.process_frame(torch.from_numpy(seq["color"][i]).cuda(), torch.from_numpy(seq["depth"][i]).cuda(), torch.from_numpy(ids).cuda(), seq["K"],
                                        np.linalg.inv(seq["poses"][i]), MaskDilationOptions(num_iterations=0), MeshFilteringOptions(), buffers=buffers,
                                        enable_cc_analysis=True)
        if mesh is not None:
            scene.add_geometry({k: mesh[k].clone() for k in ("vertices", "faces", "uv", "texture")}, node_name=f"{i:06d}")
    return scene


def background_arrays(side=605):
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:side, 0:side]
    vertices = np.stack([x * 0.01, y * 0.01, 2.0 + 0.2 * np.sin(x * 0.05) * np.cos(y * 0.04)], axis=-1).reshape(-1, 3)
    ids = np.arange(side * side).reshape(side, side)
    a, b, c, d = ids[:-1, :-1].ravel(), ids[:-1, 1:].ravel(), ids[1:, :-1].ravel(), ids[1:, 1:].ravel()
    faces = np.stack([np.stack([a, c, b], 1), np.stack([b, c, d], 1)], 1).reshape(-1, 3)
    return vertices, faces, rng.integers(0, 256, (side * side, 3), dtype=np.uint8)


def host_baseline(scene, quantize, lut, repeats):
    """(median seconds of the tensors' download, of the numpy conversion, the bytes) for the scene's meshes taken to the host as they are."""
    import torch
    import gltf_restatement as R
    from hive_amd.gltf import mesh_fields
    down, convert, data = [], [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meshes = []
        for m in scene.meshes():
            v, f, uv, texture, colors = mesh_fields(m)
            host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            row = {"vertices": host(v), "faces": host(f)}
            if colors is not None:
                row["colors"] = host(colors)
            else:
                row["uv"] = host(uv)
            meshes.append(row)
        t1 = time.perf_counter()
        data, _ = R.pack(meshes, quantize, lut)
        t2 = time.perf_counter()
        down.append(t1 - t0)
        convert.append(t2 - t1)
    return statistics.median(down), statistics.median(convert), data


def measure(scene, lut, repeats, folder):
    import torch
    from hive_amd import gltf
    out = {"meshes": len(scene.meshes()), "vertices": int(sum(len(gltf.mesh_fields(m)[0]) for m in scene.meshes())),
           "faces": int(sum(len(gltf.mesh_fields(m)[1]) for m in scene.meshes()))}
    for quantize in (False, True):
        samples, sizes = [], None
        for i in range(repeats + 2):
            scene._packed = {}
            timings = {}
            sizes = gltf.write_glb(os.path.join(folder, "probe.glb"), scene, quantize=quantize, lut=lut, timings=timings)
            if i >= 2:
                samples.append(timings)
        row = {key: 1e3 * statistics.median(s.get(key, 0.0) for s in samples) for key in ("pack", "download", "json", "png", "file")}
        row["total_ms"] = sum(row.values())
        row["pack_min_max"] = [1e3 * min(s["pack"] for s in samples), 1e3 * max(s["pack"] for s in samples)]
        alone = []  # layout + pack + bounds read-back with no download and no file write between the calls
        for i in range(repeats + 2):
            scene._packed = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gltf._pack(scene, quantize, lut)
            alone.append(1e3 * (time.perf_counter() - t0))
        row["pack_alone"] = statistics.median(alone[2:])
        row["pack_alone_min_max"] = [min(alone[2:]), max(alone[2:])]
        down, convert, data = host_baseline(scene, quantize, lut, max(2, repeats // 2))
        device_bytes = gltf._pack(scene, quantize, lut)[0].cpu().numpy().tobytes()
        assert device_bytes == data, "the host baseline and the device make the same bytes"
        row.update(bytes=sizes, baseline_download_ms=1e3 * down, baseline_numpy_ms=1e3 * convert, geometry_ms=row["pack"] + row["download"],
                   baseline_geometry_ms=1e3 * (down + convert))
        out["quantised" if quantize else "plain"] = row
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--frames", type=int, default=8)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "gltf_probe.json"))
    args = parser.parse_args()
    import torch
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    lut = (255 * np.power(np.arange(256) / 255, 2.2)).astype(np.uint8)
    result = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "repeats": args.repeats, "unit": "milliseconds, medians"}
    with tempfile.TemporaryDirectory() as folder:
        result["foreground_three_ellipses"] = measure(foreground_scene(args.frames), None, args.repeats, folder)
        vertices, faces, colours = background_arrays()
        on_device = gltf.Scene()
        on_device.add_geometry({"vertices": torch.from_numpy(vertices).cuda(), "faces": torch.from_numpy(faces).cuda(), "vertex_colors": torch.from_numpy(colours).cuda()},
                               node_name="000000")
        result["background_730k_faces_device_float64"] = measure(on_device, lut, args.repeats, folder)
        on_host = gltf.Scene()
        on_host.add_geometry(Mesh(vertices.astype(np.float32), faces.astype(np.int32), colours), node_name="000000")
        result["background_730k_faces_host_float32"] = measure(on_host, lut, args.repeats, folder)
    result["not_measured"] = ["opening the files in three.js or trimesh", "draco_transcoder", "PNG encoding and the file write on the baseline side (the same code)"]
    text = json.dumps(result, indent=2)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
