"""Timings, sizes and PSNR of the GPU JPEG encoder (hive_amd.jpeg; csrc/jpeg.hip) on the MI355X (not gated by any test; no ratio is fixed in advance; DESIGN.md
records the figures).  Pictures: the atlases of the eight-frame foreground scene of tools/probe_gltf.py, and one 640 x 480 frame.

  * encode: ms per scene (all atlases in one call) and per texture for the GPU encoder called back to back -- ``encode_to_device`` (launches and the sizes'
    read-back, no download) and ``encode`` (with the download of the files) -- against the PNG step ``write_glb`` takes by default (the texture's download and
    PIL's PNG encoder) and against Pillow's JPEG encoder on the downloaded texture at the same settings, whose files are checked equal to the GPU's: the
    like-for-like host baseline.  The three are timed in turn inside every repeat (alternation), medians over --repeats after two warm-up rounds.
  * write_glb: wall time, its ``png`` / ``jpeg`` step (median, minimum, maximum: inside ``write_glb`` a step behind a large host copy can stall) and the file's
    bytes for PNG and JPEG textures, plain and quantised.
  * PSNR of the decoded (Pillow) textures against the originals at quality 90 and 75, 4:4:4 and 4:2:0, with the bytes.
What is NOT measured: a player (three.js) opening the files; the pipeline end to end; any quality metric but PSNR."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}


def pillow_jpeg(array, quality, subsampling):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(array).save(out, format="JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[subsampling], optimize=False, restart_marker_rows=1)
    return out.getvalue()


def median_ms(samples):
    return 1e3 * statistics.median(samples)


def time_encoders(textures, quality, subsampling, repeats):
    """ms of each way to turn these device textures into files, the ways alternating inside every repeat."""
    import torch
    from hive_amd import gltf, jpeg
    rows = {"gpu_encode_to_device": [], "gpu_encode_with_download": [], "png_step_download_and_pil": [], "pillow_jpeg_download": [], "pillow_jpeg_encode": []}
    files = None
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jpeg.encode_to_device(textures, quality, subsampling)  # returns after the device has finished
        t1 = time.perf_counter()
        files = jpeg.encode(textures, quality, subsampling)
        t2 = time.perf_counter()
        for t in textures:
            gltf._png_bytes(t)
        t3 = time.perf_counter()
        host = [t.cpu().numpy() for t in textures]
        t4 = time.perf_counter()
        theirs = [pillow_jpeg(a, quality, subsampling) for a in host]
        t5 = time.perf_counter()
        assert theirs == files, "Pillow's files and the GPU's are the same bytes"
        if i >= 2:
            for key, value in zip(rows, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                rows[key].append(value)
    out = {key: median_ms(v) for key, v in rows.items()}
    out["gpu_encode_to_device_min_max"] = [1e3 * min(rows["gpu_encode_to_device"]), 1e3 * max(rows["gpu_encode_to_device"])]
    out.update(textures=len(textures), pixels=int(sum(t.shape[0] * t.shape[1] for t in textures)), jpeg_bytes=int(sum(len(f) for f in files)),
               png_bytes=int(sum(len(gltf._png_bytes(t)) for t in textures)))
    out["per_texture"] = {key: out[key] / len(textures) for key in rows}
    return out


def time_write_glb(scene, repeats, folder):
    from hive_amd import gltf
    out = {}
    for fmt in ("png", "jpeg"):
        for quantize in (False, True):
            walls, steps, sizes = [], [], None
            for i in range(repeats + 2):
                scene._packed = {}
                timings = {}
                t0 = time.perf_counter()
                sizes = gltf.write_glb(os.path.join(folder, "probe.glb"), scene, quantize=quantize, texture_format=fmt, timings=timings)
                if i >= 2:
                    walls.append(time.perf_counter() - t0)
                    steps.append(timings[fmt])
            out[f"{fmt}_{'quantised' if quantize else 'plain'}"] = {"wall_ms": median_ms(walls), "texture_step_ms": median_ms(steps),
                                                                    "texture_step_min_max": [1e3 * min(steps), 1e3 * max(steps)], "bytes": sizes}
    return out


def psnr_table(textures):
    from PIL import Image
    from hive_amd import jpeg
    host = [t.cpu().numpy() for t in textures]
    out = {}
    for quality in (90, 75):
        for subsampling in ("4:4:4", "4:2:0"):
            files = jpeg.encode(textures, quality, subsampling)
            error = sum(float(((np.asarray(Image.open(io.BytesIO(f)).convert("RGB")).astype(np.float64) - a) ** 2).sum()) for f, a in zip(files, host))
            mse = error / sum(a.size for a in host)
            out[f"q{quality}_{subsampling}"] = {"psnr_db": float(10 * np.log10(255.0 ** 2 / mse)) if mse else float("inf"), "bytes": int(sum(len(f) for f in files))}
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--frames", type=int, default=8)
    parser.add_argument("--repeats", type=int, default=9)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_probe.json"))
    args = parser.parse_args()
    import torch
    from hive_amd import gltf, synthetic
    from probe_gltf import foreground_scene
    scene = foreground_scene(args.frames)
    atlases = [gltf.mesh_fields(m)[3][:, :, :3].contiguous() for m in scene.meshes()]
    frame = torch.from_numpy(synthetic.make_sequence(num_frames=1, height=480, width=640)["color"][0]).cuda()
    result = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "repeats": args.repeats, "unit": "milliseconds, medians; quality 90, 4:2:0 unless named",
              "atlas_shapes": [list(a.shape[:2]) for a in atlases]}
    result["foreground_atlases"] = time_encoders(atlases, 90, "4:2:0", args.repeats)
    result["frame_640x480"] = time_encoders([frame], 90, "4:2:0", args.repeats)
    with tempfile.TemporaryDirectory() as folder:
        result["write_glb_foreground"] = time_write_glb(scene, args.repeats, folder)
    result["psnr_foreground_atlases"] = psnr_table(atlases)
    result["psnr_frame_640x480"] = psnr_table([frame])
    result["not_measured"] = ["a player (three.js) opening the files", "the pipeline end to end", "any quality metric but PSNR"]
    text = json.dumps(result, indent=2)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
