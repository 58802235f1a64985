"""Timings and sizes of the GPU PNG encoder (hive_amd.png; csrc/png.hip) on the MI355X (not gated by any test; no ratio is fixed in advance; DESIGN.md records
the figures).  Pictures: eight 640 x 480 uint16 depth maps (a smooth ramp with 3 bits of noise, tests/png_cases.py's recipe at other seeds) and the atlases of
the eight-frame foreground scene of tools/probe_gltf.py.

  * encode: ms per batch for the GPU encoder called back to back -- ``encode_to_device`` (launches and the sizes' read-back, no download) and ``encode`` (with
    the download of the files) -- against the pictures' download and Pillow's PNG encoder at compress_level 1 and at its default 6 on the downloaded pixels.
    The four are timed in turn inside every repeat (alternation), medians over --repeats after two warm-up rounds.  Every GPU file is decoded with Pillow once
    and compared with the pixels.
  * sizes: the GPU files' bytes against Pillow's at level 1 and level 6, per batch; and, from the numpy restatement (no GPU), the four cases of the size record
    that tests/test_png_cpu.py pins.
  * estimate_depth_dpt: frames per second with ``png_encoder="host"`` against ``"gpu"`` on 640 x 480 frames, from the difference of a long and a short run (the
    weights load once per run); a seeded model written to a temporary weights file if ``--weights`` names none.
What is NOT measured: ``inpaint_frame_data`` and ``write_glb`` end to end with the GPU encoder; the pipeline end to end; any picture larger than 640 x 480."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pillow_png(array, level):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(array).save(out, format="PNG", compress_level=level)
    return out.getvalue()


def median_ms(samples):
    return 1e3 * statistics.median(samples)


def depth_maps(count, height=480, width=640):
    yy, xx = np.mgrid[0:height, 0:width]
    out = []
    for k in range(count):
        rng = np.random.default_rng(100 + k)
        smooth = 1500 + 40 * k + 3 * xx + 2 * yy + (200 * np.sin((xx + 11 * k) / 37.0) * np.cos(yy / 23.0)).astype(np.int64)
        out.append((smooth + rng.integers(0, 8, (height, width))).astype(np.uint16))
    return out


def time_encoders(pictures, repeats):
    """ms of each way to turn these device pictures into PNG files, the ways alternating inside every repeat."""
    import torch
    from PIL import Image
    from hive_amd import png
    rows = {"gpu_encode_to_device": [], "gpu_encode_with_download": [], "download_pixels": [], "pillow_level_1": [], "pillow_level_6": []}
    files = level1 = level6 = host = None
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        png.encode_to_device(pictures)  # returns after the device has finished
        t1 = time.perf_counter()
        files = png.encode(pictures)
        t2 = time.perf_counter()
        host = [p.cpu().numpy() for p in pictures]
        t3 = time.perf_counter()
        level1 = [pillow_png(a, 1) for a in host]
        t4 = time.perf_counter()
        level6 = [pillow_png(a, 6) for a in host]
        t5 = time.perf_counter()
        if i >= 2:
            for key, value in zip(rows, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                rows[key].append(value)
    for f, a in zip(files, host):
        assert np.array_equal(np.array(Image.open(io.BytesIO(f))).astype(a.dtype), a), "the GPU's files decode to the pixels"
    out = {key: median_ms(v) for key, v in rows.items()}
    out["gpu_encode_to_device_min_max"] = [1e3 * min(rows["gpu_encode_to_device"]), 1e3 * max(rows["gpu_encode_to_device"])]
    sizes = {"gpu": sum(len(f) for f in files), "pillow_level_1": sum(len(f) for f in level1), "pillow_level_6": sum(len(f) for f in level6),
             "raw": int(sum(a.nbytes for a in host))}
    out.update(pictures=len(pictures), bytes=sizes, gpu_over_level_1=sizes["gpu"] / sizes["pillow_level_1"], gpu_over_level_6=sizes["gpu"] / sizes["pillow_level_6"])
    out["per_picture"] = {key: out[key] / len(pictures) for key in rows}
    return out


def size_record():
    """ours / Pillow from the restatement alone (what tests/test_png_cpu.py pins)."""
    import png_cases as C
    out = {}
    for content, kind in C.SIZE_RECORD:
        picture = np.asarray(C.picture(content, kind))
        ours, level1, level6 = len(C.restated(content, kind)[0]), len(pillow_png(picture, 1)), len(pillow_png(picture, 6))
        out[f"{content}_{kind}"] = {"ours": ours, "pillow_level_1": level1, "pillow_level_6": level6, "raw": int(picture.nbytes), "over_level_1": ours / level1,
                                    "over_level_6": ours / level6}
    return out


def depth_estimation_rate(weights, repeats, short=16, long=80):
    """frames per second of estimate_depth_dpt per encoder: (long - short) frames over the difference of the two runs' wall times."""
    import torch
    from hive_amd import depth, synthetic
    frames = list(synthetic.make_sequence(num_frames=8, height=480, width=640)["color"])
    seeded = weights is None
    with tempfile.TemporaryDirectory() as folder:
        if seeded:
            model = depth.build_model(None, device="cpu", dtype=None, engine="torch", init_seed=4)
            torch.save(model.state_dict(), os.path.join(folder, "dpt_hybrid_nyu.pt"))
            del model
            weights_dir = folder
        else:
            weights_dir = os.path.dirname(os.path.abspath(weights))
        previous = os.environ.get("WEIGHTS_PATH")
        os.environ["WEIGHTS_PATH"] = weights_dir
        try:
            walls = {"host": {short: [], long: []}, "gpu": {short: [], long: []}}
            for i in range(repeats + 1):
                for count in (short, long):
                    for encoder in ("host", "gpu"):
                        data = [frames[k % len(frames)] for k in range(count)]
                        t0 = time.perf_counter()
                        depth.estimate_depth_dpt(data, os.path.join(folder, f"{encoder}_{count}"), weights_filename=os.path.basename(weights) if weights else "dpt_hybrid_nyu.pt",
                                                 png_encoder=encoder)
                        if i >= 1:
                            walls[encoder][count].append(time.perf_counter() - t0)
        finally:
            if previous is None:
                del os.environ["WEIGHTS_PATH"]
            else:
                os.environ["WEIGHTS_PATH"] = previous
    out = {"weights": "seeded (hive_amd.dpt.init, seed 4)" if seeded else os.path.basename(weights), "frames_short": short, "frames_long": long}
    for encoder in walls:
        a, b = statistics.median(walls[encoder][short]), statistics.median(walls[encoder][long])
        out[encoder] = {"wall_s_short": a, "wall_s_long": b, "frames_per_second": (long - short) / (b - a) if b > a else None}
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--frames", type=int, default=8)
    parser.add_argument("--repeats", type=int, default=9)
    parser.add_argument("--weights", default=None, help="a DPT-Hybrid weights file for the estimate_depth_dpt rows (default: a seeded model)")
    parser.add_argument("--skip_depth_estimation", action="store_true")
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_probe.json"))
    args = parser.parse_args()
    import torch
    from hive_amd import gltf
    from probe_gltf import foreground_scene
    scene = foreground_scene(args.frames)
    atlases = [gltf.mesh_fields(m)[3][:, :, :3].contiguous() for m in scene.meshes()]
    maps = [torch.from_numpy(a).cuda() for a in depth_maps(args.frames)]
    result = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "repeats": args.repeats, "unit": "milliseconds, medians of the repeats after 2 warm-up rounds",
              "atlas_shapes": [list(a.shape[:2]) for a in atlases]}
    result["depth_maps_640x480_uint16"] = time_encoders(maps, args.repeats)
    result["foreground_atlases"] = time_encoders(atlases, args.repeats)
    result["size_record_from_the_restatement"] = size_record()
    if not args.skip_depth_estimation:
        result["estimate_depth_dpt"] = depth_estimation_rate(args.weights, 3)
    result["not_measured"] = ["inpaint_frame_data and write_glb end to end with png_encoder='gpu'", "the pipeline end to end", "pictures larger than 640 x 480"]
    text = json.dumps(result, indent=2)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
