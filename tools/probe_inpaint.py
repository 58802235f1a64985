#!/usr/bin/env python3
"""Cost of the background inpainting (hive_inpaint_frames: colour + depth, masks dilated 5 x 5 five times, radius 30 -- what --inpainting_mode 1 runs) at
640 x 480 and 1920 x 1080, ellipse masks of 1-3 objects, batches of 1 and 32 frames of the synthetic room.  Each configuration: the median wall time of
REPEATS calls after a warm-up (3 calls where one takes more than half a second), per frame, with the hole pixels and the level counts.  Prints one JSON object.
Usage (GPU box): python tools/probe_inpaint.py [--sizes vga,1080p] [--batches 1,32]
Per-kernel split: rocprofv3 --kernel-trace --stats -- python tools/probe_inpaint.py --sizes vga --batches 32"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hive_amd import _lib, synthetic  # noqa: E402
from hive_amd.dataset_adaptors import INPAINTING_MASK_DILATION, INPAINTING_RADIUS  # noqa: E402
from hive_amd.image_processing import inpaint_frames  # noqa: E402

REPEATS, WARMUP = 20, 2
SIZES = {"vga": (480, 640), "1080p": (1080, 1920)}


def time_calls(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    repeats = 3 if first > 0.5 else REPEATS
    for _ in range(0 if first > 0.5 else WARMUP):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(samples)), repeats


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", default="vga,1080p")
    parser.add_argument("--batches", default="1,32")
    parser.add_argument("--objects", default="1,2,3")
    args = parser.parse_args()
    ctx = _lib.default_context(0)
    out = {}
    for size in args.sizes.split(","):
        H, W = SIZES[size]
        seq = synthetic.make_sequence(num_frames=2, height=H, width=W, yaw_step_deg=2.4)
        for batch in (int(b) for b in args.batches.split(",")):
            pick = np.arange(batch) % 2
            rgb = torch.from_numpy(seq["color"][pick]).cuda()
            depth = torch.from_numpy((seq["depth"][pick] * 1000.0).astype(np.uint16)).cuda()
            for objects in (int(o) for o in args.objects.split(",")):
                masks = torch.from_numpy(synthetic.ellipse_masks(batch, H, W, num_objects=objects, seed=3)).cuda()
                call = lambda: inpaint_frames(rgb, depth, masks, dilation=INPAINTING_MASK_DILATION, radius=INPAINTING_RADIUS, ctx=ctx, return_levels=True)
                filled_rgb, _, levels = call()
                holes = int((filled_rgb != rgb).any(dim=3).sum())  # (a lower bound: a filled pixel may come back with its captured colour)
                ms, repeats = time_calls(call)
                out[f"{size}_batch{batch}_objects{objects}"] = {"ms_per_call": ms, "ms_per_frame": ms / batch, "repeats": repeats, "levels_max": int(levels.max()),
                                                                  "levels_mean": float(levels.mean()), "changed_pixels_per_frame": holes / batch}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "radius": INPAINTING_RADIUS, "dilation": INPAINTING_MASK_DILATION, "results": out}, indent=1))


if __name__ == "__main__":
    main()
