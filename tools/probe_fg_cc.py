#!/usr/bin/env python3
"""Cost of the connected-component clean-up on the frame path: ms per object of hive_fg_frame_mesh against hive_fg_frame_mesh_cc (the same mesh plus the
floater removal, the texture window over the vertices left) at 640 x 480 and 1920 x 1080 -- a full-frame object and an ellipse object of the synthetic room, each
call timed over repeats after a warm-up (one read-back per call: the wall time per call is the per-object cost the pipeline pays).  Prints one JSON object.
Usage (GPU box): python tools/probe_fg_cc.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hive_amd import _lib, foreground, synthetic  # noqa: E402
from hive_amd.options import MeshFilteringOptions  # noqa: E402

REPEATS, WARMUP = 50, 5


def time_calls(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        samples.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(samples))


def main():
    ctx = _lib.default_context(0)
    opts = MeshFilteringOptions()
    out = {}
    for H, W in ((480, 640), (1080, 1920)):
        seq = synthetic.make_sequence(num_frames=1, height=H, width=W, yaw_step_deg=2.4)
        w2c = np.linalg.inv(seq["poses"][0])
        R, t, K = w2c[:3, :3], w2c[:3, 3:4], seq["K"]
        depth, rgb = torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(seq["color"][0]).cuda()
        ellipse = torch.from_numpy(synthetic.ellipse_masks(1, H, W, num_objects=1, seed=3)[0] == 1).cuda()
        buffers = foreground.FrameMeshBuffers(H, W)
        for name, mask in (("full_frame", None), ("ellipse", ellipse)):
            plain = lambda: foreground.frame_mesh(depth, mask, rgb, K, R, t, opts, ctx=ctx, buffers=buffers)
            cc = lambda: foreground.frame_mesh(depth, mask, rgb, K, R, t, opts, ctx=ctx, buffers=buffers, enable_cc_analysis=True)
            a, b = plain(), cc()
            row = {"faces": int(a["faces"].shape[0]), "faces_after_cc": int(b["faces"].shape[0]), "vertices": int(a["vertices"].shape[0]),
                   "vertices_after_cc": int(b["vertices"].shape[0]), "ms_fg_frame_mesh": time_calls(plain), "ms_fg_frame_mesh_cc": time_calls(cc)}
            row["ms_cleanup"] = row["ms_fg_frame_mesh_cc"] - row["ms_fg_frame_mesh"]
            out[f"{W}x{H}_{name}"] = row
    print(json.dumps({"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "results": out}, indent=1))


if __name__ == "__main__":
    main()
