"""Timings of the ray cast and the tracker (csrc/raycast.hip, csrc/track.hip, hive_amd/tracking.py) at 640 x 480 on the MI355X.  Records, not pass conditions: no
test gates them and there is no earlier figure to compare against (DESIGN.md section 5.13 quotes them).  The scene is the small room of tests/tracking_cases.py seen
from its corner orbit:

  * ``TSDFVolume.raycast`` of a fused 512^3 volume (3.1 mm voxels), depth alone and with all four planes: the median over --repeats calls between device events;
  * one ``icp_align`` at the default settings (3 levels, 10 + 5 + 4 iterations, one copy of 29 numbers per iteration) against a --track-voxels^3 volume: wall clock;
  * ``track_and_fuse`` over the 12-pose orbit with device-resident frames: tracked frames per second (wall clock, integration included) and the ATE RMSE.

Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(samples):
    return round(float(np.median(samples)), 4)


def _time_events(fn, repeats, warmup=5):
    import torch
    samples = []
    for i in range(repeats + warmup):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            samples.append(start.elapsed_time(stop))
    return _median_ms(samples)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--raycast-voxels", type=int, default=512)
    ap.add_argument("--track-voxels", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tracking_cases as tc
    from hive_amd import fusion, tracking
    from hive_amd.geometric import Trajectory
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    H, W = args.height, args.width
    K, orbit = tc.intrinsics(H, W), tc.corner_orbit(12)
    frames = [tc.room_frame(p, K, H, W, seed=i) for i, p in enumerate(orbit)]
    colors = [torch.from_numpy(f[0]).cuda() for f in frames]
    depths = [torch.from_numpy(f[1]).cuda() for f in frames]
    result = {"height": H, "width": W, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "scene": "small room, corner orbit of 12 poses"}

    vol = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / args.raycast_voxels)
    for i in range(4):
        vol.integrate(colors[i], depths[i], K, orbit[i])
    depth = vol.raycast(K, orbit[0], (H, W))
    truth = torch.from_numpy(frames[0][1]).cuda()
    hit = depth > 0
    err_mm = 1000.0 * (depth - truth).abs()[hit]
    result["raycast"] = {
        "voxels": args.raycast_voxels, "frames_fused": 4,
        "depth_only_ms": _time_events(lambda: vol.raycast(K, orbit[0], (H, W)), args.repeats),
        "all_planes_ms": _time_events(lambda: vol.raycast(K, orbit[0], (H, W), return_vertex=True, return_normal=True, return_color=True), args.repeats),
        "hit_share": round(float(hit.float().mean()), 4), "median_error_mm": round(float(err_mm.median()), 4), "max_error_mm": round(float(err_mm.max()), 4)}
    del vol

    vol = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / args.track_voxels)
    vol.integrate(colors[0], depths[0], K, orbit[0])
    samples = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tracking.icp_align(vol, depths[1], K, orbit[0])
        samples.append(1e3 * (time.perf_counter() - t0))
    result["icp_align"] = {"voxels": args.track_voxels, "ms": _median_ms(samples), "ok": bool(res.ok), "iterations": res.iterations_run, "pairs": res.pairs,
                           "cond": round(res.cond, 1), "translation_error_mm": round(1000.0 * float(np.linalg.norm(res.pose[:3, 3] - orbit[1][:3, 3])), 4)}
    del vol

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vol, trajectory, results = tracking.track_and_fuse(colors, depths, K, tc.bounds(), tc.VOLUME / args.track_voxels, first_pose=orbit[0])
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    ate = Trajectory.from_homogenous_transforms(np.linalg.inv(orbit)).calculate_ate(trajectory)
    result["track_and_fuse"] = {"voxels": args.track_voxels, "frames": len(results), "frames_ok": int(sum(r.ok for r in results)),
                                "tracked_frames_per_second": round((len(results) - 1) / seconds, 2),
                                "ate_rmse_mm": round(1000.0 * float(np.sqrt(np.mean(np.sum(ate ** 2, axis=1)))), 4)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
