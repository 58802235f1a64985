"""What the photometric term costs (csrc/track.hip hive_rgbd_icp_step, hive_amd/tracking.py) on the MI355X: one ``icp_align`` at 640 x 480 against a 512^3 volume
(3.1 mm voxels) at the default settings -- 3 levels, 10 + 5 + 4 iterations -- with colour off and colour on (photometric_weight 0.1) in turn, wall clock, the
medians of 9 runs after 2.  A record, not a pass condition: no test gates it (DESIGN.md section 5.13 quotes it).  Structurally the two differ by one colour
plane per level's ray cast, the intensity pyramid once per frame, and 58 numbers instead of 29 per iteration from the same launch pair and the same one copy.

The scene is the small room of tests/tracking_cases.py: the corner view, where both variants run all 19 iterations, and the two-wall view, which only colour
keeps.  Prints one JSON object and writes it to --out (default profiles/photometric_probe.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WEIGHT = 0.1


def _align_ms(tracking, torch, runs, warmup, *args, **kw):
    samples = []
    for i in range(runs + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tracking.icp_align(*args, **kw)
        if i >= warmup:
            samples.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(samples)), 4), res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxels", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_probe.json"))
    args = ap.parse_args()
    import torch
    import photometric_cases as pc
    import tracking_cases as tc
    from hive_amd import fusion, tracking
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    H, W = args.height, args.width
    K = tc.intrinsics(H, W)
    result = {"height": H, "width": W, "voxels": args.voxels, "runs": args.runs, "warmup": args.warmup, "photometric_weight": WEIGHT,
              "device": torch.cuda.get_device_name(0)}
    two_wall = [tc.two_wall_pose(), tc.two_wall_pose()]
    two_wall[1][:3, 3] += pc.TWO_WALL_MOVE
    for name, (model_pose, live_pose) in (("corner", tc.corner_orbit(12)[:2]), ("two_wall", two_wall)):
        frames = [tc.room_frame(p, K, H, W, seed=i) for i, p in enumerate((model_pose, live_pose))]
        colors = [torch.from_numpy(f[0]).cuda() for f in frames]
        depths = [torch.from_numpy(f[1]).cuda() for f in frames]
        vol = fusion.TSDFVolume(tc.bounds(), tc.VOLUME / args.voxels)
        vol.integrate(colors[0], depths[0], K, model_pose)
        entry = {}
        for label, kw in (("colour_off", {}), ("colour_on", {"color": colors[1], "photometric_weight": WEIGHT})):
            ms, res = _align_ms(tracking, torch, args.runs, args.warmup, vol, depths[1], K, model_pose, **kw)
            entry[label] = {"ms": ms, "ok": bool(res.ok), "iterations": res.iterations_run, "pairs": res.pairs, "cond": round(res.cond, 1) if np.isfinite(res.cond) else None,
                            "translation_error_mm": round(1000.0 * float(np.linalg.norm(res.pose[:3, 3] - live_pose[:3, 3])), 4)}
        if entry["colour_off"]["iterations"] == entry["colour_on"]["iterations"]:
            entry["on_over_off"] = round(entry["colour_on"]["ms"] / entry["colour_off"]["ms"], 3)
        result[name] = entry
        del vol
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
