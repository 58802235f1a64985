"""Timings of the rigid RANSAC of frame registration (hive_amd.features.ransac_rigid; csrc/register.hip) on the MI355X (not gated by any test; there is no earlier
number to beat, so no threshold; DESIGN.md section 5.20 records the figures).  The rows are those of tools/probe_pairs.py -- the keypoint-rich blob pair of
tests/sift_cases.py at 640 x 480, detected once and matched -- over a constant-depth plane, on which the pixel shift between the two pictures is a rigid motion;
pair p of a batch has the pair key (p, p + 1), so every pair draws its own samples over the same correspondences.

  * ransac_rigid with --trials trials alone between device events after warm-up: the median over --repeats calls with the minimum and the maximum beside it,
    for one pair and for --batch pairs; ransac_homography on the same rows beside it;
  * for orientation only, the host time of tests/rigid_restatement.py (numpy, one core) for one pair.

It asserts what it times: the first pair's T, scale, rms, mask and winning trial against the restatement, bit for bit.  Prints one JSON object; --out also
writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, repeats, warmup=3):
    """(median, min, max) milliseconds of ``call`` between device events."""
    import torch
    samples = []
    for i in range(repeats + warmup):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        if i >= warmup:
            samples.append(start.elapsed_time(stop))
    return tuple(round(float(f(samples)), 4) for f in (np.median, np.min, np.max))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--trials", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--capacity", type=int, default=8192)
    ap.add_argument("--min-features", type=int, default=20)
    ap.add_argument("--depth", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rigid_restatement as GR
    import sift_cases
    from hive_amd import features
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    ref, est = sift_cases.pair(args.height, args.width, 0, True)
    sift = features.SIFT(nfeatures=2048, capacity=args.capacity)
    feats = sift.detect_device(torch.from_numpy(np.stack([ref, est])).cuda())
    counts = feats[2].cpu().numpy()
    sift.check_counts(counts)
    depth = torch.full((2, args.height, args.width), args.depth, dtype=torch.float32).cuda()
    K = np.array([[525.0, 0.0, (args.width - 1) / 2], [0.0, 525.0, (args.height - 1) / 2], [0.0, 0.0, 1.0]])
    result = {"height": args.height, "width": args.width, "batch": args.batch, "trials": args.trials, "repeats": args.repeats, "threshold": args.threshold,
              "depth": args.depth, "device": torch.cuda.get_device_name(0),
              "rows": "tests/sift_cases.pair(H, W, 0, noise=True) detected once with nfeatures = 2048 and matched (ratio 0.7) over a constant-depth plane; pair p has the key (p, p + 1)",
              "keypoints": [int(counts[0, 2]), int(counts[1, 2])],
              "times": "milliseconds between device events: median [min, max] over the repeats, every call alone"}
    for count in (1, args.batch):
        keys = torch.tensor([(p, p + 1) for p in range(count)], dtype=torch.int32).cuda()
        pairs = torch.tensor([(0, 1)] * count, dtype=torch.int32).cuda()
        rows, pair_counts = features.match_pairs(feats, pairs, depth, 0.7, args.min_features)
        rigid_call = lambda: features.ransac_rigid(rows, pair_counts[:, 1], keys, K, args.threshold, args.trials, 0, args.min_features)
        T, scale, rms, mask, res = rigid_call()
        rigid = timed(rigid_call, args.repeats)
        homography = timed(lambda: features.ransac_homography(rows, pair_counts[:, 1], keys, 3.0, args.trials, 0, args.min_features), args.repeats)
        pc, res_h = pair_counts.cpu().numpy(), res.cpu().numpy()
        result["one_pair" if count == 1 else f"{count}_pairs"] = {
            "rigid_ms": rigid[0], "rigid_min_max_ms": rigid[1:], "rigid_per_pair_ms": round(rigid[0] / count, 4),
            "homography_ms": homography[0], "homography_min_max_ms": homography[1:], "homography_per_pair_ms": round(homography[0] / count, 4),
            "rows": int(pc[0, 1]), "inliers_min": int(res_h[:, 2].min()), "inliers_max": int(res_h[:, 2].max()),
            "distinct_winning_trials": int(len(set(res_h[:, 0].tolist())))}
        n = int(pc[0, 1])
        t0 = time.perf_counter()
        fit = GR.ransac(rows[0, :n].cpu().numpy(), GR.camera_of(K), args.threshold, args.trials, 0, (0, 1), min_count=args.min_features)
        t1 = time.perf_counter()
        assert res_h[0].tolist() == [fit["trial"], fit["winner_count"], fit["count"]] and T[0].cpu().numpy().tobytes() == fit["T"].tobytes()
        assert (mask[0, :n].cpu().numpy() == fit["mask"]).all() and float(rms[0]) == fit["rms"] and float(scale[0]) == fit["scale"]
        result["restatement_host_seconds_one_pair"] = round(t1 - t0, 3)
        result["first_pair_matches_the_restatement_bit_for_bit"] = True
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    sift.close()
