"""Timings of the feature-pair stage of the pose optimiser (hive_amd.features.match_pairs and ransac_homography; csrc/pairs.hip) at 640 x 480 on the MI355X (not
gated by any test; there is no earlier number to beat, so no threshold; DESIGN.md section 5.15 records the figures).  The pictures are the keypoint-rich blob
pair of tests/sift_cases.py at that size, detected once; pair p of a batch is (reference, estimate) with the pair key (p, p + 1), so every pair draws its own
samples over the same correspondences.

  * the matcher with its filter, and the RANSAC with --trials trials, each alone between device events after warm-up: the median over --repeats calls with the
    minimum and the maximum beside it, for one pair and for --batch pairs; the compaction likewise;
  * for orientation only, the host time of tests/ransac_restatement.py (numpy, one core) for the filter and for the RANSAC of one pair.

It asserts what it times: the first pair's rows, counts, H, mask and winning trial against the restatement, bit for bit.  Prints one JSON object; --out also
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=8192)
    ap.add_argument("--min-features", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ransac_restatement as RR
    import sift_cases
    from hive_amd import features
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    ref, est = sift_cases.pair(args.height, args.width, 0, True)
    sift = features.SIFT(nfeatures=2048, capacity=args.capacity)
    feats = sift.detect_device(torch.from_numpy(np.stack([ref, est])).cuda())
    counts = feats[2].cpu().numpy()
    sift.check_counts(counts)
    yy, xx = np.mgrid[0:args.height, 0:args.width]
    depth_h = np.stack([(1.0 + 0.01 * yy + 0.005 * xx).astype(np.float32)] * 2)
    depth_h[0, args.height // 3:args.height // 3 + 40, args.width // 2:args.width // 2 + 60] = 0.0  # some keypoints without depth
    depth = torch.from_numpy(depth_h).cuda()
    result = {"height": args.height, "width": args.width, "batch": args.batch, "trials": args.trials, "repeats": args.repeats, "capacity": args.capacity,
              "min_features": args.min_features, "device": torch.cuda.get_device_name(0),
              "pictures": "tests/sift_cases.pair(H, W, 0, noise=True) detected once with nfeatures = 2048; pair p is (reference, estimate) with the key (p, p + 1)",
              "keypoints": [int(counts[0, 2]), int(counts[1, 2])],
              "times": "milliseconds between device events: median [min, max] over the repeats, every stage alone"}
    for count in (1, args.batch):
        pictures = [(0, 1)] * count
        keys = torch.tensor([(p, p + 1) for p in range(count)], dtype=torch.int32).cuda()
        pairs = torch.tensor(pictures, dtype=torch.int32).cuda()
        rows, pair_counts = features.match_pairs(feats, pairs, depth, 0.7, args.min_features)
        H, mask, res = features.ransac_homography(rows, pair_counts[:, 1], keys, 3.0, args.trials, 0, args.min_features)
        match = timed(lambda: features.match_pairs(feats, pairs, depth, 0.7, args.min_features), args.repeats)
        ransac = timed(lambda: features.ransac_homography(rows, pair_counts[:, 1], keys, 3.0, args.trials, 0, args.min_features), args.repeats)
        compact = timed(lambda: features.compact_pairs(rows, pair_counts, mask, res, args.min_features), args.repeats)
        pc, res_h = pair_counts.cpu().numpy(), res.cpu().numpy()
        result["one_pair" if count == 1 else f"{count}_pairs"] = {
            "match_ms": match[0], "match_min_max_ms": match[1:], "match_per_pair_ms": round(match[0] / count, 4),
            "ransac_ms": ransac[0], "ransac_min_max_ms": ransac[1:], "ransac_per_pair_ms": round(ransac[0] / count, 4),
            "compact_ms": compact[0], "compact_min_max_ms": compact[1:],
            "ratio_survivors": int(pc[0, 0]), "survivors": int(pc[0, 1]), "inliers_min": int(res_h[:, 2].min()), "inliers_max": int(res_h[:, 2].max()),
            "distinct_winning_trials": int(len(set(res_h[:, 0].tolist())))}
        # what is timed is what the tests check: the first pair against the restatement, bit for bit
        kps, desc = feats[0].cpu().numpy(), feats[1].cpu().numpy()
        t0 = time.perf_counter()
        want = RR.match_filter(kps[0, :counts[0, 2]], desc[0, :counts[0, 2]], kps[1, :counts[1, 2]], desc[1, :counts[1, 2]], depth_h[0], depth_h[1], 0.7, args.min_features)
        t1 = time.perf_counter()
        n = want["survivors"]
        got = rows[0, :n].cpu().numpy()
        assert pc[0].tolist() == [want["ratio_survivors"], n] and got[:, 0:2].tobytes() == want["points_i"].tobytes() and got[:, 2:4].tobytes() == want["points_j"].tobytes()
        t2 = time.perf_counter()
        fit = RR.ransac(want["points_i"], want["points_j"], 3.0, args.trials, 0, (0, 1), min_count=args.min_features)
        t3 = time.perf_counter()
        assert res_h[0].tolist() == [fit["trial"], fit["winner_count"], fit["count"]] and H[0].cpu().numpy().tobytes() == fit["H"].tobytes()
        assert (mask[0, :n].cpu().numpy() == fit["mask"]).all()
        result["restatement_host_seconds_one_pair"] = {"filter": round(t1 - t0, 3), "ransac": round(t3 - t2, 3)}
        result["first_pair_matches_the_restatement_bit_for_bit"] = True
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    sift.close()
