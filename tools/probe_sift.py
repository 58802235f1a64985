"""Timings of MIFD (hive_amd.features: SIFT, the exact matcher, the score; csrc/sift.hip) at 640 x 480 on the MI355X (not gated by any test; there is no earlier
number to beat, so no threshold; DESIGN.md section 5.14 records the figures).  Two sets of gray pictures resident on the device: frames of the
benchmark's synthetic room (hive_amd.synthetic.make_sequence; pair k is frames k and k + 1; smooth walls, so few keypoints), and the keypoint-rich blob pair of
tests/sift_cases.py at the same size, repeated in every slot.

  * one pair and --batch pairs: the whole of detect + match + score between device events after warm-up, the median over --repeats calls with the minimum and
    the maximum beside it, each call with its copy back of the counts and the scores;
  * the split: the same call stopped after the pyramid and after the sorted keypoints (hive_sift_set_last_stage), and the match alone; a stage is the
    difference of two medians, so the parts carry the spread of both;
  * for orientation only, the host time of tests/sift_restatement.py on the first pair of each set (numpy, one core).

It asserts what it times: the first pair's score and match count of each set against the restatement, bit for bit.  Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys
import time
import warnings

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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--capacity", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sift_restatement as R
    from hive_amd import features, synthetic
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    import sift_cases
    seq = synthetic.make_sequence(num_frames=args.batch + 1, height=args.height, width=args.width)
    color = np.asarray(seq["color"]).astype(np.int64)
    room = ((1868 * color[..., 0] + 9617 * color[..., 1] + 4899 * color[..., 2] + 8192) >> 14).astype(np.uint8)
    blob_ref, blob_est = sift_cases.pair(args.height, args.width, 0, True)
    workloads = {"room": (room[:-1], room[1:], "frames k and k + 1 of hive_amd.synthetic.make_sequence, the benchmark's room (smooth walls: few keypoints)"),
                 "blobs": (np.stack([blob_ref] * args.batch), np.stack([blob_est] * args.batch),
                           "tests/sift_cases.pair(H, W, 0, noise=True), the same pair in every slot (keypoint-rich)")}
    sift = features.SIFT(capacity=args.capacity)
    ctx = sift._context(torch.device("cuda", 0))
    result = {"height": args.height, "width": args.width, "batch": args.batch, "repeats": args.repeats, "capacity": args.capacity,
              "device": torch.cuda.get_device_name(0),
              "times": "milliseconds between device events: median [min, max] over the repeats; pyramid / detect / describe are differences of medians"}
    for name, (refs, ests, what) in workloads.items():
        result[name] = {"pictures": what}
        for count in (1, args.batch):
            pictures = torch.from_numpy(np.concatenate([refs[:count], ests[:count]])).cuda()

            def run(stage):
                found = sift.detect_device(pictures, None, ctx)
                scored = features.score_pairs(sift, found, 0, count, count, ctx) if stage == 3 else None
                counts = found[2].cpu().numpy()  # the copy back a caller needs anyway
                return found, counts, (scored[0].cpu().numpy(), scored[1].cpu().numpy()) if scored else None
            found, counts, scored = run(3)
            sift.check_counts(counts)
            handle = sift._last[1]
            whole = timed(lambda: run(3), args.repeats)
            medians = {}
            for stage_name, stage in (("pyramid", 1), ("keypoints", 2), ("descriptors", 0)):
                ctx.check(ctx.lib.hive_sift_set_last_stage(handle, stage))
                medians[stage_name] = timed(lambda: run(stage), args.repeats)
            ctx.check(ctx.lib.hive_sift_set_last_stage(handle, 0))
            match = timed(lambda: features.score_pairs(sift, found, 0, count, count, ctx)[0].cpu(), args.repeats)
            result[name]["one_pair" if count == 1 else f"{count}_pairs"] = {
                "whole_ms": whole[0], "whole_min_max_ms": whole[1:], "per_pair_ms": round(whole[0] / count, 4),
                "pyramid_ms": medians["pyramid"][0], "detect_ms": round(medians["keypoints"][0] - medians["pyramid"][0], 4),
                "describe_ms": round(medians["descriptors"][0] - medians["keypoints"][0], 4), "match_ms": match[0],
                "cumulative_min_max_ms": {k: v[1:] for k, v in medians.items()}, "match_min_max_ms": match[1:],
                "keypoints_per_picture_mean": round(float(counts[:, 2].mean()), 1), "keypoints_per_picture_max": int(counts[:, 2].max()),
                "candidates_per_picture_max": int(counts[:, 0].max()), "matches_mean": round(float(scored[1].mean()), 1),
                "first_pair_mifd": float(scored[0][0]), "first_pair_matches": int(scored[1][0])}
        # what is timed is what the tests check: the first pair against the restatement, bit for bit
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = R.mifd(refs[0], ests[0], with_matches=True)
        result[name]["restatement_host_seconds_first_pair"] = round(time.perf_counter() - t0, 2)
        for key in ("one_pair", f"{args.batch}_pairs"):
            got = result[name][key]
            assert np.float64(got["first_pair_mifd"]).tobytes() == np.float64(want[0]).tobytes() and got["first_pair_matches"] == want[1], (name, key, got, want)
        result[name]["first_pair_matches_the_restatement_bit_for_bit"] = True
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    sift.close()
