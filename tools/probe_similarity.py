"""Timings of the picture scores (hive_amd.evaluation.image_similarity, csrc/similarity.hip) at 640 x 480 on the MI355X (not gated by any test; DESIGN.md section
5.11 records the figures):

  * one pair and 64 pairs, plain and masked together (what compare_renders asks for), with and without MS-SSIM, device-resident pictures, between device events
    after warm-up: the median over --repeats calls, each call with its one copy back of the scores;
  * the numpy / torch-CPU restatement of the same rules (tests/similarity_restatement.py) for one pair, plain and masked, on the same box, and the ratio.

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


def _time_device(ref, est, ms_ssim, repeats, warmup=5):
    import torch
    from hive_amd.evaluation import image_similarity
    samples = []
    for i in range(repeats + warmup):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = image_similarity(ref, est, ms_ssim=ms_ssim, mask_background=True)
        stop.record()
        stop.synchronize()
        if i >= warmup:
            samples.append(start.elapsed_time(stop))
    return _median_ms(samples), out


def _time_host(ref, est, ms_ssim, repeats):
    import similarity_restatement as SR
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for frame in (ref, SR.mask_background(ref, est)):
            out = SR.compare(frame, est)
            if ms_ssim:
                out["ms_ssim"] = SR.ms_ssim(frame, est)
        samples.append(1e3 * (time.perf_counter() - t0))
    return _median_ms(samples), out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import similarity_restatement as SR
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    pairs = [SR.smooth_pair(args.height, args.width, seed=k, whites=2000) for k in range(args.batch)]
    ref = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    est = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    result = {"height": args.height, "width": args.width, "batch": args.batch, "repeats": args.repeats, "variants": "plain and masked in one call",
              "device": torch.cuda.get_device_name(0)}
    for ms in (False, True):
        key = "ssim_psnr_msssim" if ms else "ssim_psnr"
        one_ms, one = _time_device(ref[:1], est[:1], ms, args.repeats)
        many_ms, many = _time_device(ref, est, ms, args.repeats)
        host_ms, host = _time_host(pairs[0][0], pairs[0][1], ms, args.host_repeats)
        assert one.ssim_masked[0] == many.ssim_masked[0] == host["ssim"] and one.psnr_masked[0] == host["psnr"], "the probe times what the tests check"
        if ms:
            assert abs(many.ms_ssim_masked[0] - host["ms_ssim"]) <= 1e-9
        result[key] = {"one_pair_ms": one_ms, f"{args.batch}_pairs_ms": many_ms, f"per_pair_in_{args.batch}_ms": round(many_ms / args.batch, 4),
                       "host_restatement_one_pair_ms": host_ms, "host_over_device_one_pair": round(host_ms / one_ms, 1),
                       f"host_over_device_per_pair_in_{args.batch}": round(host_ms / (many_ms / args.batch), 1)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
