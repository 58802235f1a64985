"""Timings of LPIPS (hive_amd.evaluation.LPIPS, csrc/lpips.hip) at 640 x 480 on the MI355X with seeded weights (not gated by any test; DESIGN.md section 5.12
records the figures):

  * one pair and 64 pairs, plain and masked together (three pictures a pair: the frame, the whitened frame, the render), device-resident pictures, between device
    events after warm-up: the median over --repeats calls, each call with its one copy back of the scores;
  * beside each, alternating with it, the same network through torch's own operators on the same device: the float32 formulation of
    tests/lpips_restatement.py moved to the GPU, which is what the reference's lpips_fn runs;
  * the achieved fraction of the 157 TFLOP/s float32-matrix peak, from the FLOPs the layer list executes (computed from the shapes below), over the whole call.

It asserts what it times: the first pair's scores against the float64 restatement, within the tests' bound (64 x the float32 torch-CPU formulation's own
distance).  Prints one JSON object; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32_MATRIX_PEAK = 157e12


def flops_per_picture(h, w):
    """2 K C_out per output pixel of every row."""
    import lpips_restatement as LR
    return sum(2 * cin * k * k * cout * fh * fw for (cin, cout, k, _, _, _), (fh, fw) in zip(LR.LAYERS, LR.feature_sizes(h, w)))


class TorchOperators:
    """lpips_restatement.score_f32 for a batch, plain and masked, on the device."""

    def __init__(self, model, dev):
        import torch
        import lpips_restatement as LR
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.conv = [(t(model.conv_w[l]), t(model.conv_b[l]), LR.LAYERS[l]) for l in range(5)]
        self.lin = [t(model.lin_w[l]).reshape(1, -1, 1, 1) for l in range(5)]
        self.shift = torch.tensor(LR.SHIFT, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
        self.scale = torch.tensor(LR.SCALE, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)

    def __call__(self, ref, est):
        import torch
        import torch.nn.functional as F
        n = ref.shape[0]
        pictures = torch.cat([ref, torch.where(est == 255, est, ref), est]).permute(0, 3, 1, 2)
        x = (((pictures.double() / 255) * 2.0 - 1.0).float() - self.shift) / self.scale
        total = None
        for (w, b, (_, _, _, stride, pad, pool)), lin in zip(self.conv, self.lin):
            if pool:
                x = F.max_pool2d(x, kernel_size=3, stride=2)
            x = torch.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
            unit = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            diff = (unit[:2 * n] - unit[2 * n:].repeat(2, 1, 1, 1)) ** 2
            value = F.conv2d(diff, lin).mean([2, 3])
            total = value if total is None else total + value
        return total.reshape(2, n).cpu().numpy()  # the copy back of the scores


def time_alternating(calls, repeats, warmup=5):
    """Median milliseconds of each call, the calls taking turns."""
    import torch
    samples = [[] for _ in calls]
    outs = [None] * len(calls)
    for i in range(repeats + warmup):
        for which, call in enumerate(calls):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            outs[which] = call()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                samples[which].append(start.elapsed_time(stop))
    return [round(float(np.median(s)), 4) for s in samples], outs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import lpips_restatement as LR
    import similarity_restatement as SR
    from hive_amd.evaluation import LPIPS
    assert torch.cuda.is_available(), "the probe measures the GPU: no device, no number"
    model = LPIPS.seeded(1)
    pairs = [SR.smooth_pair(args.height, args.width, seed=k, whites=2000) for k in range(args.batch)]
    ref = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    est = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    operators = TorchOperators(model, ref.device)
    flops = flops_per_picture(args.height, args.width)
    result = {"height": args.height, "width": args.width, "batch": args.batch, "repeats": args.repeats, "variants": "plain and masked in one call",
              "device": torch.cuda.get_device_name(0), "gflop_per_picture": round(flops / 1e9, 3), "pictures_per_pair": 3,
              "f32_matrix_peak_tflops": F32_MATRIX_PEAK / 1e12}
    # what is timed is what the tests check: the first pair against the float64 restatement
    frame, render = pairs[0]
    want, yardstick = [], 0.0
    for f in (frame, LR.mask_background(frame, render)):
        s64, s32 = LR.score(f, render, model)[0], LR.score_f32(f, render, model)[0]
        want.append(s64)
        yardstick = max(yardstick, abs(s32 - s64) / s64)
    for count in (1, args.batch):
        (hip_ms, torch_ms), (hip_out, torch_out) = time_alternating(
            [lambda: model(ref[:count], est[:count], mask_background=True), lambda: operators(ref[:count], est[:count])], args.repeats)
        got = (hip_out.lpips[0], hip_out.lpips_masked[0])
        distance = max(abs(g - w) / w for g, w in zip(got, want))
        assert distance <= 64 * yardstick, (got, want, yardstick)
        torch_distance = max(abs(float(torch_out[v, 0]) - w) / w for v, w in enumerate(want))
        executed = flops * 3 * count
        result["one_pair" if count == 1 else f"{count}_pairs"] = {
            "hip_ms": hip_ms, "torch_operators_ms": torch_ms, "torch_over_hip": round(torch_ms / hip_ms, 3), "hip_per_pair_ms": round(hip_ms / count, 4),
            "hip_tflops_over_the_call": round(executed / (hip_ms * 1e-3) / 1e12, 2), "hip_fraction_of_f32_matrix_peak": round(executed / (hip_ms * 1e-3) / F32_MATRIX_PEAK, 4),
            "first_pair_relative_distance_from_float64": float(f"{distance:.3g}"), "torch_operators_relative_distance_from_float64": float(f"{torch_distance:.3g}"),
            "yardstick_float32_torch_cpu": float(f"{yardstick:.3g}")}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
