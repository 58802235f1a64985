#!/usr/bin/env python3
"""Records the bits of the float64 sums that no restatement holds bit for bit -- the ICP normal equations (csrc/track.hip), the trajectory smoothing
(csrc/fts.hip), the pose optimiser (csrc/poseopt.hip) and the layer means of LPIPS (csrc/lpips.hip: tests/test_lpips_gpu.py holds the per-pixel distances bit
for bit but their tree sum within 1e-10) -- into tests/golden/sum_pins.npz, with the commit they were taken at.  tests/test_sum_pins_gpu.py
compares ``compute()`` with the file as uint64 views: a change to the order of a sum shows as a changed bit.  Run on the commit whose bits are to be kept,
on an MI355X, with the library built: python tools/record_sum_pins.py

No recorded quantity passes through a library function other than sqrt on the device (sqrt and / are correctly rounded; the kernels are built without
contraction), so the pins hold for any compiler that keeps the stated operation order.  The INPUTS are made on the host with numpy and scipy."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "tests"), ROOT):
    if path not in sys.path:
        sys.path.insert(0, path)

PINS = os.path.join(ROOT, "tests", "golden", "sum_pins.npz")
POSE_ROWS = [0, 1, 63, 64, 149, 255, 256, 299]


def icp_pins(ctx, oracle):
    """``tracking.icp_step`` on the corner scene at (24, 32) and (47, 63), both poses of test_icp_step_sums_and_pairs: one and twelve workgroups."""
    import torch
    import tracking_restatement as tr
    from hive_amd import tracking
    out = {}
    for H, W, voxels in ((24, 32, 32), (47, 63, 64)):
        s = tr.icp_scene(oracle, H, W, voxels)
        dist, cos_min = 2 * s["vol"]._trunc_margin, float(np.cos(np.deg2rad(20.0)))
        dev = [torch.from_numpy(s[k]).cuda() for k in ("live_v", "live_n", "model_v", "model_n")]
        for name, est in (("start", s["orbit"][0]), ("goal", s["orbit"][1])):
            sums, pairs = tracking.icp_step(ctx, s["K"], *dev, s["orbit"][0], est, dist, cos_min)
            out[f"icp_{H}x{W}_{name}"] = np.append(sums, float(pairs))
    return out


def fts_pins(ctx):
    """``fts_optimise`` over 70 frames in the chunks (0, 3) and (3, 67): the second is longer than a wave."""
    import fts_restatement as F
    from hive_amd import pose_optimisation
    traj, centroids, _ = F.jittery_case(num_frames=70, seed=3, empty=())
    params, losses, grad = pose_optimisation.fts_optimise(traj.astype(np.float64), centroids, [(0, 3), (3, 67)], num_epochs=3, return_gradient=True, ctx=ctx)
    return {"fts_params": params, "fts_losses": losses, "fts_gradient": grad}


def pose_case(n):
    """The case builder of the pose optimiser tests with positions and depths spread over several binades."""
    import pose_optimiser_restatement as R
    return R.make_case(n=n, seed=5, skip_frames=(), depth_range=(0.25, 16.0), walk_t=0.003, turn=min(1.0, 9.0 / n))


def pose_pins(ctx):
    """``optimise_poses`` at 5 and at 300 frames (more frames than the 256 threads that add the loss shares), both residual types, Rigid and Affine."""
    import torch
    import pose_optimiser_restatement as R
    from hive_amd import pose_optimisation as P
    out = {}
    for n in (5, 300):
        case = pose_case(n)
        side = lambda s: P.FeatureData(torch.from_numpy(case["index_" + s]), torch.from_numpy(case["points_" + s]), torch.from_numpy(case["depth_" + s]))
        feature_set = P.FeatureSet(torch.from_numpy(R.camera_matrix(case)), side("i"), side("j")).to("cuda")
        rng = np.random.default_rng(3)
        scale, shift = 1.0 + 0.05 * rng.standard_normal(n), 0.01 * rng.standard_normal(n)
        for residual in (P.ResidualType.World3D, P.ResidualType.Image2D):
            for affine in (False, True):
                poses = case["start"].astype(np.float64)
                params = P.OptimisationParameters(poses, P.AlignmentType.Affine, scale, shift) if affine else P.OptimisationParameters(poses, P.AlignmentType.Rigid)
                got, losses, rates, ran, loss, grad = P.optimise_poses(feature_set, params, P.OptimisationOptions(), residual, True, fps=case["fps"], num_epochs=3,
                                                                       return_gradient=True, ctx=ctx)
                key = f"pose_{n}_{residual.name}_{'affine' if affine else 'rigid'}"
                rows = POSE_ROWS if n > len(POSE_ROWS) else slice(None)  # the long case keeps a few frames: every frame's sum is a workgroup of its own
                out[key + "_poses"], out[key + "_losses"], out[key + "_loss"], out[key + "_gradient"] = got.poses()[rows], losses, np.array([loss]), grad[rows]
                if affine:
                    out[key + "_scale"], out[key + "_shift"] = np.asarray(got.scale, np.float64)[rows], np.asarray(got.shift, np.float64)[rows]
    return out


def lpips_pins(ctx):
    """``LPIPS.seeded(1)`` on two seeded 67 x 131 pairs, plain and masked: 512 pixels in the first layer (two workgroups of the tail kernel), 21 in the last."""
    from hive_amd.evaluation import LPIPS
    rng = np.random.default_rng(23)
    ref, est = (rng.integers(0, 256, (2, 67, 131, 3), dtype=np.uint8) for _ in range(2))
    est[:, ::5, ::3, 1] = 255  # single channels at 255: the masked variant differs
    model = LPIPS.seeded(1)
    got = model(ref, est, mask_background=True, ctx=ctx)
    model.close()
    return {"lpips_layers": got.layers, "lpips_layers_masked": got.layers_masked, "lpips": got.lpips, "lpips_masked": got.lpips_masked}


def compute(ctx, oracle):
    """name -> float64 array, every pinned quantity."""
    out = {}
    for part in (icp_pins(ctx, oracle), fts_pins(ctx), pose_pins(ctx), lpips_pins(ctx)):
        out.update({k: np.ascontiguousarray(v, dtype=np.float64) for k, v in part.items()})
    return out


def main():
    import oracle
    from hive_amd import _lib
    oracle.build()
    # the commit: the first argument (a tree without its history), else git's HEAD
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    pins = compute(_lib.default_context(0), oracle)
    np.savez_compressed(PINS, commit=np.array(commit), **pins)
    print(f"{PINS}: {len(pins)} arrays, {sum(v.size for v in pins.values())} numbers, {os.path.getsize(PINS)} bytes, commit {commit}")


if __name__ == "__main__":
    main()
