"""Milliseconds per epoch of the pose optimiser on the MI355X (not gated by any test; README.md and DESIGN.md §5.16 quote profiles/pose_optimiser_probe.json):

  * hive_pose_optimise (two launches an epoch, scheduler and early stop on the device, one read-back per check_every epochs) at 800 frames with hierarchical
    pairs, for 1e5 and 1e6 correspondences, World3D residuals, Rigid alignment, smoothing terms on, no clip;
  * the same epoch written with torch operators on the same GPU, the way the reference writes it: the restatement's loss (tests/pose_optimiser_restatement.py) in
    float32, autograd, torch.optim.Adam, ReduceLROnPlateau fed with the loss read back every epoch.

Both sides run the same number of epochs (patiences too large to stop), after a warm-up; every timed window ends in a device synchronise.  The setup of
hive_pose_optimise -- the index read-back, the incidence lists on the host, the widening pass -- is inside its window and also reported alone (num_epochs = 0).
Not measured: Image2D, Affine, the clip with steps to clip, other frame counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _case(frames, matches):
    import pose_optimiser_restatement as R
    pairs = R.hierarchical_pairs(frames)
    return R.make_case(n=frames, counts=(max(1, matches // len(pairs)),), skip_frames=(), walk_t=0.002, walk_r=0.002, turn=0.02)  # a slow turn: every point stays in front of every camera


def _torch_epochs(case, epochs, device="cuda"):
    """The reference's way: small torch operators, autograd, one loss read-back an epoch; float32 parameters on the GPU."""
    import torch
    import pose_optimiser_restatement as R
    data = {k: (v.to(device) if hasattr(v, "to") else v) for k, v in R.tensors_of(case).items()}
    start = torch.tensor(case["start"]).to(device)
    q, t = torch.nn.Parameter(start[:, :4].clone()), torch.nn.Parameter(start[:, 4:].clone())
    one, zero = torch.ones(len(start), device=device), torch.zeros(len(start), device=device)
    optimiser = torch.optim.Adam([q, t], lr=1e-2)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimiser, patience=10 ** 6, mode="min", threshold=1e-4, threshold_mode="abs")
    for _ in range(epochs):
        with torch.no_grad():
            q.copy_(q / torch.linalg.norm(q, ord=2, dim=1, keepdim=True))
        optimiser.zero_grad()
        value = R.loss(q, t, one, zero, data)
        value.backward()
        q.grad[0] = 0.0
        t.grad[0] = 0.0
        optimiser.step()
        scheduler.step(value)
        value.detach().cpu().item()
    return torch.cat((q, t), dim=1).detach()


def timings(frames, matches, epochs, repeats):
    import torch
    import pose_optimiser_restatement as R
    from hive_amd import _lib, pose_optimisation as P
    case = _case(frames, matches)
    side = lambda s: P.FeatureData(torch.from_numpy(case["index_" + s]), torch.from_numpy(case["points_" + s]), torch.from_numpy(case["depth_" + s]))
    fs = P.FeatureSet(torch.from_numpy(R.camera_matrix(case)), side("i"), side("j")).to("cuda")
    params = P.OptimisationParameters(case["start"].astype(np.float64), P.AlignmentType.Rigid)
    options = P.OptimisationOptions(num_epochs=epochs, lr_scheduler_patience=10 ** 6, early_stopping_patience=10 ** 6, clip_distance=None)
    ctx = _lib.default_context(0)
    kernel, setup, operators = [], [], []
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got, _, _, ran = P.optimise_poses(fs, params, options, ctx=ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        P.optimise_poses(fs, params, options, num_epochs=0, ctx=ctx)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        want = _torch_epochs(case, epochs)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert ran == epochs
        if i >= 2:
            kernel.append(t1 - t0)
            setup.append(t2 - t1)
            operators.append(t3 - t2)
    k, s, o = (float(np.median(v)) for v in (kernel, setup, operators))
    return {"frames": frames, "correspondences": len(fs), "pairs": len(case["pairs"]), "epochs": epochs,
            "hive_pose_optimise_ms_per_epoch": round(1e3 * (k - s) / epochs, 4), "hive_pose_optimise_setup_ms": round(1e3 * s, 3),
            "torch_operators_same_gpu_ms_per_epoch": round(1e3 * o / epochs, 4),
            "max_abs_difference_float64_kernel_vs_float32_operators": float(np.abs(got.poses() - want.cpu().numpy().astype(np.float64)).max())}


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_optimiser_probe.json"))
    parser.add_argument("--epochs", type=int, default=200)
    parser.add_argument("--repeats", type=int, default=3)
    args = parser.parse_args()
    result = {"device": "MI355X", "residuals": "World3D", "alignment": "Rigid", "smoothing_terms": True, "clip": None,
              "cases": [timings(800, m, args.epochs, args.repeats) for m in (100_000, 1_000_000)]}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))
