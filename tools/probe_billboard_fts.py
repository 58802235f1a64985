"""Timings of the two foreground stages behind --billboard and --fts_num_epochs on the MI355X (not gated by any test; DESIGN_LOG.md records the figures):

  * the billboard call (hive_fg_billboard + the second hive_texture_window) per object at 640 x 480, next to frame_mesh without it;
  * hive_fts_optimise for 1000 frames x 100 epochs (one launch) next to the same loop written with torch operators on the same GPU.

Warm-up, then several repeats with the two sides alternating; every timed window ends in a device synchronise.  Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(samples):
    return round(1e3 * float(np.median(samples)), 4)


def billboard_timings(repeats=30):
    import torch
    from hive_amd import _lib, foreground, synthetic
    h, w = 480, 640
    seq = synthetic.make_sequence(num_frames=1, height=h, width=w, yaw_step_deg=2.4)
    masks = synthetic.ellipse_masks(1, h, w, num_objects=3, seed=3)[0]
    pose = np.linalg.inv(seq["poses"][0])
    R, t, K = pose[:3, :3], pose[:3, 3:4], seq["K"]
    ctx = _lib.default_context(0)
    depth, img = torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(seq["color"][0]).cuda()
    buffers = foreground.FrameMeshBuffers(h, w)
    out = {}
    for name, mask in [("object %d" % k, torch.from_numpy(masks == k).cuda()) for k in (1, 2, 3)] + [("whole frame", None)]:
        plain, flat = [], []
        for i in range(repeats + 5):
            for bucket, on in ((plain, False), (flat, True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                mesh = foreground.frame_mesh(depth, mask, img, K, R, t, ctx=ctx, buffers=buffers, billboard=on)
                torch.cuda.synchronize()
                if i >= 5:
                    bucket.append(time.perf_counter() - t0)
        out[name] = {"vertices": int(mesh["vertices"].shape[0]), "frame_mesh_ms": _median_ms(plain), "frame_mesh_billboard_ms": _median_ms(flat),
                     "billboard_ms": round(_median_ms(flat) - _median_ms(plain), 4)}
    return out


def _torch_loop(start, centroids, chunks, lr, epochs, device):
    """The reference's loop with torch operators on ``device``, float64 parameters (the formulation of tests/fts_restatement.py)."""
    import torch

    def hamilton(a, b):
        ax, ay, az, aw = a.unbind(1)
        bx, by, bz, bw = b.unbind(1)
        return torch.stack((aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                            aw * bw - ax * bx - ay * by - az * bz), dim=1)

    sign = torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=torch.float64, device=device)

    def world(q, t, c):
        n = q / torch.linalg.norm(q, dim=1, keepdim=True)
        v = c - t
        return hamilton(hamilton(n * sign, torch.cat((v, torch.zeros_like(v[:, :1])), dim=1)), n)[:, :3]

    p = torch.tensor(start, device=device)
    q, t = torch.nn.Parameter(p[:, :4].clone()), torch.nn.Parameter(p[:, 4:].clone())
    c = torch.tensor(centroids, device=device)
    optimiser = torch.optim.Adam([q, t], lr=lr, weight_decay=1e-4)
    with torch.no_grad():
        gt = world(q, t, c)
    index = [torch.arange(s, s + m, device=device) for s, m in chunks]
    for _ in range(epochs):
        optimiser.zero_grad()
        loss = torch.zeros((), dtype=torch.float64, device=device)
        for chunk in index:
            tc = t[chunk]
            loss = loss + (0.01 * torch.mean(torch.norm(gt[chunk] - world(q[chunk], tc, c[chunk]), dim=1)) + 0.1 * torch.norm(tc[:-2] - 2 * tc[1:-1] + tc[2:])
                           + 0.1 * torch.norm(tc[:-1] - tc[1:]))
        loss.backward()
        optimiser.step()
    return torch.cat((q.detach(), t.detach()), dim=1)


def fts_timings(frames=1000, epochs=100, repeats=7):
    import torch
    from scipy.spatial.transform import Rotation
    from hive_amd import _lib, pose_optimisation
    rng = np.random.default_rng(0)
    s = np.linspace(0.0, 1.0, frames)
    quats = Rotation.from_euler("xyz", np.stack([0.3 * s, 0.2 * np.sin(2 * s), 0.1 * s], 1) + 0.01 * rng.standard_normal((frames, 3))).as_quat()
    positions = np.stack([0.5 * s, 0.1 * np.sin(3 * s), 0.3 * s * s], 1) + 0.005 * rng.standard_normal((frames, 3))
    start = np.hstack((quats, positions)).astype(np.float32).astype(np.float64)
    centroids = np.stack([0.4 * np.cos(4 * s), 0.3 * np.sin(5 * s), 2.5 + 0.5 * s], 1) + 0.02 * rng.standard_normal((frames, 3))
    counts = np.ones(frames, np.int64)
    counts[rng.permutation(frames)[:frames // 50]] = 0  # about twenty chunks
    chunks = pose_optimisation.find_chunks(counts)
    ctx = _lib.default_context(0)
    kernel, operators = [], []
    for i in range(repeats + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got, _ = pose_optimisation.fts_optimise(start, centroids, chunks, 1e-5, epochs, ctx=ctx)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        want = _torch_loop(start, centroids, chunks, 1e-5, epochs, "cuda")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            kernel.append(t1 - t0)
            operators.append(t2 - t1)
    return {"frames": frames, "epochs": epochs, "chunks": len(chunks), "hive_fts_optimise_ms": _median_ms(kernel), "torch_operators_same_gpu_ms": _median_ms(operators),
            "max_abs_difference": float(np.abs(got - want.cpu().numpy()).max())}


if __name__ == "__main__":
    print(json.dumps({"billboard_640x480": billboard_timings(), "trajectory_smoothing": fts_timings()}, indent=1))
