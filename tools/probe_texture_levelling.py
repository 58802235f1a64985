"""Timings of the exposure gains and the seam levelling of background texturing (hive_amd.texturing.texture_mesh with ``exposure`` / ``levelling``,
csrc/texture_level.hip) on the MI355X (not gated by any test; DESIGN.md and the README record the figures; writes profiles/texture_levelling_probe.json):

  * the mesh of the synthetic room the benchmark fuses (--frames frames into a volume of --voxel metres: about 730 k faces) textured from 8 and from 32 key frames
    at 640 x 480 with cell 8, everything device-resident; the key frames are multiplied per channel by factors that cycle through three exposures, so that the
    gains have something to find;
  * the wall time of the whole texture_mesh call plain, with ``exposure``, with ``levelling`` at --sweeps, and with both, in the same session;
  * per stage between HIP events: hive_texture_samples for one view, hive_texture_exposure_sums (with its read-back), the host solve (wall time),
    hive_texture_level at 0 sweeps and at --sweeps (their difference is the sweeps), hive_texture_fill_adjusted beside hive_texture_fill;
  * the gains' spread, the pair counts' range, seam vertices and the largest offset.

Medians of 9 after 2 warm-up runs; every timed window ends in a device synchronise.  Not measured here: a real capture, a viewer that filters bilinearly, more
than 32 views."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from probe_texturing import _events, _median_ms, _wall, REPEATS, WARMUP  # noqa: E402

FACTORS = ((0.85, 0.80, 0.90), (1.0, 1.0, 1.0), (1.15, 1.20, 1.10))


def stages(mesh, frames, K, poses, cell, sweeps):
    """The calls texture_mesh adds on its adjusted path, stage by stage, on device-resident inputs."""
    import torch
    from hive_amd import _lib, texturing
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers
    ctx = _lib.default_context(0)
    lib, handle = ctx.lib, ctx.handle
    v, f, c = mesh["vertices"], mesh["faces"], mesh["vertex_colors"]
    nv, nf = v.shape[0], f.shape[0]
    n, h, w = frames.shape[:3]
    buffers = RenderBuffers(h, w)
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    area = torch.empty((n, nf), dtype=torch.int64, device="cuda")
    samples = torch.empty((n, nf, 3), dtype=torch.int16, device="cuda")

    def view(k, sample=True):
        R, t = np.ascontiguousarray(poses[k, :3, :3]), np.ascontiguousarray(poses[k, :3, 3])
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
        ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), h, w, 0.05, ptr(xy), ptr(z), ptr(large), ptr(counts), ptr(buffers.key)))
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, None, None, ptr(depth), None))
        ctx.check(lib.hive_texture_vote(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), None, h, w, k, 0.05, 0, ptr(area)))
        if sample:
            ctx.check(lib.hive_texture_samples(handle, ptr(f), nf, nv, ptr(xy), ptr(area), ptr(frames[k]), h, w, k, ptr(samples)))

    for k in range(n):
        view(k)
    out = {"samples_one_view_ms": _events(lambda: ctx.check(lib.hive_texture_samples(handle, ptr(f), nf, nv, ptr(xy), ptr(area), ptr(frames[n - 1]), h, w, n - 1,
                                                                                      ptr(samples)))),
           "exposure_sums_ms": _events(lambda: texturing.exposure_sums(samples, ctx=ctx)), "samples_bytes": int(samples.numel() * 2)}
    G, D, N = texturing.exposure_sums(samples, ctx=ctx)
    solve = []
    for i in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        q, fallback = texturing.solve_gains(G, D, 0.01)
        if i >= WARMUP:
            solve.append(time.perf_counter() - t0)
    out["solve_gains_host_ms"] = _median_ms(solve)
    off = N[~np.eye(n, dtype=bool)]
    out["pair_counts_min_max"] = [int(off.min()), int(off.max())]
    out["gains_min_max"] = [float(q.min() / 65536.0), float(q.max() / 65536.0)]
    out["fallback_channels"] = fallback
    labels = texturing.texture_mesh(mesh, frames, K, poses, cell=cell, return_views=True)["views"]
    level = lambda s: texturing.level_offsets(mesh, labels, frames, K, poses, q, s, ctx=ctx)
    out["level_0_sweeps_ms"], out[f"level_{sweeps}_sweeps_ms"] = _events(lambda: level(0)), _events(lambda: level(sweeps))
    out["one_sweep_ms"] = round((out[f"level_{sweeps}_sweeps_ms"] - out["level_0_sweeps_ms"]) / max(1, sweeps), 5)
    offsets, out["levelling"] = level(sweeps)
    out["offsets_bytes"] = int(offsets.numel() * 8)
    best = torch.where(labels >= 0, (1 << 16) | (65535 - labels.to(torch.int64)), torch.zeros_like(labels, dtype=torch.int64)).contiguous()
    d_q = torch.from_numpy(q.view(np.int32)).cuda()
    d_poses = torch.from_numpy(np.ascontiguousarray(np.concatenate([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3]], axis=1))).cuda()
    wt, ht, _ = texturing.atlas_layout(nf, cell)
    atlas = torch.empty((ht, wt, 3), dtype=torch.uint8, device="cuda")
    args = (handle, ptr(v), nv, ptr(c), ptr(f), nf, ptr(best), ptr(frames), n, h, w, ptr(K), ptr(d_poses), 0.05, cell)
    out["fill_ms"] = _events(lambda: ctx.check(lib.hive_texture_fill(*args, ptr(atlas))))
    out["fill_adjusted_ms"] = _events(lambda: ctx.check(lib.hive_texture_fill_adjusted(*args, ptr(d_q), ptr(offsets), ptr(atlas))))
    return out


def room(frames_fused, voxel, cell, sweeps):
    import torch
    from hive_amd import _lib, fusion, synthetic, texturing
    h, w = 480, 640
    seq = synthetic.make_sequence(num_frames=32, height=h, width=w, yaw_step_deg=360.0 / 32)
    vol = fusion.TSDFVolume(synthetic.room_bounds(), voxel, ctx=_lib.default_context(0))
    for i in np.linspace(0, 31, frames_fused).round().astype(int):
        vol.integrate(seq["color"][i], seq["depth"][i], seq["K"], seq["poses"][i])
    verts, faces, _, colors = vol.get_mesh()
    mesh = {"vertices": torch.from_numpy(np.asarray(verts, np.float64)).cuda(), "faces": torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda(),
            "vertex_colors": torch.from_numpy(np.ascontiguousarray(colors[:, :3], dtype=np.uint8)).cuda()}
    K = np.ascontiguousarray(seq["K"], np.float64)
    w2c = np.linalg.inv(seq["poses"])
    result = {"voxel_m": voxel, "frames_fused": frames_fused, "vertices": int(len(verts)), "faces": int(len(faces)), "cell": cell, "frame_size": [w, h],
              "sweeps": sweeps, "exposure_factors_cycled": FACTORS}
    for n in (8, 32):
        ids = np.arange(0, 32, 32 // n)
        factors = np.asarray([FACTORS[k % 3] for k in range(n)], np.float64)[:, None, None, :]
        frames = torch.from_numpy(np.clip(np.floor(seq["color"][ids] * factors + 0.5), 0, 255).astype(np.uint8)).cuda()
        poses = np.ascontiguousarray(w2c[ids])
        call = lambda **kw: _wall(lambda: texturing.texture_mesh(mesh, frames, K, poses, cell=cell, **kw))[1]
        result[f"{n}_key_frames"] = {"texture_mesh_plain_ms": call(), "texture_mesh_exposure_ms": call(exposure=True),
                                     "texture_mesh_levelling_ms": call(levelling=True, levelling_sweeps=sweeps),
                                     "texture_mesh_both_ms": call(exposure=True, levelling=True, levelling_sweeps=sweeps),
                                     **stages(mesh, frames, K, poses, cell, sweeps)}
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the synthetic room fused into the background volume")
    ap.add_argument("--voxel", type=float, default=0.02, help="0.02 -> 256^3 over the 5.12 m volume: about 730 k faces")
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=64, help="Jacobi sweeps of the levelling (texture_mesh's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_levelling_probe.json"))
    args = ap.parse_args()
    result = {"what": "medians of 9 after 2 warm-up runs; stages between HIP events, texture_mesh and the host solve as wall time (texture_mesh ends in a synchronise)",
              "room_640x480": room(args.frames, args.voxel, args.cell, args.sweeps),
              "not_measured": ["a real capture", "a viewer that filters bilinearly", "more than 32 views"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
