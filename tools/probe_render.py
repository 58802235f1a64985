"""Timings of the mesh renderer (hive_amd.render.render_mesh, csrc/render.hip) at 640 x 480 on the MI355X (not gated by any test; DESIGN.md section 3b records the
figures):

  * the background mesh of the synthetic room the benchmark fuses (here --frames frames into a volume of --voxel metres), from a pose of the sequence;
  * one foreground.process_frame mesh (three ellipse objects, textured) from its own pose;
  * per stage of each: hive_render_clear, hive_render_draw (projection + the two raster kernels), hive_render_shade, hive_render_resolve, between HIP events;
  * the median absolute difference between the rendered depth of the fused room and synthetic.raycast_room_depth from the same pose -- the first check of
    the whole chain depth -> fusion -> marching cubes -> picture against the input.

Warm-up, then several repeats; every timed window ends in a device synchronise.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(samples):
    return round(1e3 * float(np.median(samples)), 4)


def _time_render(K, pose, meshes, h, w, repeats):
    """Wall time of whole render_mesh calls on device-resident meshes (scratch reused), and the path counts."""
    import torch
    from hive_amd.render import RenderBuffers, render_mesh
    buffers = RenderBuffers(h, w)
    samples = []
    for i in range(repeats + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render_mesh(K, pose, *meshes, size=(h, w), return_depth=True, return_faces=True, buffers=buffers)
        torch.cuda.synchronize()
        if i >= 5:
            samples.append(time.perf_counter() - t0)
    small, large = buffers.path_counts()
    return out, {"render_mesh_ms": _median_ms(samples), "faces_one_thread_each": small, "faces_one_workgroup_each": large}


def _time_stages(K, pose, meshes, h, w, repeats):
    """The four entry points one by one between HIP events (what render_mesh issues, for device-resident meshes)."""
    import torch
    from hive_amd import _lib
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers, _camera, _mesh_arrays
    ctx = _lib.default_context(0)
    lib, handle = ctx.lib, ctx.handle
    Kd, R, t, h, w = _camera(K, pose, (h, w))
    dev = torch.device("cuda", 0)
    buffers = RenderBuffers(h, w)
    arrays, base = [], 0
    for k, m in enumerate(meshes):
        a = _mesh_arrays(m, dev)
        arrays.append((a, base, buffers.slot(k, a[0].shape[0], a[1].shape[0])))
        base += int(a[1].shape[0])
    color = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    bg = np.full(3, 255, np.uint8)

    def clear():
        ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))

    def draw():
        for (v, f, c, uv, tex), face_base, (xy, z, large, counts) in arrays:
            ctx.check(lib.hive_render_draw(handle, ptr(v), v.shape[0], ptr(f), f.shape[0], face_base, ptr(Kd), ptr(R), ptr(t), h, w, 0.05, ptr(xy), ptr(z), ptr(large),
                                           ptr(counts), ptr(buffers.key)))

    def shade():
        for (v, f, c, uv, tex), face_base, (xy, z, large, counts) in arrays:
            ht, wt = (0, 0) if tex is None else (int(tex.shape[0]), int(tex.shape[1]))
            ctx.check(lib.hive_render_shade(handle, v.shape[0], ptr(f), f.shape[0], face_base, ptr(xy), ptr(z), ptr(c), ptr(uv), ptr(tex), ht, wt, ptr(buffers.key), h, w,
                                            ptr(color)))

    def resolve():
        ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, ptr(bg), ptr(color), ptr(depth), None))

    stages = (("clear", clear), ("draw", draw), ("shade", shade), ("resolve", resolve))
    times = {name: [] for name, _ in stages}
    for i in range(repeats + 3):
        for name, fn in stages:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if i >= 3:
                times[name].append(start.elapsed_time(stop) * 1e-3)
    return {name + "_ms": _median_ms(v) for name, v in times.items()}


def room(frames, voxel, repeats):
    import torch
    from hive_amd import _lib, fusion, synthetic
    h, w = 480, 640
    seq = synthetic.make_sequence(num_frames=frames, height=h, width=w, yaw_step_deg=360.0 / frames)
    ctx = _lib.default_context(0)
    vol = fusion.TSDFVolume(synthetic.room_bounds(), voxel, ctx=ctx)
    for i in range(frames):
        vol.integrate(seq["color"][i], seq["depth"][i], seq["K"], seq["poses"][i])
    verts, faces, _, colors = vol.get_mesh()
    mesh = {"vertices": torch.from_numpy(np.asarray(verts, np.float64)).cuda(), "faces": torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda(),
            "vertex_colors": torch.from_numpy(np.ascontiguousarray(colors[:, :3], dtype=np.uint8)).cuda()}
    K = np.asarray(seq["K"], np.float64)
    c2w = seq["poses"][frames // 3]
    pose = np.linalg.inv(c2w)
    (color, depth, face), out = _time_render(K, pose, [mesh], h, w, repeats)
    out = {"voxel_m": voxel, "frames_fused": frames, "vertices": int(len(verts)), "faces": int(len(faces)), **out, **_time_stages(K, pose, [mesh], h, w, repeats)}
    want = synthetic.raycast_room_depth(c2w, K, h, w)[0]
    got = depth.cpu().numpy()
    hit = got > 0
    out["pixels_hit_share"] = round(float(hit.mean()), 4)
    out["depth_vs_raycast_median_abs_m"] = float(np.median(np.abs(got[hit].astype(np.float64) - want[hit])))
    out["depth_vs_raycast_p99_abs_m"] = float(np.percentile(np.abs(got[hit].astype(np.float64) - want[hit]), 99))
    from hive_amd.render import psnr
    out["psnr_vs_frame_db"] = round(psnr(color, seq["color"][frames // 3], mask=hit), 2)
    return out


def frame_mesh(repeats):
    import torch
    from hive_amd import _lib, foreground, synthetic
    from hive_amd.options import MaskDilationOptions
    from hive_amd.render import psnr
    h, w = 480, 640
    seq = synthetic.make_sequence(num_frames=1, height=h, width=w, yaw_step_deg=2.4)
    ids = synthetic.ellipse_masks(1, h, w, num_objects=3, seed=3)[0].copy()
    ids[seq["depth"][0] == 0] = 0
    pose = np.linalg.inv(seq["poses"][0])
    mesh = foreground.process_frame(torch.from_numpy(seq["color"][0]).cuda(), torch.from_numpy(seq["depth"][0]).cuda(), torch.from_numpy(ids).cuda(), seq["K"], pose,
                                    MaskDilationOptions(num_iterations=0), ctx=_lib.default_context(0))
    mesh = dict(mesh, faces=mesh["faces"].to(torch.int32))
    K = np.asarray(seq["K"], np.float64)
    (color, depth, face), out = _time_render(K, pose, [mesh], h, w, repeats)
    hit = (face >= 0).cpu().numpy()
    return {"vertices": int(mesh["vertices"].shape[0]), "faces": int(mesh["faces"].shape[0]), **out, **_time_stages(K, pose, [mesh], h, w, repeats),
            "pixels_hit_share": round(float(hit.mean()), 4), "psnr_vs_frame_db": psnr(color, seq["color"][0], mask=hit)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the synthetic room fused into the background volume (a full turn)")
    ap.add_argument("--voxel", type=float, default=0.02, help="0.02 -> 256^3 over the 5.12 m volume (the benchmark's 0.01 gives four times the faces)")
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    print(json.dumps({"room_640x480": room(args.frames, args.voxel, args.repeats), "process_frame_640x480": frame_mesh(args.repeats)}, indent=1))
