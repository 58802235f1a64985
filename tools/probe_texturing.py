"""Timings of background texturing (hive_amd.texturing.texture_mesh, csrc/texture.hip) on the MI355X (not gated by any test; DESIGN.md section 5.22 and the README
record the figures; writes profiles/texturing_probe.json):

  * the mesh of the synthetic room the benchmark fuses (--frames frames into a volume of --voxel metres: about 730 k faces) textured from 8 and from 32 key frames
    at 640 x 480 with cell 8, everything device-resident;
  * per stage between HIP events: the votes of all views (clear + draw + resolve + select per view) and hive_texture_select alone, hive_texture_unweld,
    hive_texture_fill; and the wall time of the whole texture_mesh call;
  * beside them the numpy restatement (tests/texturing_restatement.py) on one small case (513 faces, 3 views, 64 x 48) on the same machine, with the kernels' time
    on that case -- a statement about the restatement's cost, not a speed-up of anything a user runs.

Medians of 9 after 2 warm-up runs; every timed window ends in a device synchronise.  Not measured here: a real capture, a player opening the file, seams."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS = 2, 9


def _median_ms(samples):
    return round(1e3 * float(np.median(samples)), 4)


def _events(fn):
    import torch
    samples = []
    for i in range(WARMUP + REPEATS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        if i >= WARMUP:
            samples.append(start.elapsed_time(stop) * 1e-3)
    return _median_ms(samples)


def _wall(fn):
    import torch
    samples = []
    for i in range(WARMUP + REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= WARMUP:
            samples.append(time.perf_counter() - t0)
    return out, _median_ms(samples)


def stages(mesh, frames, K, poses, cell):
    """What texture_mesh issues, stage by stage, on device-resident inputs."""
    import torch
    from hive_amd import _lib, texturing
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers
    ctx = _lib.default_context(0)
    lib, handle = ctx.lib, ctx.handle
    v, f, c = mesh["vertices"], mesh["faces"], mesh["vertex_colors"]
    nv, nf = v.shape[0], f.shape[0]
    n, h, w = frames.shape[:3]
    wt, ht, _ = texturing.atlas_layout(nf, cell)
    buffers = RenderBuffers(h, w)
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    best = torch.zeros(nf, dtype=torch.int64, device="cuda")
    d_poses = torch.from_numpy(np.ascontiguousarray(np.concatenate([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3]], axis=1))).cuda()
    out_v, out_f = torch.empty((3 * nf, 3), dtype=torch.float64, device="cuda"), torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    uv, views = torch.empty((3 * nf, 2), dtype=torch.float64, device="cuda"), torch.empty(nf, dtype=torch.int32, device="cuda")
    atlas = torch.empty((ht, wt, 3), dtype=torch.uint8, device="cuda")

    def select(k):
        ctx.check(lib.hive_texture_select(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), None, h, w, k, 0.05, ptr(best)))

    def votes():
        best.zero_()
        for k in range(n):
            R, t = np.ascontiguousarray(poses[k, :3, :3]), np.ascontiguousarray(poses[k, :3, 3])
            ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
            ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), h, w, 0.05, ptr(xy), ptr(z), ptr(large), ptr(counts), ptr(buffers.key)))
            ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, None, None, ptr(depth), None))
            select(k)

    out = {"votes_all_views_ms": _events(votes), "select_one_view_ms": _events(lambda: select(n - 1))}
    votes()
    out["unweld_ms"] = _events(lambda: ctx.check(lib.hive_texture_unweld(handle, ptr(v), nv, ptr(f), nf, cell, ptr(best), ptr(out_v), ptr(out_f), ptr(uv), ptr(views))))
    out["fill_ms"] = _events(lambda: ctx.check(lib.hive_texture_fill(handle, ptr(v), nv, ptr(c), ptr(f), nf, ptr(best), ptr(frames), n, h, w, ptr(K), ptr(d_poses), 0.05,
                                                                      cell, ptr(atlas))))
    out["atlas"] = [wt, ht]
    out["faces_with_a_view_share"] = round(float((views >= 0).float().mean()), 4)
    return out


def room(frames_fused, voxel, cell):
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
    K = np.asarray(seq["K"], np.float64)
    w2c = np.linalg.inv(seq["poses"])
    result = {"voxel_m": voxel, "frames_fused": frames_fused, "vertices": int(len(verts)), "faces": int(len(faces)), "cell": cell, "frame_size": [w, h]}
    for n in (8, 32):
        ids = np.arange(0, 32, 32 // n)
        frames, poses = torch.from_numpy(seq["color"][ids]).cuda(), np.ascontiguousarray(w2c[ids])
        _, whole = _wall(lambda: texturing.texture_mesh(mesh, frames, K, poses, cell=cell))
        result[f"{n}_key_frames"] = {"texture_mesh_ms": whole, **stages(mesh, frames, K, poses, cell)}
    return result


def restatement():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import texturing_cases as C
    import texturing_restatement as TR
    from hive_amd import texturing
    case = C.soup_case(513, 9, 3, False)
    samples = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = TR.texture_mesh(case["mesh"], case["frames"], C.K, case["poses"], cell=9)
        samples.append(time.perf_counter() - t0)
    got, kernels = _wall(lambda: texturing.texture_mesh(case["mesh"], case["frames"], C.K, case["poses"], cell=9))
    assert np.array_equal(got["texture"].cpu().numpy(), want["texture"])
    return {"faces": 513, "views": 3, "frame_size": [C.W, C.H], "cell": 9, "numpy_restatement_ms": _median_ms(samples), "texture_mesh_host_inputs_ms": kernels}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the synthetic room fused into the background volume")
    ap.add_argument("--voxel", type=float, default=0.02, help="0.02 -> 256^3 over the 5.12 m volume: about 730 k faces")
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texturing_probe.json"))
    args = ap.parse_args()
    result = {"what": "medians of 9 after 2 warm-up runs; stages between HIP events, texture_mesh as wall time ending in a synchronise",
              "room_640x480": room(args.frames, args.voxel, args.cell), "small_case_against_the_numpy_restatement": restatement(),
              "not_measured": ["a real capture", "a player opening the file", "seams"]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
