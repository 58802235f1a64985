"""Timings of the label smoothing of background texturing (hive_amd.texturing.texture_mesh with ``smoothness``, csrc/texture_smooth.hip) on the MI355X (not gated
by any test; DESIGN.md and the README record the figures; writes profiles/texture_smoothing_probe.json):

  * the mesh of the synthetic room the benchmark fuses (--frames frames into a volume of --voxel metres: about 730 k faces) textured from 8 and from 32 key frames
    at 640 x 480 with cell 8, everything device-resident, at --smoothness px^2;
  * per stage between HIP events: the table of all views (clear + draw + resolve + vote per view) and hive_texture_vote alone, hive_mesh_face_neighbours (with
    its read-back), hive_texture_smooth (with its read-backs);
  * the wall time of the whole texture_mesh call with smoothing beside the same call without it in the same session -- the reference of this probe -- and with
    the back-face test alone;
  * rounds, label changes, seam entries before and after, the area given up; the size of the table of areas (8 n F bytes).

Medians of 9 after 2 warm-up runs; every timed window ends in a device synchronise.  Not measured here: a real capture, visible seams, a viewer."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from probe_texturing import _events, _wall  # noqa: E402


def stages(mesh, frames, K, poses, seam_cost):
    """What texture_mesh issues on its smoothing path before unweld and fill, stage by stage, on device-resident inputs."""
    import torch
    from hive_amd import _lib, texturing
    from hive_amd._lib import ptr
    from hive_amd.render import RenderBuffers
    ctx = _lib.default_context(0)
    lib, handle = ctx.lib, ctx.handle
    v, f = mesh["vertices"], mesh["faces"]
    nv, nf = v.shape[0], f.shape[0]
    n, h, w = frames.shape[:3]
    buffers = RenderBuffers(h, w)
    xy, z, large, counts = buffers.slot(0, nv, nf)
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    area = torch.empty((n, nf), dtype=torch.int64, device="cuda")

    def vote(k):
        ctx.check(lib.hive_texture_vote(handle, ptr(f), nf, nv, ptr(xy), ptr(z), ptr(depth), None, h, w, k, 0.05, 0, ptr(area)))

    def table():
        for k in range(n):
            R, t = np.ascontiguousarray(poses[k, :3, :3]), np.ascontiguousarray(poses[k, :3, 3])
            ctx.check(lib.hive_render_clear(handle, ptr(buffers.key), h, w))
            ctx.check(lib.hive_render_draw(handle, ptr(v), nv, ptr(f), nf, 0, ptr(K), ptr(R), ptr(t), h, w, 0.05, ptr(xy), ptr(z), ptr(large), ptr(counts), ptr(buffers.key)))
            ctx.check(lib.hive_render_resolve(handle, ptr(buffers.key), h, w, None, None, ptr(depth), None))
            vote(k)

    out = {"table_all_views_ms": _events(table), "vote_one_view_ms": _events(lambda: vote(n - 1)), "table_bytes": int(area.numel() * 8)}
    table()
    out["face_neighbours_ms"] = _events(lambda: texturing.face_neighbours(f, nv, ctx=ctx))
    offsets, neighbours = texturing.face_neighbours(f, nv, ctx=ctx)
    out["neighbour_entries"] = int(neighbours.shape[0])
    out["smooth_ms"] = _events(lambda: texturing.smooth_labels(area, offsets, neighbours, seam_cost, ctx=ctx))
    return out


def room(frames_fused, voxel, cell, smoothness):
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
    seam_cost = int(np.floor(smoothness * texturing.AREA_UNITS_PER_PX2 + 0.5))
    result = {"voxel_m": voxel, "frames_fused": frames_fused, "vertices": int(len(verts)), "faces": int(len(faces)), "cell": cell, "frame_size": [w, h],
              "smoothness_px2": smoothness}
    for n in (8, 32):
        ids = np.arange(0, 32, 32 // n)
        frames, poses = torch.from_numpy(seq["color"][ids]).cuda(), np.ascontiguousarray(w2c[ids])
        _, plain = _wall(lambda: texturing.texture_mesh(mesh, frames, K, poses, cell=cell))
        smoothed, whole = _wall(lambda: texturing.texture_mesh(mesh, frames, K, poses, cell=cell, smoothness=smoothness, return_stats=True))
        culled, cull = _wall(lambda: texturing.texture_mesh(mesh, frames, K, poses, cell=cell, cull_back_faces=True, return_views=True))
        result[f"{n}_key_frames"] = {"texture_mesh_without_smoothing_ms": plain, "texture_mesh_smoothed_ms": whole, "texture_mesh_back_faces_culled_ms": cull,
                                     "faces_with_a_front_view_share": round(float((culled["views"] >= 0).float().mean()), 4),
                                     **stages(mesh, frames, K, poses, seam_cost), "smoothing": smoothed["stats"]}
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the synthetic room fused into the background volume")
    ap.add_argument("--voxel", type=float, default=0.02, help="0.02 -> 256^3 over the 5.12 m volume: about 730 k faces")
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--smoothness", type=float, default=4.0, help="px^2 a face may give up to remove one seam edge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_smoothing_probe.json"))
    args = ap.parse_args()
    result = {"what": "medians of 9 after 2 warm-up runs; stages between HIP events, texture_mesh as wall time ending in a synchronise",
              "room_640x480": room(args.frames, args.voxel, args.cell, args.smoothness), "not_measured": ["a real capture", "visible seams", "a viewer"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
