"""What the sparse merge (hive_amd.distributed.fuse_sharded(merge="sparse")) saves and costs on ONE GPU, with a single-rank RCCL group.

Two 512^3 volumes over the synthetic room: `static`, the benchmark's sequence fused as it is, and `foreground`, the same frames with the depth kept only under
the drifting ellipse masks (what the dynamic path's foreground volume sees).  For each it records the share of active segments at L = 64, 256 and 1024, the
time of every LOCAL pass of both merge modes (HIP events; the segment list by a host clock, because its count read-back is a synchronisation) and of the whole
`fuse_sharded` call, and `merge_plan`'s bytes per GPU for 2, 4 and 8 ranks.  The two modes are timed in alternation, repetition by repetition.  The dense
passes are the code the default merge has always run, so they are the yardstick.  No link is involved: at world size 1 a collective is a local copy, and
link time is not measured here or anywhere else.

    python tools/probe_sparse_merge.py --out profiles/sparse_merge_probe.json
"""
import argparse
import json
import os
import signal
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sparse_merge_probe.json")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--voxel", type=float, default=0.01, help="0.01 -> 512^3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the process is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)

    import numpy as np
    import torch
    import torch.distributed as dist
    from hive_amd import _lib, distributed as hdist, fusion, synthetic
    assert torch.cuda.is_available(), "probe_sparse_merge.py needs an MI355X"
    torch.cuda.set_device(0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    ctx = _lib.default_context(0)

    T, H, W = args.frames, 480, 640
    seq = synthetic.make_sequence(T, H, W, seed=1234, yaw_step_deg=360.0 / T)
    masks = synthetic.ellipse_masks(T, H, W, num_objects=3, seed=1234)
    color, depth = torch.from_numpy(seq["color"]).cuda(), torch.from_numpy(seq["depth"]).cuda()
    depths = {"static": depth, "foreground": depth * (torch.from_numpy(masks).cuda() != 0)}

    def median_ms(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    result = {"device": torch.cuda.get_device_name(0), "frames": T, "image": [H, W], "voxel_m": args.voxel, "reps": args.reps, "volumes": {},
              "note": "single GPU, world size 1: the collectives are local copies and no link time is measured; modes timed in alternation"}
    for name, d in depths.items():
        vol = fusion.TSDFVolume(synthetic.room_bounds(), args.voxel, ctx=ctx)
        for lo in range(0, T, 20):
            vol.integrate_batch(color[lo:lo + 20], d[lo:lo + 20], seq["K"], seq["poses"][lo:lo + 20])
        n = vol.num_voxels
        weight = vol.device_tensors()[1]
        observed = int((weight > 0).sum().item())
        entry = {"dims": [int(v) for v in vol.vol_dim], "voxels": n, "voxels_observed": observed, "observed_fraction": round(observed / n, 5), "active_fraction": {},
                 "local_passes": {}, "plan_bytes_per_gpu": {}}
        del weight
        active = {}
        for segment in (64, 256, 1024):
            flags = vol.mark_segments(segment)
            active[segment] = int(flags.sum().item())
            entry["active_fraction"][str(segment)] = {"segments": flags.numel(), "active": active[segment], "fraction": round(active[segment] / flags.numel(), 5)}
            entry["plan_bytes_per_gpu"][str(segment)] = {
                str(w): {k: v for k, v in hdist.merge_plan(n, min(n, active[segment] * segment), w, segment=segment).items() if k.startswith(("bytes", "ms", "mode"))}
                for w in (2, 4, 8)}
        for segment in (64, 256, 1024):
            part = hdist.VoxelPartition(n)
            dense_pieces = torch.empty((1, 5, part.chunk), dtype=torch.float32, device="cuda")
            dense_share = torch.zeros((3, part.chunk), dtype=torch.float32, device="cuda")
            a = active[segment]
            sparse_pieces = torch.empty((1, 5, a * segment), dtype=torch.float32, device="cuda")
            sparse_share = torch.zeros((3, a * segment), dtype=torch.float32, device="cuda")
            state = {}

            def sparse_list():
                state["list"], state["a"] = fusion.segment_list(state["flags"], ctx=ctx)

            passes = {
                "dense": [("accum_from_volume_sharded", lambda: vol.accum_from_volume_sharded(dense_pieces, 1, part.chunk)),
                          ("fold", lambda: vol.accum_finalize_range(dense_pieces[0], part.chunk, n, [dense_share[0], dense_share[1], dense_share[2]])),
                          ("set_volume_range", lambda: vol.set_volume_range(0, n, tsdf=dense_share[0], weight=dense_share[1], color=dense_share[2]))],
                "sparse": [("mark", lambda: state.__setitem__("flags", vol.mark_segments(segment))),
                           ("list", sparse_list),
                           ("pack", lambda: vol.accum_from_volume_segments(sparse_pieces, state["list"], a, segment, 1, a)),
                           ("fold", lambda: vol.accum_finalize_range(sparse_pieces[0], a * segment, a * segment, [sparse_share[0], sparse_share[1], sparse_share[2]])),
                           ("scatter", lambda: vol.set_volume_segments(sparse_share.view(1, 3, -1), state["list"], a, segment, 1, a))],
            }
            samples = {mode: {p: [] for p, _ in steps} for mode, steps in passes.items()}
            whole = {"dense": [], "sparse": []}
            for rep in range(args.reps + 1):  # (the first repetition warms up and is dropped)
                for mode, steps in passes.items():
                    for p, fn in steps:
                        ms = host_ms(fn)[0] if p == "list" else event_ms(fn)
                        if rep:
                            samples[mode][p].append(ms)
                    assert mode == "dense" or state["a"] == a
                for mode in ("dense", "sparse"):
                    ms = host_ms(lambda: hdist.fuse_sharded(vol, merge=mode, segment=segment))[0]
                    if rep:
                        whole[mode].append(ms)
            entry["local_passes"][str(segment)] = {
                mode: dict({p: median_ms(v) for p, v in samples[mode].items()}, sum_of_medians_ms=round(sum(statistics.median(v) for v in samples[mode].values()), 4),
                           fuse_sharded_world1_host_ms=median_ms(whole[mode])) for mode in passes}
            del dense_pieces, dense_share, sparse_pieces, sparse_share
        assert int((vol.device_tensors()[1] > 0).sum().item()) == observed  # (the repeated merges of one rank's volume keep its weights)
        result["volumes"][name] = entry
        vol.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"observed": v["observed_fraction"], "active": {s: a["fraction"] for s, a in v["active_fraction"].items()},
                          "L256": {m: p["sum_of_medians_ms"] for m, p in v["local_passes"]["256"].items()}} for k, v in result["volumes"].items()}))
    dist.destroy_process_group()
    signal.alarm(0)


if __name__ == "__main__":
    main()
