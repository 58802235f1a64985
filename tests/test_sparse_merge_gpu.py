"""The sparse merge (``fuse_sharded(merge="sparse")``): its four kernels against their torch restatements in ``hive_amd.distributed`` (exact), the whole
merge against the dense one on a single-rank RCCL group (bit for bit), and on two gloo ranks sharing the one GPU (bit for bit between the modes and
between the ranks).  Volumes have voxel size 1 and bounds [0, X] x [0, Y] x [0, Z]; their planes are set from seeded arrays, so the tests control which
segments are active: weights are small integers, tsdf is uniform in [-1, 1] where the weight is non-zero and 1 elsewhere, colours are packed bytes where the
weight is non-zero and 0 elsewhere (the contract on unobserved voxels)."""
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# N = 1: one segment of one voxel; 512: exactly 2 (L = 256) / 8 (L = 64) segments; 385: the last segment holds 129 / 1 voxels; 10080: 40 segments, the last
# holds 96, and 40 is no multiple of 3 (L = 256); 158 segments, the last holds 32 (L = 64)
DIMS = [(1, 1, 1), (8, 8, 8), (5, 7, 11), (24, 20, 21)]
SEGMENTS = [64, 256]


def _volume(dims, ctx, storage=None):
    from hive_amd import fusion
    return fusion.TSDFVolume(np.array([[0.0, dims[0]], [0.0, dims[1]], [0.0, dims[2]]]), 1.0, ctx=ctx, storage=storage)


def _planes(n, segment, active, seed):
    """(tsdf, weight, colour) float32 [n] whose non-zero weights lie in the segments of ``active`` (bool [S]); every such segment gets at least one."""
    rng = np.random.default_rng(seed)
    weight = np.zeros(n, np.float32)
    for s in np.flatnonzero(active):
        lo, hi = s * segment, min((s + 1) * segment, n)
        w = rng.integers(1, 6, hi - lo) * (rng.random(hi - lo) < 0.5)
        w[rng.integers(0, hi - lo)] = rng.integers(1, 6)
        weight[lo:hi] = w
    seen = weight != 0
    tsdf = np.where(seen, rng.uniform(-1.0, 1.0, n), 1.0).astype(np.float32)
    color = np.where(seen, rng.integers(0, 1 << 24, n), 0).astype(np.float32)
    return tsdf, weight, color


def _set_planes(vol, planes):
    import torch
    t, w, c = (torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)
    torch.cuda.synchronize()
    vol.set_volume_range(0, vol.num_voxels, tsdf=t, weight=w, color=c)
    vol._ctx.synchronize()


def _bits(t):
    """A float32 tensor's words, on the host: comparisons of these are bit for bit (-0.0 != +0.0, a NaN equals itself)."""
    import torch
    return t.detach().contiguous().cpu().view(torch.int32)


def _sums(planes):
    """[5, n] float32: the five sums the merge adds, in torch on the host (one float32 multiply each, as in the kernel)."""
    import torch
    t, w, c = (torch.from_numpy(p) for p in planes)
    ci = c.to(torch.int64)
    return torch.stack([t * w, w, (ci & 255).float() * w, ((ci >> 8) & 255).float() * w, (ci >> 16).float() * w])


def _weight_patterns(n, segment):
    n_segments = -(-n // segment)
    rng = np.random.default_rng(n + segment)

    def single(at, value=3.0):
        w = np.zeros(n, np.float32)
        w[at] = value
        return w
    every = np.zeros(n, np.float32)
    third = np.zeros(n, np.float32)
    for s in range(n_segments):
        lo, hi = s * segment, min((s + 1) * segment, n)
        every[rng.integers(lo, hi)] = 1.0
        if s % 3 == 0:
            third[rng.integers(lo, hi)] = 2.0
    return {
        "all zero": np.zeros(n, np.float32),
        "first word of a segment": single((n_segments // 2) * segment),
        "last word of a segment": single(min(segment, n) - 1),
        "last valid voxel of the last segment": single(n - 1),
        "a single -0.0f": single(n // 2, -0.0),
        "every segment": every,
        "every third segment": third,
    }


@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("dims", DIMS)
def test_flags_and_list_are_exact(gpu_ctx, dims, segment):
    import torch
    from hive_amd import distributed as hdist, fusion
    n = dims[0] * dims[1] * dims[2]
    n_segments = -(-n // segment)
    vol = _volume(dims, gpu_ctx)
    for name, weight in _weight_patterns(n, segment).items():
        words = np.zeros(n_segments * segment, np.uint32)
        words[:n] = weight.view(np.uint32)
        want = (words.reshape(n_segments, segment) != 0).any(axis=1)
        assert np.array_equal(hdist.segment_flags(torch.from_numpy(weight), segment).numpy(), want.astype(np.uint8)), name
        w_dev = torch.from_numpy(weight).cuda()
        vol.set_volume_range(0, n, weight=w_dev)
        flags = vol.mark_segments(segment)
        assert flags.dtype == torch.uint8 and np.array_equal(flags.cpu().numpy(), want.astype(np.uint8)), name
        assert torch.equal(fusion.mark_segments(w_dev, segment, ctx=gpu_ctx), flags), name
        seg_list, n_active = fusion.segment_list(flags, ctx=gpu_ctx)
        assert seg_list.dtype == torch.int32 and seg_list.numel() == n_segments
        assert n_active == int(want.sum()) and np.array_equal(seg_list[:n_active].cpu().numpy(), np.flatnonzero(want)), name
    assert _weight_patterns(n, segment)["a single -0.0f"].view(np.uint32).max() == 0x80000000  # (the -0.0f really is one)


@pytest.mark.parametrize("n_segments", [1023, 1025, 5000, 1024 * 1024 + 1500])
def test_segment_list_over_many_blocks(gpu_ctx, n_segments):
    """One workgroup lists 1024 flags, one scan thread takes ceil(blocks / 1024) blocks: both sides of each, and the 4.2 M segments of 1024^3 in spirit."""
    import torch
    from hive_amd import fusion
    flags = np.random.default_rng(n_segments).random(n_segments) < 0.37
    flags[[0, -1]] = True
    seg_list, n_active = fusion.segment_list(torch.from_numpy(flags.astype(np.uint8) * 255).cuda(), ctx=gpu_ctx)  # (any non-zero byte is a flag)
    assert n_active == int(flags.sum()) and np.array_equal(seg_list[:n_active].cpu().numpy(), np.flatnonzero(flags))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("segment", SEGMENTS)
@pytest.mark.parametrize("dims", DIMS)
def test_pack_and_scatter_match_the_torch_forms(gpu_ctx, dims, segment, world):
    import torch
    from hive_amd import distributed as hdist, fusion
    n = dims[0] * dims[1] * dims[2]
    n_segments = -(-n // segment)
    active = np.arange(n_segments) % 3 == 0
    active[-1] = True  # the ragged last segment takes part
    planes = _planes(n, segment, active, seed=n + segment)
    vol = _volume(dims, gpu_ctx)
    _set_planes(vol, planes)
    seg_list, n_active = fusion.segment_list(vol.mark_segments(segment), ctx=gpu_ctx)
    assert n_active == int(active.sum())
    per = -(-n_active // world)
    sums = _sums(planes)
    want = hdist.pack_segments(sums, seg_list[:n_active].cpu(), segment, world)
    assert tuple(want.shape) == (world, 5, per * segment)
    # the zero padding: past the list, and the lanes past N of the last segment
    assert not want[-1, :, max(0, n_active - (world - 1) * per) * segment:].any()
    got = torch.full((world, 5, per * segment), float("nan"), dtype=torch.float32, device="cuda")
    vol.accum_from_volume_segments(got, seg_list, n_active, segment, world, per)
    assert torch.equal(_bits(got), _bits(want)), "volume form"
    got.fill_(float("nan"))
    fusion.accum_pack_segments(sums.cuda(), got, seg_list, n_active, segment, world, per, ctx=gpu_ctx)
    assert torch.equal(_bits(got), _bits(want)), "accumulator form"
    # the way back: all-gather-shaped data into a volume in caller-owned storage with a guard behind every plane
    rng = np.random.default_rng(7 * n + world)
    gathered = torch.from_numpy(rng.uniform(-4.0, 4.0, (world, 3, per * segment)).astype(np.float32))
    guard = 4096
    store = [torch.full((n + guard,), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    dst = _volume(dims, gpu_ctx, storage=tuple(s[:n] for s in store))
    before = [torch.from_numpy(rng.uniform(10.0, 20.0, n).astype(np.float32)) for _ in range(3)]
    dst.set_volume_range(0, n, tsdf=before[0].cuda(), weight=before[1].cuda(), color=before[2].cuda())
    dst.set_volume_segments(gathered.cuda(), seg_list, n_active, segment, world, per)
    gpu_ctx.synchronize()
    expect = hdist.unpack_segments(gathered, seg_list[:n_active].cpu(), segment, torch.stack(before).clone())
    outside = torch.from_numpy(~np.repeat(active, segment)[:n])
    for k in range(3):
        assert torch.equal(_bits(store[k][:n]), _bits(expect[k])), k
        assert torch.equal(store[k][:n].cpu()[outside], before[k][outside]), "voxels of inactive segments are untouched"
        assert bool((store[k][n:] == -7.0).all()), "nothing is written beyond N"


# ---- the whole merge on a single-rank RCCL group: the very collectives of the 8-GPU job ---------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_group():
    import torch
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    yield dist
    dist.destroy_process_group()


@pytest.fixture()
def collective_calls(monkeypatch):
    import torch.distributed as tdist
    calls = {"reduce_scatter_tensor": 0, "all_gather_into_tensor": 0, "all_reduce": 0}
    for name in calls:
        def wrapped(*a, _orig=getattr(tdist, name), _name=name, **k):
            assert a[0].is_cuda and a[0].numel() > 0, "collectives run on non-empty device buffers"
            calls[_name] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(tdist, name, wrapped)
    return calls


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("dims", [(24, 20, 21), (5, 7, 11)])
def test_rccl_sparse_merge_equals_dense_bit_for_bit(gpu_ctx, nccl_group, collective_calls, dims, side_stream):
    import torch
    from hive_amd import depth as depth_mod, distributed as hdist
    segment = 256
    n = dims[0] * dims[1] * dims[2]
    n_segments = -(-n // segment)
    active = np.arange(n_segments) % 2 == 1  # (5 x 7 x 11: the ragged last segment alone)
    planes = _planes(n, segment, active, seed=n)
    ctx = depth_mod.DepthFusionStream.side_stream_context(0) if side_stream else gpu_ctx
    merged = {}
    for mode in ("dense", "sparse"):
        vol = _volume(dims, ctx)
        _set_planes(vol, planes)
        assert hdist.fuse_sharded(vol, merge=mode, segment=segment) is vol
        merged[mode] = vol.device_tensors()
        torch.cuda.synchronize()
        assert vol.merge_stats["mode"] == mode
    assert collective_calls == {"reduce_scatter_tensor": 2, "all_gather_into_tensor": 2, "all_reduce": 1}  # the flags' all-reduce is the sparse mode's
    for k, name in enumerate(("tsdf", "weight", "colour")):
        assert torch.equal(_bits(merged["sparse"][k]), _bits(merged["dense"][k])), name
    assert torch.equal(merged["dense"][1].cpu(), torch.from_numpy(planes[1]))  # (one rank: the merge gives the weights back)
    per_l = int(active.sum()) * segment
    assert vol.merge_stats == {"mode": "sparse", "segment": segment, "segments": n_segments, "active": int(active.sum()), "bytes_flags": n_segments,
                               "bytes_reduce_scatter": 4 * 5 * per_l, "bytes_all_gather": 4 * 3 * per_l}


def test_rccl_sparse_merge_of_accumulators_equals_dense(gpu_ctx, nccl_group):
    """`fuse_sharded(volume, accum, merge="sparse")`: raw accumulator planes go through the plain gather; the volume holds its initial values elsewhere."""
    import torch
    from hive_amd import distributed as hdist
    dims, segment = (24, 20, 21), 64
    n = dims[0] * dims[1] * dims[2]
    active = np.arange(-(-n // segment)) % 5 < 2
    accum = _sums(_planes(n, segment, active, seed=3)).cuda().reshape(-1)
    merged = {}
    for mode in ("dense", "sparse"):
        vol = _volume(dims, gpu_ctx)
        hdist.fuse_sharded(vol, accum, merge=mode, segment=segment)
        merged[mode] = vol.device_tensors()
    assert vol.merge_stats["active"] == int(active.sum()) < vol.merge_stats["segments"]
    for a, b in zip(merged["sparse"], merged["dense"]):
        assert torch.equal(_bits(a), _bits(b))


def test_rccl_sparse_merge_of_an_unobserved_volume(gpu_ctx, nccl_group, collective_calls):
    """A == 0: the volume stays as it is, and nothing of size zero is launched or sent (the flags' all-reduce is the only collective)."""
    import torch
    from hive_amd import distributed as hdist
    vol = _volume((5, 7, 11), gpu_ctx)
    before = [t.clone() for t in vol.device_tensors()]
    hdist.fuse_sharded(vol, merge="sparse", segment=64)
    assert collective_calls == {"reduce_scatter_tensor": 0, "all_gather_into_tensor": 0, "all_reduce": 1}
    assert vol.merge_stats == {"mode": "sparse", "segment": 64, "segments": 7, "active": 0, "bytes_flags": 7, "bytes_reduce_scatter": 0, "bytes_all_gather": 0}
    for a, b in zip(vol.device_tensors(), before):
        assert torch.equal(_bits(a), _bits(b))
    # the entry points themselves take A == 0 (no buffer, no launch)
    empty, no_list = torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    vol.accum_from_volume_segments(empty, no_list, 0, 64, 1, 0)
    vol.set_volume_segments(empty, no_list, 0, 64, 1, 0)
    gpu_ctx.synchronize()


def test_rccl_auto_takes_the_mode_the_plan_names(gpu_ctx, nccl_group, monkeypatch):
    from hive_amd import distributed as hdist
    dims, segment = (24, 20, 21), 256
    n = dims[0] * dims[1] * dims[2]
    active = np.arange(-(-n // segment)) % 2 == 0
    chosen = []
    for sync_ms in (hdist.SPARSE_SYNC_MS, 0.0):  # (at this size the assumed read-back cost decides: with it dense, without it sparse)
        monkeypatch.setattr(hdist, "SPARSE_SYNC_MS", sync_ms)
        vol = _volume(dims, gpu_ctx)
        _set_planes(vol, _planes(n, segment, active, seed=11))
        hdist.fuse_sharded(vol, merge="auto", segment=segment)
        plan = hdist.merge_plan(n, int(active.sum()) * segment, 1, segment=segment)
        assert vol.merge_stats["mode"] == plan["mode"] and vol.merge_stats["active"] == plan["active"] == int(active.sum())
        chosen.append(plan["mode"])
    assert chosen == ["dense", "sparse"]


def test_bad_merge_arguments_raise_before_any_collective(gpu_ctx, nccl_group, collective_calls):
    from hive_amd import distributed as hdist
    vol = _volume((5, 7, 11), gpu_ctx)
    for kwargs in ({"merge": "sparce"}, {"merge": "sparse", "segment": 100}, {"merge": "sparse", "segment": 32}, {"merge": "dense", "segment": 8192},
                   {"merge": "auto", "segment": 256.0}):
        with pytest.raises(ValueError):
            hdist.fuse_sharded(vol, **kwargs)
    assert not any(collective_calls.values())


# ---- two ranks (gloo) sharing the one GPU: three processes hold it, the parent and the two workers -------------------------------------------------
def _two_rank_worker(rank, world, port, out_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HIVE_DIST_BACKEND="gloo")
    import torch
    from hive_amd import _lib, distributed as hdist
    from hive_amd.options import BackgroundMeshOptions
    from test_distributed_gpu import _ShardedFake
    hdist.init_from_env()
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    out = {}
    dims = (24, 20, 21)
    n = dims[0] * dims[1] * dims[2]
    for segment in (256, 64):
        s = np.arange(-(-n // segment))
        planes = _planes(n, segment, s % (4 if rank == 0 else 3) == 0, seed=100 * rank + segment)
        for mode in ("dense", "sparse"):
            vol = _volume(dims, ctx)
            _set_planes(vol, planes)
            hdist.fuse_sharded(vol, merge=mode, segment=segment)
            t, c, w = vol.get_volume(with_weight=True)
            out[f"{mode}_{segment}"] = np.stack([t, w, c])
        out[f"stats_{segment}"] = np.array([vol.merge_stats["active"], vol.merge_stats["segments"]])
    options = BackgroundMeshOptions(sdf_voxel_size=0.05, sdf_max_voxels=400_000, depth_mask_dilation_iterations=2)
    for mode in ("dense", "sparse"):
        vols = hdist.tsdf_fusion_fg_bg_sharded(_ShardedFake(7), options, merge=mode, segment=256)
        for name, vol in vols.items():
            t, c, w = vol.get_volume(with_weight=True)
            out[f"{name}_{mode}"] = np.stack([t, w, c])
            out[f"{name}_stats_{mode}"] = np.array([vol.merge_stats["active"] or 0, vol.merge_stats["segments"]])
            assert vol.merge_stats["mode"] == mode
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    hdist.barrier()
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def two_rank_results(gpu_ctx, tmp_path_factory):
    """ONE pair of worker processes runs every two-rank case; a rank that dies or stalls ends the wait instead of hanging it."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_dir = str(tmp_path_factory.mktemp("sparse_two_rank"))
    procs = mp.start_processes(_two_rank_worker, args=(2, port, out_dir), nprocs=2, join=False, start_method="spawn")
    deadline = time.monotonic() + 300.0
    while not procs.join(timeout=2.0):  # (raises as soon as one worker failed, after ending the other)
        if time.monotonic() > deadline:
            for p in procs.processes:
                p.kill()
            pytest.fail("the two-rank workers did not finish in 300 s")
    return [np.load(os.path.join(out_dir, f"rank{r}.npz")) for r in range(2)]


def _same_words(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("segment", [256, 64])
def test_two_rank_sparse_merge_equals_dense_bit_for_bit(two_rank_results, segment):
    """Rank 0 observed the segments with s % 4 == 0, rank 1 those with s % 3 == 0: half of the segments are in the union, a twelfth on both ranks."""
    r0, r1 = two_rank_results
    active, segments = (int(v) for v in r0[f"stats_{segment}"])
    assert segments == -(-24 * 20 * 21 // segment) and 0.4 <= active / segments <= 0.6
    assert np.array_equal(r0[f"stats_{segment}"], r1[f"stats_{segment}"])
    dense = r0[f"dense_{segment}"]
    assert (dense[1] > 5).any(), "some voxels were summed over both ranks"
    for got in (r0[f"sparse_{segment}"], r1[f"sparse_{segment}"], r1[f"dense_{segment}"]):
        assert _same_words(got, dense)


def test_two_rank_dynamic_path_sparse_equals_dense(two_rank_results):
    r0, r1 = two_rank_results
    for name in ("bg", "fg"):
        assert (r0[f"{name}_dense"][1] > 0).any(), name
        for got in (r0[f"{name}_sparse"], r1[f"{name}_sparse"], r1[f"{name}_dense"]):
            assert _same_words(got, r0[f"{name}_dense"]), name
    active, segments = (int(v) for v in r0["fg_stats_sparse"])
    assert 0 < active < segments, "the foreground volume holds a few objects: most of its segments stay home"
